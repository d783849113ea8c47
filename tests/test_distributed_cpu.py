"""Data parallelism on CPU with the gloo backend (2 ranks, spawned processes).

Checks the properties the reference's DDP setup gets wrong (SURVEY D4, D5,
D10, D15) plus plain DP correctness:
* parameters stay bit-identical across ranks after several steps (base, DOT, CRD);
* the all-reduced gradient equals the mean of the per-rank gradients;
* only student + distiller-module gradients go on the wire (no teacher);
* DOT reduces BOTH gradient sets;
* CRD memory banks stay identical across ranks;
* global rank is RANK, not LOCAL_RANK (multi-node simulation);
* ranks seeded differently start identical (rank-0 broadcast, DDP's C2);
* gradient buckets launch from inside backward (overlap) after calibration;
* BN buffer sync before eval reproduces DDP's broadcast_buffers semantics.
"""
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _all_equal(dist, world, t):
    allt = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(allt, t.contiguous())
    return all(torch.equal(allt[0], a) for a in allt)


def _worker(rank, world, port, scenario, outdir, local_rank_offset):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world),
                      RANK=str(rank), LOCAL_RANK=str((rank + local_rank_offset) % world),
                      MDA_BACKEND="torch")
    torch.set_num_threads(1)
    from mdistiller_ddp_amd.config import get_cfg
    from mdistiller_ddp_amd.parallel import dist as D
    from mdistiller_ddp_amd.engine.build import build_distiller
    from mdistiller_ddp_amd.engine.step import TrainStep
    from mdistiller_ddp_amd.data.synthetic import SyntheticLoader
    import torch.distributed as dist

    info = D.init_distributed("gloo", 60.0, device="cpu")
    assert info.rank == rank and dist.get_rank() == rank
    typ, trainer = {"base": ("KD", "base"), "dot": ("KD", "dot"), "crd": ("CRD", "crd"),
                    "dkd": ("DKD", "base")}[scenario]
    cfg = get_cfg()
    cfg.DISTILLER.TYPE = typ
    cfg.DISTILLER.TEACHER = "resnet20"
    cfg.DISTILLER.STUDENT = "resnet8"
    cfg.DISTILLER.RANDOM_TEACHER = True
    cfg.SOLVER.TRAINER = trainer
    cfg.CRD.NCE.K = 32
    cfg.CRD.FEAT.STUDENT_DIM = 64
    cfg.CRD.FEAT.TEACHER_DIM = 64
    cfg.DIST.BUCKET_MB = 0.05  # several buckets even for a tiny student
    # DIFFERENT init on every rank: TrainStep's rank-0 broadcast (DDP's C2)
    # must make the replicas identical anyway
    torch.manual_seed(100 + rank)
    d = build_distiller(cfg, 100, "cpu", num_data=200)
    d.train()
    keys = ("image", "target", "index", "contrastive_index") if typ == "CRD" else ("image", "target")
    st = TrainStep(d, cfg, "cpu", trainer=trainer, dtype=torch.float32, batch_keys=keys)
    from mdistiller_ddp_amd.parallel import state_checksum
    c0 = state_checksum(d, st.flat, buffers=True)
    g0 = [torch.empty_like(c0) for _ in range(world)]
    dist.all_gather(g0, c0)
    init_equal = all(torch.equal(g0[0], g) for g in g0)
    st.set_epoch(1.0)
    # different data per rank
    ld = SyntheticLoader("cifar100", 8, "cpu", steps_per_epoch=3, crd_k=32, num_data=200, seed=rank)
    if typ == "CRD":  # distinct dataset indices across ranks (a sharded sampler's guarantee)
        for i, b in enumerate(ld.batches):
            b["index"] = torch.arange(8) + 8 * (2 * i + rank) % 200
            b["contrastive_index"][:, 0] = b["index"]
    grads_ok = True
    for b in ld:
        st.step(b)
    flat = st.flat.data.clone()
    gathered = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    out = {"params_equal": all(torch.equal(gathered[0], g) for g in gathered),
           "init_equal": init_equal, "early": st.reducer.early_launches,
           "teacher_equal": _all_equal(dist, world, torch.cat(
               [p.detach().reshape(-1) for p in d.teacher.parameters()])),
           "bytes": st.reducer.bytes_reduced, "calls": st.reducer.calls,
           "student_bytes": 4 * sum(p.numel() for p in d.get_learnable_parameters()),
           "flat_bytes": 4 * st.flat.numel * st.flat.num_grad_sets}
    if typ == "CRD":
        m = d.contrast.memory_v1.clone()
        gm = [torch.empty_like(m) for _ in range(world)]
        dist.all_gather(gm, m)
        out["memory_equal"] = all(torch.equal(gm[0], g) for g in gm)
    # DP gradient correctness: reduced grad == mean of local grads
    if scenario == "base":
        st.flat.zero_grad()
        b = ld.batches[0]
        preds, losses = st._forward({"image": b["image"], "target": b["target"]})
        sum(losses.values()).backward()
        local = st.flat.grads[0].clone()
        allg = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(allg, local)
        st.reducer.reduce_all()
        reduced = st.flat.grads[0] / world
        out["grad_mean_ok"] = torch.allclose(reduced, torch.stack(allg).mean(0), atol=1e-6, rtol=1e-5)
    # BN buffer sync (rank 0's running stats everywhere)
    from mdistiller_ddp_amd.engine.trainer import BaseTrainer
    BaseTrainer.sync_buffers(type("T", (), {"distiller": d})())
    rm = d.student.bn1.running_mean.clone()
    grm = [torch.empty_like(rm) for _ in range(world)]
    dist.all_gather(grm, rm)
    out["bn_equal"] = all(torch.equal(grm[0], g) for g in grm)
    torch.save(out, os.path.join(outdir, f"r{rank}.pt"))
    D.destroy()


def _spawn(scenario, world=2, local_rank_offset=0):
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(world, _free_port(), scenario, td, local_rank_offset), nprocs=world,
                 join=True)
        return [torch.load(os.path.join(td, f"r{r}.pt"), weights_only=True) for r in range(world)]


@pytest.mark.parametrize("scenario", ["base", "dkd"])
def test_dp_replicas_identical(scenario):
    res = _spawn(scenario)
    for r in res:
        assert r["init_equal"]  # rank-0 broadcast at construction (C2)
        assert r["teacher_equal"]
        assert r["params_equal"]
        assert r["bn_equal"]
    # buckets launched from inside backward once the per-param gradient
    # counts are calibrated (step 1): steps 2 and 3 overlap comm with backward
    assert res[0]["early"] > 0
    r = res[0]
    # only student grads on the wire: 3 steps x flat buffer (+ the explicit reduce)
    assert r["bytes"] <= 4 * r["flat_bytes"]
    assert r["flat_bytes"] < 1.1 * r["student_bytes"] + 4 * 64 * 200
    assert r["calls"] >= 3
    if scenario == "base":
        assert r["grad_mean_ok"]


def test_dp_dot_reduces_both_grad_sets():
    res = _spawn("dot")
    assert all(r["params_equal"] for r in res)
    r = res[0]
    assert r["flat_bytes"] == 2 * 4 * (r["flat_bytes"] // 8)
    assert r["bytes"] == 3 * r["flat_bytes"]  # one call per step covering both sets


def test_dp_crd_memory_consistent():
    res = _spawn("crd")
    for r in res:
        assert r["init_equal"]  # incl. both memory banks, broadcast at construction
        assert r["params_equal"]
        assert r["memory_equal"]


def test_global_rank_is_rank_not_local_rank():
    # simulate a second node: LOCAL_RANK differs from RANK
    res = _spawn("base", local_rank_offset=1)
    assert all(r["params_equal"] for r in res)


def test_bench_self_launch_two_ranks_cpu():
    """``python bench.py --gpus 2`` launches 2 ranks itself and reports n_gpus 2
    (``--full``: the replica check is not part of a plain run)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.pop("WORLD_SIZE", None)
    for scaling, want_global in (("weak", 8), ("strong", 4)):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2",
                              "--steps", "1", "--warmup", "1", "--batch", "4", "--global-batch", "4",
                              "--scaling", scaling, "--full", "DISTILLER.STUDENT", "resnet8",
                              "DISTILLER.TEACHER", "resnet20"],
                             capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert out.returncode == 0, out.stderr[-3000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
        r = json.loads(line)
        assert r["n_gpus"] == 2 and r["scaling"] == scaling
        assert r["config"]["global_batch"] == want_global
        assert r["replicas_identical"] is True


def test_bench_refuses_mismatched_world():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="1")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"],
                         capture_output=True, text=True, timeout=300, env=env, cwd=root)
    assert out.returncode != 0 and "WORLD_SIZE" in (out.stderr + out.stdout)


def _crd_exchange_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world),
                      RANK=str(rank), LOCAL_RANK=str(rank), MDA_BACKEND="torch")
    torch.set_num_threads(1)
    import torch.distributed as dist
    from mdistiller_ddp_amd.parallel import dist as D
    from mdistiller_ddp_amd.distillers.CRD import ContrastMemory
    D.init_distributed("gloo", 60.0, device="cpu")
    torch.manual_seed(0)  # identical banks on every rank
    mem = ContrastMemory(16, 64, K=8)
    start = (mem.memory_v1.clone(), mem.memory_v2.clone())
    g = torch.Generator().manual_seed(7)
    rows = []
    # a full batch (B=4), then the epoch's partial last batch (B=3), then a full one:
    # each step stages its own rows, all-gathers them and applies every rank's in order
    for step, B in enumerate((4, 3, 4)):
        allv = [(torch.randn(B, 16, generator=g), torch.randn(B, 16, generator=g)) for _ in range(world)]
        ally = [torch.arange(B) + 8 * (step * world + r) for r in range(world)]
        rows.append((allv, ally))
        v1, v2 = allv[rank]
        mem._pending = (v1, v2, ally[rank])
        mem.apply_pending()
        mem.exchange()
        mem.apply_exchange()
    out = {"v1": mem.memory_v1.clone(), "v2": mem.memory_v2.clone(), "keys": len(mem._xbufs)}
    # single-process reference: the concatenated rows of every rank, in rank order
    from mdistiller_ddp_amd.ops import crd as CO
    r1, r2 = start[0].clone(), start[1].clone()
    for allv, ally in rows:
        y = torch.cat(ally)
        CO.update_ref(r1, y, torch.cat([a for a, _ in allv]), mem.momentum)
        CO.update_ref(r2, y, torch.cat([b for _, b in allv]), mem.momentum)
    out["ref_v1"], out["ref_v2"] = r1, r2
    out["start_v1"] = start[0]
    torch.save(out, os.path.join(outdir, f"r{rank}.pt"))
    D.destroy()


def test_crd_exchange_matches_single_process_update_with_partial_batch():
    """the gathered update equals a single-process update over the
    concatenated per-rank rows, and a partial batch gets its own buffers (the
    full-batch pair a captured graph was recorded against is never rebound)."""
    world = 2
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_crd_exchange_worker, args=(world, _free_port(), td), nprocs=world, join=True)
        res = [torch.load(os.path.join(td, f"r{r}.pt"), weights_only=True) for r in range(world)]
    for r in res:
        assert r["keys"] == 2  # B=4 and B=3 pairs, both kept
        assert not torch.equal(r["v1"], r["start_v1"])  # the bank really changed
        # fp64 staging + the same per-row arithmetic: equal to fp32 rounding
        assert torch.allclose(r["v1"], r["ref_v1"], atol=1e-6, rtol=0)
        assert torch.allclose(r["v2"], r["ref_v2"], atol=1e-6, rtol=0)
    assert torch.equal(res[0]["v1"], res[1]["v1"]) and torch.equal(res[0]["v2"], res[1]["v2"])
