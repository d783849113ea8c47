"""The kernels every training step ends with, against float64 references at
their edge shapes: fused logit loss + axpby (``csrc/losses.hip``), flat
optimizers + norm + multi-copy (``csrc/optim.hip``), meters
(``csrc/head.hip::meters_kernel``).  References and cases: ``tests/_step_tail.py``
(checked on the CPU by ``test_step_tail_refs_cpu.py``).

Which test reaches what
-----------------------
logit_loss_kernel
  NPL = 2 / 4 / 8 / 16 / 32, fp32 and bf16, KD and DKD ... test_logit_loss_grid
      (C = 2..128 / 129 / 300, 512 / 1000 / 1025, 2048; boundaries 64|65, 128|129)
  last-arriver stride loop (> 64 blocks, partial last block) test_logit_loss_grid, B = 257, 1027
  workspace full at B = 8192, C = 65 ....................... test_logit_loss_limit_and_axpby_grid_stride
  dispatch limits B = 8193, C = 2049 -> PyTorch fallback ... test_logit_loss_fallback_beyond_limits
  bf16 student + fp32 teacher, fp32 student + bf16 teacher . test_logit_loss_mixed_dtypes
  MODE_CE against a reference .............................. test_ce_alone
  zero-CE wrappers ......................................... test_zero_ce_wrappers
  confident (right / wrong) student, student + teacher ..... test_logit_loss_extreme_logits
  counter reset between grids of different size ............ test_counter_resets_between_launches
  g_sum (through the registered unit seed) ................. every test above that takes gradients
axpby_kernel grid-stride loop (> 2048 blocks), a, b, a+b ... test_logit_loss_limit_and_axpby_grid_stride
sgd_kernel / adam_kernel / dot_kernel grid-stride loops,
  sq_norm_kernel loop + 512-partial final pass ............. test_optimizers_large_buffer_vs_float64
FlatOptimizer.set_active (sub-range launches) .............. test_set_active_hip
state_dict round trip ...................................... test_checkpoint_round_trip_bitwise
multi_copy_kernel: vector path, byte tail, byte-only path,
  block table with an empty pair, 1 / 16 / 17 pairs ........ test_multi_copy_*
meters_kernel: B x C x dtype x nloss x ties ................ test_meters_grid

fp32 PyTorch backend against the float64 references, on the CPU, same inputs
(``test_step_tail_refs_cpu.py`` re-measures and asserts these):
  losses, error / scale (tolerance 1e-4): grid + mixed + limit + fallback +
      counter cases: KD 8.0e-7, DKD 8.1e-7; extreme logits, KD: 2.6e-7 (student),
      1.9e-43 (both), 1.9e-7 (wrong); extreme logits, DKD: not finite
      (``dkd_loss_ref`` takes log(0)), only the float64 value exists there.
  optimizers, error / tolerance (atol = rtol = 1e-5) after four steps on the
      1 049 728-element buffer: sgd 0.015, sgd_clip 0.014, adam 0.014,
      adamw 0.023, adam + clip 0.014, dot 0.018.
Gradients are compared at atol = tol * max|reference gradient| (floored at
ce_w / B, ``_step_tail.grad_unit``), never at tol * 1: at B = 1027 the
gradients are 1e-3 and smaller.
"""
import contextlib

import pytest
import torch

from tests import _step_tail as R
from mdistiller_ddp_amd.ops import _ext
from mdistiller_ddp_amd.ops import losses as L
from mdistiller_ddp_amd.ops.backend import use_backend

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = R.F32, R.BF16
DTYPES = [F32, BF16]


@contextlib.contextmanager
def launches():
    """Names of the native launchers called inside the block."""
    names, orig = [], _ext.call

    def rec(name, *a, **k):
        names.append(name)
        return orig(name, *a, **k)

    _ext.call = rec
    try:
        yield names
    finally:
        _ext.call = orig


@pytest.fixture(scope="module")
def unit():
    u = torch.ones((), device=DEV)
    L.register_unit_seed(u)
    return u


def _fwd(kind, s, t, y, hp):
    if kind == "kd":
        return L.ce_kd(s, t, y, hp["T"], hp["ce_w"], hp["kd_w"])
    return L.ce_dkd(s, t, y, hp["ce_w"], hp["alpha"], hp["beta"], hp["T"])


def hip_all(kind, s, t, y, hp, unit, native=True):
    """(ce, kd, g_ce, g_kd, g_sum) of the fused path.  With the registered unit
    seed the backward hands out the kernel's own g_ce / g_kd / g_sum buffers
    and launches nothing."""
    s = s.to(DEV).requires_grad_(True)
    t, y = t.to(DEV), y.to(DEV)
    with use_backend("hip"), launches() as names:
        ce, kd = _fwd(kind, s, t, y, hp)
        assert names.count("mda_logit_loss") == (1 if native else 0), names
        gce, = torch.autograd.grad(ce, s, unit, retain_graph=True)
        gkd, = torch.autograd.grad(kd, s, unit, retain_graph=True)
        gsum, = torch.autograd.grad([ce, kd], s, [unit, unit], retain_graph=True)
        if native:
            assert "mda_axpby" not in names, names
            assert gce.dtype == s.dtype and gsum.dtype == s.dtype
    return (ce, kd, gce, gkd, gsum), (s, ce, kd)


def check(kind, inputs, hp, unit, tol=None, native=True):
    s, t, y = inputs
    got, graph = hip_all(kind, s, t, y, hp, unit, native)
    tol = tol or R.TOL[s.dtype]
    R.assert_loss_close(got, R.ref_all(kind, s, t, y, hp), tol, R.grad_unit(hp, s.shape[0]))
    return graph


# ---- logit loss ------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C", R.GRID)
@pytest.mark.parametrize("kind", ["kd", "dkd"])
def test_logit_loss_grid(kind, B, C, dtype, unit):
    check(kind, R.loss_inputs(B, C, dtype), R.HP[kind], unit)


@pytest.mark.parametrize("kind", ["kd", "dkd"])
def test_logit_loss_limit_and_axpby_grid_stride(kind, unit):
    """B = 8192: 2048 blocks fill the 4096-float workspace.  Its 532 480
    gradient elements take axpby past the 2048-block cap, with ordinary seeds
    of different values."""
    hp = R.HP[kind]
    inputs = R.loss_inputs(*R.LIMIT)
    s, ce, kd = check(kind, inputs, hp, unit)
    _, _, gce, gkd, _ = R.ref_all(kind, *inputs, hp)
    a, b = torch.tensor(0.7, device=DEV), torch.tensor(-1.3, device=DEV)
    with use_backend("hip"), launches() as names:
        g_ab, = torch.autograd.grad([ce, kd], s, [a, b], retain_graph=True)
        g_a, = torch.autograd.grad(ce, s, a, retain_graph=True)
        g_b, = torch.autograd.grad(kd, s, b)
    assert names == ["mda_axpby"] * 3
    assert s.numel() > 2048 * 256
    unit_g = R.grad_unit(hp, s.shape[0])
    for got, ref in ((g_ab, 0.7 * gce - 1.3 * gkd), (g_a, 0.7 * gce), (g_b, -1.3 * gkd)):
        scale = max(ref.abs().max().item(), unit_g)
        torch.testing.assert_close(got.cpu().double(), ref, atol=1e-4 * scale, rtol=1e-4)


@pytest.mark.parametrize("B,C", R.FALLBACK)
@pytest.mark.parametrize("kind", ["kd", "dkd"])
def test_logit_loss_fallback_beyond_limits(kind, B, C, unit):
    """One row or one class past the kernel's limits: no launch, PyTorch math."""
    check(kind, R.loss_inputs(B, C), R.HP[kind], unit, native=False)


@pytest.mark.parametrize("ds,dt", R.MIXED, ids=["bf16s_fp32t", "fp32s_bf16t"])
@pytest.mark.parametrize("kind", ["kd", "dkd"])
def test_logit_loss_mixed_dtypes(kind, ds, dt, unit):
    check(kind, R.loss_inputs(*R.MIXED_SHAPE, ds, dt), R.HP[kind], unit)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C", R.CE_SHAPES)
def test_ce_alone(B, C, dtype, unit):
    """MODE_CE: value, stored gradient (unit seed) and scaled gradient."""
    s0, _, y = R.loss_inputs(B, C, dtype)
    s = s0.to(DEV).requires_grad_(True)
    with use_backend("hip"), launches() as names:
        ce = L.ce(s, y.to(DEV), 0.7)
        g1, = torch.autograd.grad(ce, s, unit, retain_graph=True)
        assert names == ["mda_logit_loss"]
        g2, = torch.autograd.grad(ce, s, torch.tensor(0.5, device=DEV))
        assert names == ["mda_logit_loss", "mda_axpby"]
    s64 = s0.double().requires_grad_(True)
    ref = 0.7 * R.ce64(s64, y)
    gref, = torch.autograd.grad(ref, s64)
    tol = R.TOL[dtype]
    torch.testing.assert_close(ce.cpu().double(), ref.detach(), atol=tol * max(1.0, ref.item()), rtol=tol)
    for g, r in ((g1, gref), (g2, 0.5 * gref)):
        assert g.dtype == dtype
        torch.testing.assert_close(g.cpu().double(), r, atol=tol * r.abs().max().item(), rtol=tol)


def test_zero_ce_wrappers():
    s, t, y = R.loss_inputs(33, 100)
    with use_backend("hip"), launches() as names:
        kd = L.kd_loss(s.to(DEV), t.to(DEV), 4.0)
        dkd = L.dkd_loss(s.to(DEV), t.to(DEV), y.to(DEV), 1.0, 8.0, 4.0)
    assert names == ["mda_logit_loss"] * 2
    torch.testing.assert_close(kd.cpu().double(), R.kd64(s, t, 4.0), atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(dkd.cpu().double(), R.dkd64(s, t, y, 1.0, 8.0, 4.0), atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C,gap,T", R.EXTREME)
@pytest.mark.parametrize("where", R.EXTREME_WHERE)
@pytest.mark.parametrize("kind", ["kd", "dkd"])
def test_logit_loss_extreme_logits(kind, where, B, C, gap, T, dtype, unit):
    """Near-one-hot student (right or wrong class), alone and together with a
    near-one-hot teacher.  The fp32 PyTorch DKD evaluates log(0) here; the
    float64 reference is finite, and so must every kernel output be
    (assert_loss_close checks finiteness first)."""
    hp = dict(R.HP[kind], T=T)
    check(kind, R.loss_inputs(B, C, dtype, gap=gap, where=where), hp, unit)


@pytest.mark.parametrize("kind", ["kd", "dkd"])
def test_counter_resets_between_launches(kind, unit):
    """257, 2 and 65 blocks back to back on one stream: the arrival counter
    must be back at zero after each grid, whatever its size."""
    hp = R.HP[kind]
    cases = [R.loss_inputs(B, 100) for B in R.COUNTER_BS]
    outs = [hip_all(kind, s, t, y, hp, unit)[0] for s, t, y in cases]   # no sync in between
    for (s, t, y), got in zip(cases, outs):
        R.assert_loss_close(got, R.ref_all(kind, s, t, y, hp), 1e-4, R.grad_unit(hp, s.shape[0]))
    assert int(L.workspace(DEV).counter[0]) == 0


# ---- optimizers --------------------------------------------------------------

@pytest.mark.parametrize("kind", R.OPT_KINDS)
def test_optimizers_large_buffer_vs_float64(kind):
    """Four steps, changing lr, on a buffer past every grid cap, against
    torch.optim (+ clip_grad_norm_) / the DOT transcription in float64; the
    params are compared after every step (DOT: the ``first`` one included),
    ``norm_t`` too for the clip kinds."""
    per_step = []
    with use_backend("hip"), launches() as names:
        worst = R.run_flat_vs_torch64(kind, DEV, R.BIG, on_step=lambda it, w: per_step.append(w))
    kernel = {"sgd": "mda_sgd_step", "adam": "mda_adam_step", "dot": "mda_dot_step"}[kind.split("_")[0].replace("adamw", "adam")]
    assert names.count(kernel) == 4
    assert names.count("mda_sq_norm") == (4 if kind.endswith("clip") else 0)
    print(f"{kind}: error / tolerance after each step: {per_step}")
    assert worst <= 1.0, per_step


@pytest.mark.parametrize("pattern", sorted(R.ACTIVE_PATTERNS))
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_set_active_hip(kind, pattern):
    with use_backend("hip"), launches() as names:
        R.check_set_active(kind, pattern, DEV)
    # one launch with every param active, then two ranges for three steps
    assert names.count(f"mda_{kind}_step") == 1 + 3 * 2


@pytest.mark.parametrize("kind", ["sgd_clip", "adam", "dot"])
def test_checkpoint_round_trip_bitwise(kind):
    sizes = (1000, 37, 4096)
    g = torch.Generator().manual_seed(11)
    with use_backend("hip"):
        pa = R.make_params(sizes, DEV, seed=9)
        fa, oa = R.make_flat_opt(kind, pa)
        if kind == "dot":
            oa.set_reachability([True, True, False], [True, False, True])

        def step(pairs, it):
            grads = R.random_grads(pairs[0][0], g).to(DEV)
            for f, o in pairs:
                f.grads.copy_(grads)
                o.set_lr(R.base_lr(kind) / (it + 1))
                o.step()

        for it in range(2):
            step([(fa, oa)], it)
        sd = oa.state_dict()
        pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
        fb, ob = R.make_flat_opt(kind, pb)
        ob.load_state_dict(sd)
        for it in range(2, 4):
            step([(fa, oa), (fb, ob)], it)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    state = {"sgd_clip": ["buf"], "adam": ["m1", "m2", "step_t"], "dot": ["buf_t", "buf_k", "mask"]}[kind]
    for name in state:
        sa, sb = getattr(oa, name), getattr(ob, name)
        if sa.numel() == fa.numel:
            for p, off in zip(fa.params, fa.offsets):
                assert torch.equal(sa[off:off + p.numel()], sb[off:off + p.numel()]), name
        else:
            assert torch.equal(sa, sb), name


# ---- multi-copy --------------------------------------------------------------

SENTINEL = 0xA5
CHUNK = 256 * 16 * 4   # bytes per block of multi_copy_kernel
# (dtype, elements, source byte offset, destination byte offset); offsets are
# relative to a 256-byte aligned base
PAIRS = [
    (torch.uint8, 1, 0, 0),                         # one byte: tail only
    (torch.uint8, 15, 0, 16),                       # below one vector
    (torch.float32, (CHUNK + 20) // 4, 0, 0),       # > one chunk, not a multiple of 16 bytes
    (torch.int64, 2 * CHUNK // 8, 16, 32),          # exact multiple of the chunk
    (torch.float32, 0, 0, 0),                       # empty pair in the middle of the block table
    (torch.bfloat16, 1001, 2, 2),                   # both ends 2-byte aligned only: byte path
    (torch.uint8, 40000, 1, 0),                     # source at an odd byte: byte path over 3 chunks
    (torch.uint8, 777, 0, 3),                       # only the destination misaligned
    (torch.float32, CHUNK // 4, 0, 0),              # exactly one chunk
    (torch.int64, 3, 0, 0),                         # one vector + 8-byte tail
    (torch.bfloat16, 8, 0, 0),                      # exactly one vector
    (torch.uint8, CHUNK + 1, 0, 0),                 # one chunk + a one-byte block
    (torch.bfloat16, 4097, 16, 0),
    (torch.float32, 5, 4, 4),                       # 4-byte aligned only
    (torch.int64, 1, 8, 8),                         # 8-byte aligned only
    (torch.uint8, 0, 0, 0),                         # empty pair at the end
    (torch.uint8, 33, 0, 0),                        # the 17th
]


def _run_multi_copy(pairs, expect_native):
    from mdistiller_ddp_amd.engine.step import _multi_copy
    g = torch.Generator().manual_seed(len(pairs))
    pad = 64
    raws, dsts, srcs, spans = [], [], [], []
    for dtype, n, so, do in pairs:
        nb = n * dtype.itemsize
        rs = torch.randint(0, 256, (so + nb + pad,), generator=g, dtype=torch.uint8).to(DEV)
        rd = torch.full((pad + do + nb + pad,), SENTINEL, dtype=torch.uint8, device=DEV)
        assert rs.data_ptr() % 256 == 0 and rd.data_ptr() % 256 == 0
        # pad is a multiple of 16, so `do` alone decides the destination's alignment
        srcs.append(rs[so:so + nb].view(dtype))
        dsts.append(rd[pad + do:pad + do + nb].view(dtype))
        raws.append((rs, rd))
        spans.append((so, pad + do, nb))
    with launches() as names:
        _multi_copy(dsts, srcs)
    assert names == (["mda_multi_copy"] if expect_native else []), names
    for (rs, rd), (so, do, nb) in zip(raws, spans):
        assert torch.equal(rd[do:do + nb], rs[so:so + nb])
        assert bool((rd[:do] == SENTINEL).all()) and bool((rd[do + nb:] == SENTINEL).all())


def test_multi_copy_16_pairs():
    _run_multi_copy(PAIRS[:16], True)


@pytest.mark.parametrize("i", range(len(PAIRS)))
def test_multi_copy_single_pair(i):
    _run_multi_copy([PAIRS[i]], True)


def test_multi_copy_17_pairs_take_foreach_copy():
    _run_multi_copy(PAIRS, False)


# ---- meters --------------------------------------------------------------------

@pytest.mark.parametrize("ties", [False, True], ids=["noties", "ties"])
@pytest.mark.parametrize("nloss", [0, 1, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 100, 1000])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_meters_grid(B, C, dtype, nloss, ties):
    from mdistiller_ddp_amd.engine.step import DeviceMeters
    g = torch.Generator().manual_seed(R._seed(B, C, nloss, ties))
    keys = [f"loss_{i}" for i in range(nloss)]
    m_h, m_r = DeviceMeters(DEV, keys), DeviceMeters(DEV, keys)
    for _ in range(3):
        if ties:  # heavy ties with the target logit: stable-order rank, not a free hit
            preds = torch.randint(0, 3, (B, C), generator=g).to(dtype).to(DEV)
        else:
            preds = torch.randn(B, C, generator=g).to(dtype).to(DEV)
        target = torch.randint(0, C, (B,), generator=g).to(DEV)
        losses = {k: torch.rand((), generator=g).to(DEV) for k in keys}
        with use_backend("hip"), launches() as names:
            m_h.update(preds, target, losses)
        assert names == ["mda_meters_update"]
        with use_backend("torch"):
            m_r.update(preds, target, losses)
    torch.testing.assert_close(m_h.buf, m_r.buf, rtol=1e-12, atol=1e-9)
    top1, top5, samples, steps = m_h.buf[nloss + 1:].tolist()
    assert (samples, steps) == (3 * B, 3) and top1 <= top5 <= samples
    if C == 5:
        assert top5 == 3 * B   # every class is inside the top five
