"""Launch trace of the native path: which launcher ``_ext.call`` issued, in
which order, with which shapes and integers.

:func:`trace` wraps ``_ext.call`` for the duration of a block and records one
entry per launch: ``[name, arg, arg, ...]`` with every ``i`` / ``f`` / ``d``
argument by value and every ``p`` argument as ``None``, ``[shape, dtype]`` (a
tensor) or ``"ptr"`` (a raw integer / ctypes object).  No stream, no address.
The two launchers that read a host-built table (``mda_wgrad_reduce_multi``,
``mda_pack_conv_weights_multi``) also record the table's non-pointer columns.

Only launches are recorded (launchers that take a stream).  The host-side
queries (``mda_conv_plan``, ``mda_wgrad_plan``, ``mda_pack_tiles``,
``mda_bn_region_bytes``, ...) sit behind per-process memo tables, so whether
one is issued depends on what ran earlier in the process; their results are
integer arguments of the launches that follow and are pinned there.

:data:`SCENARIOS` / :func:`run_scenario` are the training steps whose traces
``tests/golden/launch_traces.json`` pins (``scripts/record_launch_trace.py``
writes it, ``tests/test_gpu_launch_trace.py`` replays it).
"""
import contextlib
import ctypes
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_traces.json")

_DT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64", torch.int32: "i32",
       torch.int64: "i64", torch.uint8: "u8", torch.float16: "f16", torch.bool: "b8"}


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return [list(a.shape), _DT.get(a.dtype, str(a.dtype))]
    return "ptr"


# the packed-weight table lives on the device: read it back once, outside a
# capture (PackCache never rebuilds it inside one), and reuse that copy
_PACK_TABLES: dict = {}


def _pack_table(t):
    """Non-pointer columns of a ``mda_pack_conv_weights_multi`` table.  Row =
    [src, dst, wt | flag, Cout | n, kind | Cin, KH, KW, Kp, KpT, first tile]."""
    key = (t.data_ptr(), t.shape[0])
    rows = _PACK_TABLES.get(key)
    if rows is None:
        if torch.cuda.is_current_stream_capturing():
            return "unseen"
        rows = _PACK_TABLES[key] = t.cpu().tolist()
    out = []
    for r in rows:
        kind = r[4]
        if kind == -3:      # zero fill: [ptr, bytes, ...]
            out.append([r[1]] + r[2:])
        elif kind == -4:    # image pad: [src, dst, dtype flag, ...]
            out.append(r[2:])
        else:               # a layer: [w, wf, wt or 0, ...]
            out.append([int(r[2] != 0)] + r[3:])
    return out


def _reduce_table(t, n):
    """Non-pointer columns of a ``mda_wgrad_reduce_multi`` table (row =
    [partials, target, splits, Cout, Cin, KH, KW, Kp, ...])."""
    return [r[2:] for r in t[:n].tolist()]


@contextlib.contextmanager
def trace():
    """-> list that fills with one entry per native launch inside the block."""
    from mdistiller_ddp_amd.ops import _ext
    real = _ext.call
    out = []

    def call(name, *args, **kw):
        codes = _ext.SIGNATURES[name]
        if codes.endswith("s"):
            rec = [name] + [_ptr(a) if c == "p" else (int(a) if c == "i" else float(a))
                            for a, c in zip(args, codes)]
            if name == "mda_pack_conv_weights_multi":
                rec.append(_pack_table(args[0]))
            elif name == "mda_wgrad_reduce_multi":
                rec.append(_reduce_table(args[0], args[1]))
            out.append(rec)
        return real(name, *args, **kw)

    _ext.call = call
    try:
        yield out
    finally:
        _ext.call = real


# name -> (distiller, student, trainer, use_graph, deterministic, extra).  Batch 8,
# 32 x 32 inputs, a random resnet32x4 teacher; the first three steps (eager
# warm-up, capture, replay).  Together they issue every arm of the train-path
# host layer (ops/hip_train.py) at least once.
SCENARIOS = {
    "dkd_res8x4_graph": ("DKD", "resnet8x4", "base", True, False, None),
    "dkd_res8x4_eager": ("DKD", "resnet8x4", "base", False, False, None),
    "dkd_res8x4_deterministic": ("DKD", "resnet8x4", "base", True, True, None),
    "fitnet_res8x4": ("FITNET", "resnet8x4", "base", True, False, None),
    "vanilla_wrn_16_2": ("NONE", "wrn_16_2", "base", True, False, None),
    "dkd_shuv1": ("DKD", "ShuffleV1", "base", True, False, None),
    "dkd_shuv1_blockdiag": ("DKD", "ShuffleV1", "base", True, False, "blockdiag"),
    "dkd_mv2": ("DKD", "MobileNetV2", "base", True, False, None),
    "dot_res8x4": ("KD", "resnet8x4", "dot", True, False, None),
    "dot_vgg8": ("KD", "vgg8", "dot", True, False, None),
    "dot_mv2_single": ("KD", "MobileNetV2", "dot", True, False, "single"),
}

# launchers a scenario must issue: the arms it is there for
REQUIRED = {
    "dkd_res8x4_graph": ("mda_conv1x1_bnacc_apply", "mda_bn_apply_fin_vr", "mda_conv_wgrad_nored_bn",
                         "mda_conv_dgrad_bnsum2", "mda_wgrad_reduce_multi", "mda_conv_dgrad_res",
                         "mda_conv_dgrad", "mda_pack_conv_weights_pad"),
    "dkd_res8x4_eager": ("mda_conv_wgrad",),
    "dkd_res8x4_deterministic": ("mda_conv_fwd_bnstats", "mda_bn_bwd_reduce2", "mda_bn_bwd_apply"),
    "fitnet_res8x4": ("mda_bn_bwd_fused",),
    "vanilla_wrn_16_2": ("mda_conv_fwd", "mda_conv_dgrad", "mda_bn_stats_acc", "mda_act_bwd",
                         "mda_pack_conv_weights_pad"),
    "dkd_shuv1": ("mda_pack_conv_weights_gc",),
    "dkd_shuv1_blockdiag": ("mda_pack_conv_weights_grouped",),
    "dkd_mv2": ("mda_dw_fwd_bnacc", "mda_dw_dgrad", "mda_dw_wgrad"),
    "dot_res8x4": ("mda_conv_dgrad_bnsum_g", "mda_conv_wgrad_nored", "mda_pool_fc_bwd_bn"),
    "dot_vgg8": ("mda_conv_dgrad_res", "mda_conv_wgrad_nored", "mda_maxpool_bwd"),
    "dot_mv2_single": ("mda_dw_wgrad", "mda_dw_dgrad", "mda_conv_dgrad_bnsum_g"),
}


def run_scenario(name):
    """Build the scenario's distiller and step, trace its first three steps."""
    from mdistiller_ddp_amd.config import get_cfg
    from mdistiller_ddp_amd.data.synthetic import SyntheticLoader
    from mdistiller_ddp_amd.engine.build import build_distiller
    from mdistiller_ddp_amd.engine.step import TrainStep
    from mdistiller_ddp_amd.ops import hip_train
    typ, student, trainer, graph, det, extra = SCENARIOS[name]
    cfg = get_cfg()
    cfg.DISTILLER.TYPE = typ
    cfg.DISTILLER.TEACHER = "resnet32x4"
    cfg.DISTILLER.STUDENT = student
    cfg.DISTILLER.RANDOM_TEACHER = True
    cfg.SOLVER.TRAINER = trainer
    cfg.EXPERIMENT.DETERMINISTIC = det
    if extra == "single":
        cfg.RUNTIME.DOT_SINGLE_PASS = "true"
    # the BN arena sizes the step's zero fill by the largest demand the process
    # has seen: start every scenario from a fresh process's value
    for a in hip_train._ARENAS.values():
        a.high = 64 << 10
    torch.manual_seed(0)
    if extra == "blockdiag":
        hip_train.set_grouped_compact(False)
        hip_train.set_grouped_native(True)
    try:
        d = build_distiller(cfg, 100, "cuda")
        d.train()
        # one eager warm-up step, so the three traced steps are eager, capture, replay
        st = TrainStep(d, cfg, "cuda", trainer=trainer, use_graph=graph, dtype=torch.bfloat16,
                       warmup_eager=1)
        st.set_epoch(1.0)
        ld = SyntheticLoader("cifar100", 8, "cuda", steps_per_epoch=3, channels_last=True)
        with trace() as calls:
            for b in ld:
                st.step(b)
            torch.cuda.synchronize()
        assert (st._graphs is not None) == graph, name
        if extra == "single":
            assert st.dot_single
    finally:
        hip_train.set_deterministic(False)
        if extra == "blockdiag":
            hip_train.set_grouped_compact(True)
            hip_train.set_grouped_native(False)
    return calls


def encode(traces):
    """{scenario: calls} -> the golden file's form: every distinct call once
    (``calls``), each scenario a list of indices into it."""
    index, calls, seqs = {}, [], {}
    for name, tr in traces.items():
        seq = []
        for rec in tr:
            key = json.dumps(rec, separators=(",", ":"))
            i = index.get(key)
            if i is None:
                i = index[key] = len(calls)
                calls.append(rec)
            seq.append(i)
        seqs[name] = seq
    return {"calls": calls, "scenarios": seqs}


def decode(gold):
    return {name: [gold["calls"][i] for i in seq] for name, seq in gold["scenarios"].items()}


def load_golden():
    with open(GOLDEN) as f:
        return decode(json.load(f))
