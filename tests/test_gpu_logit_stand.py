"""Logit standardisation in the fused loss kernel (``mda_logit_loss_std``,
the STAND variant of ``csrc/losses.hip::logit_loss_kernel``) against float64.
References and cases: ``tests/_logit_stand.py`` (checked on the CPU by
``test_logit_stand_cpu.py``).

Which test reaches what
-----------------------
NPL = 2 / 4 / 16 / 32, KD and DKD, fp32 and bf16, T = 2 and 4,
  C = 2, one row, lane boundary 63 | 64 | 65, three blocks ... test_grid
bf16 student + fp32 teacher and the reverse ................. test_mixed_dtypes
sigma == 0 (k = 0), student row / teacher row ............... test_constant_row
warm-up factor from the device epoch tensor ................. test_dkd_warmup_follows_device_epoch
unit seeds, scaled seeds, which launcher runs ............... test_backward_plumbing
arrival counter + workspace across hipGraph replays ......... test_graph_replay
C = 2049 -> PyTorch path ..................................... test_fallback_beyond_limit
KD distiller with KD.LOGIT_STAND True ........................ test_kd_distiller

Gradients are compared row by row (``_logit_stand.row_errors``): each row is
scaled by its own largest reference gradient, floored at ce_w / B.

Measured on an MI355X, largest error / scale over this file: fp32 (tolerance
1e-4) loss 6.3e-6, gradients 9.3e-7; bf16 (tolerance 2e-2) loss 6.2e-6,
gradients 3.8e-3.
"""
import pytest
import torch

from tests import _logit_stand as S
from tests import _step_tail as R
from mdistiller_ddp_amd.ops import losses as L
from mdistiller_ddp_amd.ops.backend import use_backend

pytestmark = pytest.mark.gpu
launches = S.launches
DEV = "cuda"
F32, BF16 = R.F32, R.BF16
KINDS = ["kd", "dkd"]
STD, PLAIN = "mda_logit_loss_std", "mda_logit_loss"


@pytest.fixture(scope="module")
def unit():
    u = torch.ones((), device=DEV)
    L.register_unit_seed(u)
    return u


def _hp(kind, T):
    return dict(R.HP[kind], T=T)


def _fwd(kind, s, t, y, hp, stand=True, **kw):
    if kind == "kd":
        return L.ce_kd(s, t, y, hp["T"], hp["ce_w"], hp["kd_w"], logit_stand=stand)
    return L.ce_dkd(s, t, y, hp["ce_w"], hp["alpha"], hp["beta"], hp["T"], logit_stand=stand, **kw)


def hip_all(kind, s, t, y, hp, unit, native=True):
    """(ce, kd, g_ce, g_kd, g_sum) of the fused path with the switch on; with
    the unit seed the backward hands out the kernel's own buffers."""
    s = s.to(DEV).requires_grad_(True)
    t, y = t.to(DEV), y.to(DEV)
    with use_backend("hip"), launches() as names:
        ce, kd = _fwd(kind, s, t, y, hp)
        assert names == ([STD] if native else []), names
        gce, = torch.autograd.grad(ce, s, unit, retain_graph=True)
        gkd, = torch.autograd.grad(kd, s, unit, retain_graph=True)
        gsum, = torch.autograd.grad([ce, kd], s, [unit, unit], retain_graph=True)
        if native:
            assert names == [STD], names
            assert gce.dtype == s.dtype and gkd.dtype == s.dtype and gsum.dtype == s.dtype
    return (ce, kd, gce, gkd, gsum), (s, ce, kd)


def check(kind, inputs, hp, unit, native=True):
    s, t, y = inputs
    got, graph = hip_all(kind, s, t, y, hp, unit, native)
    S.assert_rows_close(got, S.ref_all(kind, s, t, y, hp), R.TOL[s.dtype], R.grad_unit(hp, s.shape[0]))
    return graph


@pytest.mark.parametrize("T", S.TEMPS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C", S.GRID)
@pytest.mark.parametrize("kind", KINDS)
def test_grid(kind, B, C, dtype, T, unit):
    check(kind, R.loss_inputs(B, C, dtype), _hp(kind, T), unit)


@pytest.mark.parametrize("ds,dt", S.MIXED, ids=["bf16s_fp32t", "fp32s_bf16t"])
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_dtypes(kind, ds, dt, unit):
    check(kind, R.loss_inputs(*S.MIXED_SHAPE, ds, dt), _hp(kind, 2.0), unit)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("who", ["student", "teacher"])
@pytest.mark.parametrize("kind", KINDS)
def test_constant_row(kind, who, dtype, unit):
    """One constant row beside two ordinary ones.  The student's constant row
    has z = 0, k = 0 and gradients of order T / (B * 1e-7); every row is held to
    its own scale."""
    hp = _hp(kind, 2.0)
    s, t, y = R.loss_inputs(*S.CONST_SHAPE, dtype)
    s, t = (S.with_constant_row(s), t) if who == "student" else (s, S.with_constant_row(t))
    if who == "student":
        g_ref = S.ref_all(kind, s, t, y, hp)[3]
        assert 1e4 < g_ref[1].abs().max() < 1e7 and g_ref[0].abs().max() < 10
    check(kind, (s, t, y), hp, unit)


def test_two_classes_gradient_is_zero(unit):
    """C == 2: z is (+-1/sqrt 2) whatever the logits are, so the KD gradient is
    analytically ~0 (well below the ce_w / B floor of the row scale)."""
    hp = _hp("kd", 2.0)
    s, t, y = R.loss_inputs(3, 2)
    got, _ = hip_all("kd", s, t, y, hp, unit)
    assert got[3].abs().max().item() < 1e-4 * R.grad_unit(hp, 3)


def test_dkd_warmup_follows_device_epoch(unit):
    hp = _hp("dkd", 4.0)
    s, t, y = R.loss_inputs(5, 65)
    ep = torch.tensor(5.0, device=DEV)
    sd = s.to(DEV).requires_grad_(True)
    full = S.ref_all("dkd", s, t, y, hp)
    with use_backend("hip"), launches() as names:
        for epoch, f in ((5.0, 0.25), (10.0, 0.5), (30.0, 1.0)):
            ep.fill_(epoch)
            ce, kd = _fwd("dkd", sd, t.to(DEV), y.to(DEV), hp, epoch=ep, warmup=20)
            g, = torch.autograd.grad(kd, sd, unit)
            S.assert_rows_close((ce, kd, g), (full[0], f * full[1], f * full[3]), 1e-4,
                                R.grad_unit(hp, 5), names=("ce", "kd", "g_kd"))
    assert names == [STD] * 3


@pytest.mark.parametrize("kind", KINDS)
def test_backward_plumbing(kind, unit):
    hp = _hp(kind, 2.0)
    inputs = R.loss_inputs(7, 100)
    s, ce, kd = check(kind, inputs, hp, unit)       # unit seeds: one launch, no axpby
    _, _, gce, gkd, _ = S.ref_all(kind, *inputs, hp)
    a, b = torch.tensor(0.7, device=DEV), torch.tensor(-1.3, device=DEV)
    with use_backend("hip"), launches() as names:
        g_ab, = torch.autograd.grad([ce, kd], s, [a, b], retain_graph=True)
        g_a, = torch.autograd.grad(ce, s, a, retain_graph=True)
        g_b, = torch.autograd.grad(kd, s, b)
    assert names == ["mda_axpby"] * 3
    S.assert_rows_close((g_ab, g_a, g_b), (0.7 * gce - 1.3 * gkd, 0.7 * gce, -1.3 * gkd), 1e-4,
                        R.grad_unit(hp, 7), names=("g_ab", "g_a", "g_b"))
    # the switch off: the plain launcher, and only it
    sd = inputs[0].to(DEV).requires_grad_(True)
    with use_backend("hip"), launches() as names:
        _fwd(kind, sd, inputs[1].to(DEV), inputs[2].to(DEV), hp, stand=False)
    assert names == [PLAIN]


def test_zero_ce_wrappers(unit):
    s, t, y = R.loss_inputs(5, 65)
    with use_backend("hip"), launches() as names:
        kd = L.kd_loss(s.to(DEV), t.to(DEV), 2.0, logit_stand=True)
        dkd = L.dkd_loss(s.to(DEV), t.to(DEV), y.to(DEV), 1.0, 8.0, 2.0, logit_stand=True)
    assert names == [STD] * 2
    zs, zt = S.standardize64(s), S.standardize64(t)
    for got, ref in ((kd, R.kd64(zs, zt, 2.0)), (dkd, R.dkd64(zs, zt, y, 1.0, 8.0, 2.0))):
        assert abs(got.item() - ref.item()) <= 1e-4 * max(1.0, abs(ref.item()))


def test_one_class_raises():
    s, t = torch.randn(3, 1, device=DEV), torch.randn(3, 1, device=DEV)
    y = torch.zeros(3, dtype=torch.long, device=DEV)
    with use_backend("hip"), launches() as names:
        with pytest.raises(ValueError):
            L.ce_kd(s, t, y, 4.0, 0.1, 0.9, logit_stand=True)
        with pytest.raises(ValueError):
            L.ce_dkd(s, t, y, 1.0, 1.0, 8.0, 4.0, logit_stand=True)
    assert names == []


def test_graph_replay(unit):
    """One captured forward + backward, replayed with new inputs: the arrival
    counter and the workspace are back in their start state after every
    launch, so each replay equals an eager call on the same inputs."""
    B, C = 9, 128
    hp = _hp("kd", 2.0)
    cases = [R.loss_inputs(B, C), R.loss_inputs(B, C, gap=3.0, where="student"),
             R.loss_inputs(B, C, gap=5.0, where="teacher")]
    ss = cases[0][0].to(DEV).requires_grad_(True)
    st, sy = cases[0][1].to(DEV), cases[0][2].to(DEV)
    a, b = torch.tensor(0.7, device=DEV), torch.tensor(-1.3, device=DEV)

    def run(s, t, y):
        ce, kd = _fwd("kd", s, t, y, hp)
        g_sum, = torch.autograd.grad([ce, kd], s, [unit, unit], retain_graph=True)
        g_ab, = torch.autograd.grad([ce, kd], s, [a, b])
        return ce, kd, g_sum, g_ab

    with use_backend("hip"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(ss, st, sy)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = run(ss, st, sy)
        for s, t, y in cases[1:]:
            with torch.no_grad():
                ss.copy_(s)
                st.copy_(t)
                sy.copy_(y)
            graph.replay()
            got = [o.clone() for o in outs]
            eager = run(s.to(DEV).requires_grad_(True), t.to(DEV), y.to(DEV))
            for n, g, e in zip(("ce", "kd", "g_sum", "g_ab"), got, eager):
                assert torch.equal(g, e), n
            S.assert_rows_close(got[:3], [S.ref_all("kd", s, t, y, hp)[i] for i in (0, 1, 4)], 1e-4,
                                R.grad_unit(hp, B), names=("ce", "kd", "g_sum"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", KINDS)
def test_fallback_beyond_limit(kind, unit):
    """One class past the kernel's limit: no launch, PyTorch math, same result."""
    check(kind, R.loss_inputs(4, 2049), _hp(kind, 2.0), unit, native=False)


def test_kd_distiller(monkeypatch):
    """KD.LOGIT_STAND True through the distiller: loss_kd is the float64 value
    on the logits the loss saw, and a backward reaches the student."""
    from mdistiller_ddp_amd.config import get_cfg
    from mdistiller_ddp_amd.engine.build import build_distiller
    seen = {}
    orig = L.ce_kd

    def rec(logits_s, logits_t, *a, **k):
        seen["t"] = logits_t.detach().clone()
        return orig(logits_s, logits_t, *a, **k)

    monkeypatch.setattr(L, "ce_kd", rec)
    cfg = get_cfg()
    cfg.DISTILLER.TYPE = "KD"
    cfg.DISTILLER.TEACHER = "resnet32x4"
    cfg.DISTILLER.STUDENT = "resnet8x4"
    cfg.DISTILLER.RANDOM_TEACHER = True
    cfg.merge_from_list(["KD.LOGIT_STAND", "True", "KD.TEMPERATURE", "2", "KD.LOSS.KD_WEIGHT", "9.0"])
    torch.manual_seed(0)
    d = build_distiller(cfg, 100, DEV)
    d.train()
    x = torch.randn(8, 3, 32, 32, device=DEV)
    y = R.forced_labels(torch.randint(0, 100, (8,)), 100).to(DEV)
    # a TrainStep built by an earlier test leaves cudnn.benchmark on; the
    # exhaustive search for this batch size would take most of a minute
    bench = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    try:
        with launches() as names:
            logits, losses = d.forward_train(image=x, target=y)
            (losses["loss_ce"] + losses["loss_kd"]).backward()
    finally:
        torch.backends.cudnn.benchmark = bench
    assert names.count(STD) == 1 and PLAIN not in names, names
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in d.student.parameters())
    ref = S.kd_term64("kd", logits.detach().cpu(), seen["t"].cpu(), y.cpu(), dict(T=2.0, kd_w=9.0))
    tol = R.TOL[logits.dtype]
    assert abs(losses["loss_kd"].item() - ref.item()) <= tol * max(1.0, abs(ref.item()))
