"""Float64 references and shared cases for the logit-standardisation tests
(``test_gpu_logit_stand.py`` on the GPU, ``test_logit_stand_cpu.py`` on the
CPU).

Standardisation (Sun et al., CVPR 2024) z-scores every student and teacher
row before the tempered softmax of KD / DKD; CE stays on the raw logits:

    mu = mean(x),  sigma = sqrt(sum (x - mu)^2 / (C - 1)),  z = (x - mu) / (sigma + 1e-7)

Everything here is an independent transcription; nothing calls
``ops/losses.py``.  The losses on the standardised rows are ``kd64`` /
``dkd64`` of ``tests/_step_tail.py``.
"""
import contextlib

import torch

from tests import _step_tail as R

EPS = 1e-7
F32, BF16 = R.F32, R.BF16
NAMES = ("ce", "kd", "g_ce", "g_kd", "g_sum")

# (B, C): one row; C = 2; the lane boundary 63 | 64 | 65; NPL = 2, 4, 16 and the
# ladder top 32; (9, 128) is three blocks with a partial last one
GRID = [(1, 3), (3, 2), (5, 63), (4, 64), (5, 65), (7, 100), (2, 200), (3, 1000), (2, 2048), (9, 128)]
TEMPS = [2.0, 4.0]
MIXED = [(BF16, F32), (F32, BF16)]          # (student, teacher) at MIXED_SHAPE
MIXED_SHAPE = (6, 200)
CONST_SHAPE = (3, 100)
# every element of the constant row; a row of them sums exactly in fp32 and bf16
# holds it, so the fp32 mean is the value itself and sigma is exactly 0
CONST_VALUE = 1.5


def standardize64(x):
    """z-score of each row in float64.  ``torch.std``'s backward gives a
    constant row (sigma == 0) no gradient through sigma."""
    x = x.double()
    mu = x.sum(-1, keepdim=True) / x.shape[-1]
    sigma = torch.std(x, dim=-1, correction=1, keepdim=True)
    return (x - mu) / (sigma + EPS)


def kd_term64(kind, s, t, y, hp):
    """The weighted KD / DKD scalar on the standardised rows."""
    zs, zt = standardize64(s), standardize64(t)
    if kind == "kd":
        return hp["kd_w"] * R.kd64(zs, zt, hp["T"])
    return R.dkd64(zs, zt, y, hp["alpha"], hp["beta"], hp["T"])


def ref_all(kind, s, t, y, hp):
    """(ce, kd, g_ce, g_kd, g_sum) in float64 on the CPU; the gradients are
    with respect to the raw student logits."""
    s64 = s.detach().cpu().double().requires_grad_(True)
    t64, y = t.detach().cpu().double(), y.cpu()
    ce = hp["ce_w"] * R.ce64(s64, y)
    kd = kd_term64(kind, s64, t64, y, hp)
    gce, = torch.autograd.grad(ce, s64)
    gkd, = torch.autograd.grad(kd, s64)
    return ce.detach(), kd.detach(), gce, gkd, gce + gkd


def closed_form_grad(x, g):
    """d loss / d x from g = d loss / d z, z = standardize64(x):
    (g_j - mean(g) - z_j (sum_i g_i z_i) k) / (sigma + eps),
    k = (sigma + eps) / ((C - 1) sigma), 0 where sigma == 0."""
    x, g = x.double(), g.double()
    C = x.shape[-1]
    mu = x.sum(-1, keepdim=True) / C
    sigma = ((x - mu).pow(2).sum(-1, keepdim=True) / (C - 1)).sqrt()
    z = (x - mu) / (sigma + EPS)
    k = torch.where(sigma > 0, (sigma + EPS) / ((C - 1) * sigma.clamp_min(1e-300)), torch.zeros_like(sigma))
    return (g - g.mean(-1, keepdim=True) - z * (g * z).sum(-1, keepdim=True) * k) / (sigma + EPS)


def torch_backend_all(kind, s, t, y, hp):
    """The project's fp32 PyTorch path with the switch on, same inputs (CPU)."""
    from mdistiller_ddp_amd.ops import losses as L
    s32 = s.detach().float().clone().requires_grad_(True)
    ce = hp["ce_w"] * L.cross_entropy(s32, y)
    if kind == "kd":
        kd = hp["kd_w"] * L.kd_loss_ref(s32, t.float(), hp["T"], logit_stand=True)
    else:
        kd = L.dkd_loss_ref(s32, t.float(), y, hp["alpha"], hp["beta"], hp["T"], logit_stand=True)
    gce, = torch.autograd.grad(ce, s32, retain_graph=True)
    gkd, = torch.autograd.grad(kd, s32)
    return ce.detach(), kd.detach(), gce, gkd, gce + gkd


def row_errors(got, ref, unit):
    """Error of each output in units of its tolerance scale: max(1, |ref|) for
    the two scalars; for the gradients every row has its own scale, that row's
    largest reference gradient floored at ``unit`` (one constant row has
    gradients 1e5 times its neighbours', a whole-tensor scale would hide
    errors everywhere else)."""
    out = []
    for a, b in zip(got, ref):
        a, b = a.detach().cpu().double(), b.double()
        assert a.shape == b.shape
        if not torch.isfinite(a).all():
            out.append(float("inf"))
        elif b.dim() == 0:
            out.append((a - b).abs().item() / max(1.0, b.abs().item()))
        else:
            scale = b.abs().amax(1, keepdim=True).clamp_min(unit)
            out.append(((a - b).abs() / scale).max().item())
    return out


def assert_rows_close(got, ref, tol, unit, names=NAMES):
    errs = row_errors(got, ref, unit)
    print("  ".join(f"{n}={e:.3g}" for n, e in zip(names, errs)), f"(tol {tol:g})")
    for n, e in zip(names, errs):
        assert e <= tol, f"{n}: error / scale = {e:.3g} > {tol:g}"


@contextlib.contextmanager
def launches():
    """Names of the native launchers called inside the block."""
    from mdistiller_ddp_amd.ops import _ext
    names, orig = [], _ext.call

    def rec(name, *a, **k):
        names.append(name)
        return orig(name, *a, **k)

    _ext.call = rec
    try:
        yield names
    finally:
        _ext.call = orig


def with_constant_row(x, row=1):
    """``x`` with one row set to CONST_VALUE, beside the ordinary rows."""
    x = x.clone()
    x[row] = CONST_VALUE
    return x
