"""Float64 references and shared cases for the step-tail tests
(``test_gpu_step_tail.py`` on the GPU, ``test_step_tail_refs_cpu.py`` on the
CPU): fused logit losses, flat optimizers, DOT.

Everything here is an independent transcription of the formulas; nothing
calls ``kd_loss_ref`` / ``dkd_loss_ref`` or the flat optimizers' own math.
Inputs are generated on the CPU from a seed derived from the case, so the
CPU and the GPU file see the same numbers.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 1e-4, BF16: 2e-2}   # the loss tests' own tolerances
OPT_TOL = 1e-5                  # optimizers: atol = rtol

# --------------------------------------------------------------------------
# float64 losses


def ce64(s, y):
    return F.cross_entropy(s.double(), y)


def kd64(s, t, T):
    ls = F.log_softmax(s.double() / T, dim=1)
    lt = F.log_softmax(t.double() / T, dim=1)
    return (lt.exp() * (lt - ls)).sum(1).mean() * T * T


def _split_target(z, y):
    """(z[b, y_b], z[b, every other class]) -- the non-target set is gathered,
    so no masking constant and no infinity enters the graph."""
    B, C = z.shape
    idx = torch.arange(C - 1).expand(B, C - 1)
    idx = idx + (idx >= y.reshape(-1, 1)).long()
    return z.gather(1, y.reshape(-1, 1)).squeeze(1), z.gather(1, idx)


def dkd64(s, t, y, alpha, beta, T):
    """DKD = alpha * TCKD + beta * NCKD, all in the log domain: finite for
    one-hot students and teachers."""
    zs_y, zs_o = _split_target(s.double() / T, y)
    zt_y, zt_o = _split_target(t.double() / T, y)
    ls_o, lt_o = torch.logsumexp(zs_o, 1), torch.logsumexp(zt_o, 1)
    # binary (target, rest) log-probabilities
    lbs = torch.stack([zs_y, ls_o], 1) - torch.logaddexp(zs_y, ls_o).unsqueeze(1)
    lbt = torch.stack([zt_y, lt_o], 1) - torch.logaddexp(zt_y, lt_o).unsqueeze(1)
    tckd = (lbt.exp() * (lbt - lbs)).sum(1).mean()
    lq = zs_o - ls_o.unsqueeze(1)   # log-softmax over the non-target classes
    lp = zt_o - lt_o.unsqueeze(1)
    nckd = (lp.exp() * (lp - lq)).sum(1).mean()
    return (alpha * tckd + beta * nckd) * T * T


# kind -> hyper-parameters of the weighted pair (ce term, kd term)
HP = {"kd": dict(T=4.0, ce_w=0.1, kd_w=0.9),
      "dkd": dict(T=4.0, ce_w=1.0, alpha=1.0, beta=8.0)}


def pair64(kind, s, t, y, hp):
    """The two weighted scalars the fused kernel returns, in float64."""
    ce = hp["ce_w"] * ce64(s, y)
    if kind == "kd":
        return ce, hp["kd_w"] * kd64(s, t, hp["T"])
    return ce, dkd64(s, t, y, hp["alpha"], hp["beta"], hp["T"])


def ref_all(kind, s, t, y, hp):
    """(ce, kd, g_ce, g_kd, g_sum) in float64 on the CPU."""
    s64 = s.detach().cpu().double().requires_grad_(True)
    ce, kd = pair64(kind, s64, t.detach().cpu().double(), y.cpu(), hp)
    gce, = torch.autograd.grad(ce, s64, retain_graph=True)
    gkd, = torch.autograd.grad(kd, s64)
    return ce.detach(), kd.detach(), gce, gkd, gce + gkd


def torch_backend_all(kind, s, t, y, hp):
    """The project's fp32 PyTorch path on the same inputs (CPU)."""
    from mdistiller_ddp_amd.ops import losses as L
    s32 = s.detach().float().clone().requires_grad_(True)
    ce = hp["ce_w"] * L.cross_entropy(s32, y)
    if kind == "kd":
        kd = hp["kd_w"] * L.kd_loss_ref(s32, t.float(), hp["T"])
    else:
        kd = L.dkd_loss_ref(s32, t.float(), y, hp["alpha"], hp["beta"], hp["T"])
    gce, = torch.autograd.grad(ce, s32, retain_graph=True)
    gkd, = torch.autograd.grad(kd, s32)
    return ce.detach(), kd.detach(), gce, gkd, gce + gkd


def grad_unit(hp, B):
    """Floor of the gradient scale: ce_w / B, the CE gradient of one fully
    wrong row.  It only matters where every row is confidently right and the
    exact gradient (1e-60 in float64) is below anything fp32 can hold."""
    return hp["ce_w"] / B


def _scale(i, b, unit):
    return max(1.0, b.abs().max().item()) if i < 2 else max(b.abs().max().item(), unit)


def rel_errors(got, ref, unit):
    """Error of each of the five outputs in units of its tolerance scale:
    |got - ref| / max(1, |ref|) for the scalars, / max(max|ref|, unit) for
    the gradients."""
    out = []
    for i, (a, b) in enumerate(zip(got, ref)):
        a, b = a.detach().cpu().double(), b.double()
        scale = _scale(i, b, unit)
        out.append(float("inf") if not torch.isfinite(a).all() else
                   ((a - b).abs().max().item() / scale))
    return out


def assert_loss_close(got, ref, tol, unit, names=("ce", "kd", "g_ce", "g_kd", "g_sum")):
    """Scalars: atol = tol * max(1, |ref|); gradients: atol = tol * largest
    reference gradient (floored at ``unit``, see grad_unit); rtol = tol on top,
    as in the sibling loss tests."""
    for i, (a, b, n) in enumerate(zip(got, ref, names)):
        a = a.detach().cpu().double()
        assert torch.isfinite(a).all(), f"{n} is not finite"
        scale = _scale(i, b, unit)
        torch.testing.assert_close(a, b.double(), atol=tol * scale, rtol=tol, msg=lambda m, n=n: f"{n}: {m}")


# --------------------------------------------------------------------------
# loss inputs


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def forced_labels(y, C):
    """Labels 0 and C-1 and, where C allows, the lane boundary 63 | 64."""
    forced = [0, C - 1] + ([63] if C > 63 else []) + ([64] if C > 64 else [])
    for i, v in enumerate(forced):
        y[i % y.shape[0]] = v
    return y


@functools.lru_cache(maxsize=None)
def loss_inputs(B, C, ds=F32, dt=None, gap=0.0, where="none"):
    """CPU (s, t, y).  ``where``: which logit gets ``+gap`` --
    ``student`` / ``teacher`` / ``both`` (the target) or ``wrong`` (the student's
    class y+1)."""
    dt = dt or ds
    g = torch.Generator().manual_seed(_seed(B, C, gap, where))
    s = torch.randn(B, C, generator=g) * 3
    t = torch.randn(B, C, generator=g) * 3
    y = forced_labels(torch.randint(0, C, (B,), generator=g), C)
    r = torch.arange(B)
    if where in ("student", "both"):
        s[r, y] += gap
    if where in ("teacher", "both"):
        t[r, y] += gap
    if where == "wrong":
        s[r, (y + 1) % C] += gap
    return s.to(ds), t.to(dt), y


# every C with a B > 256, every NPL instantiation (2: C<=128, 4: <=256, 8: <=512,
# 16: <=1024, 32: <=2048); B = 257 is 65 blocks with a partial last one
GRID = [(257, 2), (1027, 63), (257, 64), (1027, 65), (257, 128), (1027, 129), (257, 300),
        (257, 512), (257, 1000), (257, 1025), (257, 2048),
        (5, 2), (1, 65), (5, 129), (5, 300), (1, 1000), (1, 2048)]
MIXED = [(BF16, F32), (F32, BF16)]          # (student, teacher) at MIXED_SHAPE
MIXED_SHAPE = (37, 200)
CE_SHAPES = [(5, 100), (257, 1025)]
# (B, C, gap, T): the gaps of the confident-teacher tests
EXTREME = [(16, 1000, 150.0, 1.0), (16, 100, 400.0, 4.0)]
EXTREME_WHERE = ["student", "both", "wrong"]
LIMIT = (8192, 65)
FALLBACK = [(8193, 65), (4, 2049)]
COUNTER_BS = (1027, 5, 257)


# --------------------------------------------------------------------------
# optimizers

BIG = (1_000_000, 37, 48_640, 1000)   # 1 049 728 elements after 64-padding
OPT_KINDS = ["sgd", "sgd_clip", "adam", "adamw", "adam_clip", "dot"]
DOT_HP = dict(lr=0.1, mu_t=0.825, mu_k=0.975, wd=5e-4, gscale=0.5)
# one param per mask value 0..3: (has_task, has_kd)
DOT_REACH = ([False, True, False, True], [False, False, True, True])


def make_params(sizes, device, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).to(device)) for n in sizes]


def make_flat_opt(kind, params):
    from mdistiller_ddp_amd.engine.optim import FlatParams, FlatSGD, FlatAdam, FlatDOT
    f = FlatParams(params, 2 if kind == "dot" else 1)
    if kind == "sgd":
        o = FlatSGD(f, 0.1, 0.9, 5e-4, grad_scale=0.5)
    elif kind == "sgd_clip":
        o = FlatSGD(f, 0.1, 0.9, 5e-4, grad_clip=0.3)
    elif kind == "adam":
        o = FlatAdam(f, 1e-3, weight_decay=1e-2)
    elif kind == "adamw":
        o = FlatAdam(f, 1e-3, weight_decay=1e-2, decoupled=True)
    elif kind == "adam_clip":
        o = FlatAdam(f, 1e-3, weight_decay=1e-2, grad_clip=0.3, grad_scale=0.5)
    else:
        h = DOT_HP
        o = FlatDOT(f, h["lr"], h["mu_t"], h["mu_k"], h["wd"], grad_scale=h["gscale"])
    return f, o


def make_torch_opt(kind, p64):
    """torch.optim on float64 copies: (optimizer, grad_scale, max_norm)."""
    if kind == "sgd":
        return torch.optim.SGD(p64, lr=0.1, momentum=0.9, weight_decay=5e-4), 0.5, 0.0
    if kind == "sgd_clip":
        return torch.optim.SGD(p64, lr=0.1, momentum=0.9, weight_decay=5e-4), 1.0, 0.3
    if kind == "adam":
        return torch.optim.Adam(p64, lr=1e-3, weight_decay=1e-2), 1.0, 0.0
    if kind == "adamw":
        return torch.optim.AdamW(p64, lr=1e-3, weight_decay=1e-2), 1.0, 0.0
    if kind == "adam_clip":
        return torch.optim.Adam(p64, lr=1e-3, weight_decay=1e-2), 0.5, 0.3
    raise ValueError(kind)


def base_lr(kind):
    return 1e-3 if kind.startswith("adam") else 0.1


def random_grads(f, g):
    """CPU gradients for every set of ``f``; the alignment padding between
    params stays zero, as in training (it counts in the clip norm)."""
    grads = torch.zeros(f.grads.shape)
    for p, off in zip(f.params, f.offsets):
        grads[:, off:off + p.numel()] = torch.randn(f.grads.shape[0], p.numel(), generator=g)
    return grads


class Dot64:
    """The DOT rule of the header comment of ``csrc/optim.hip`` in float64,
    vectorised over a flat buffer with the per-element mask."""

    def __init__(self, p, mask, mu_t, mu_k, wd, gscale):
        self.p = p.double().clone()
        self.has_t = (mask & 1).bool()
        self.has_k = (mask & 2).bool()
        self.bt = torch.zeros_like(self.p)
        self.bk = torch.zeros_like(self.p)
        self.mu_t, self.mu_k, self.wd, self.s = mu_t, mu_k, wd, gscale
        self.first = True

    def step(self, gt, gk, lr):
        p, t, k = self.p, self.has_t, self.has_k
        both = t & k
        mu_avg = (self.mu_t + self.mu_k) / 2
        # task pass
        d = self.s * gt.double() + self.wd * p
        mom = torch.where(both, torch.tensor(self.mu_t, dtype=torch.float64),
                          torch.tensor(mu_avg, dtype=torch.float64))
        bt = d if self.first else mom * self.bt + d
        self.bt = torch.where(t, bt, self.bt)
        p = torch.where(t, p - lr * self.bt, p)
        # kd pass (sees the parameter after the task pass)
        dk = self.s * gk.double()
        if self.first:
            bk = dk
        else:
            bk = torch.where(both, self.mu_k * self.bk + dk, mu_avg * self.bk + dk + self.wd * p)
        self.bk = torch.where(k, bk, self.bk)
        self.p = torch.where(k, p - lr * self.bk, p)
        self.first = False


def run_flat_vs_torch64(kind, device, sizes, steps=4, on_step=None):
    """Step a flat optimizer (current backend) and its float64 reference with
    the same gradients and a changing learning rate.  Returns the largest
    |flat - ref| / (atol + rtol |ref|) seen over the parameters (and, for the
    clip kinds, the norm), i.e. <= 1 means inside ``OPT_TOL``."""
    params = make_params(sizes, device, seed=2)
    p64 = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in params]
    f, o = make_flat_opt(kind, params)
    if kind == "dot":
        o.set_reachability(*DOT_REACH)
        h = DOT_HP
        ref = Dot64(f.data.cpu(), o.mask.cpu(), h["mu_t"], h["mu_k"], h["wd"], h["gscale"])
    else:
        topt, gscale, max_norm = make_torch_opt(kind, p64)
    g = torch.Generator().manual_seed(3)
    worst = 0.0

    def ratio(a, b):
        a, b = a.detach().cpu().double(), b.detach().double()
        assert torch.isfinite(a).all()
        return ((a - b).abs() / (OPT_TOL + OPT_TOL * b.abs())).max().item()

    for it in range(steps):
        grads = random_grads(f, g)
        f.grads.copy_(grads.to(device))
        lr = base_lr(kind) / (it + 1)
        o.set_lr(lr)
        o.step()
        if kind == "dot":
            ref.step(grads[0], grads[1], lr)
            for p, off in zip(f.params, f.offsets):
                worst = max(worst, ratio(p, ref.p[off:off + p.numel()]))
        else:
            for q, p, off in zip(p64, f.params, f.offsets):
                q.grad = gscale * grads[0, off:off + p.numel()].double()
            if max_norm > 0:
                norm = torch.nn.utils.clip_grad_norm_(p64, max_norm)
                worst = max(worst, ratio(o.norm_t.reshape(()), norm))
            topt.param_groups[0]["lr"] = lr
            topt.step()
            for q, p in zip(p64, f.params):
                worst = max(worst, ratio(p, q))
        if on_step is not None:
            on_step(it, worst)
    return worst


# five parameters; inactive at the front / in the middle (A) and in the middle /
# at the end (B); each has two adjacent active ones that merge into one range
ACTIVE_SIZES = (100, 37, 4096, 64, 1000)
ACTIVE_PATTERNS = {"A": [False, True, True, False, True], "B": [True, False, True, True, False]}


def check_set_active(kind, pattern, device):
    """FlatOptimizer.set_active == torch.optim with ``.grad = None``: one step
    with every param active (so the state is non-zero), then three with the
    pattern.  Inactive params and their state must not change by a bit, in
    spite of weight decay and a non-zero gradient."""
    active = ACTIVE_PATTERNS[pattern]
    params = make_params(ACTIVE_SIZES, device, seed=5)
    p64 = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in params]
    f, o = make_flat_opt(kind, params)
    topt, gscale, _ = make_torch_opt(kind, p64)
    state = [o.buf] if kind == "sgd" else [o.m1, o.m2]
    g = torch.Generator().manual_seed(6)
    frozen = None
    for it in range(4):
        if it == 1:
            o.set_active(active)
            n_act = sum(active)
            assert len(o._spans()) == n_act - 1, "two adjacent active params merge into one range"
            frozen = [f.data.clone()] + [b.clone() for b in state]
        grads = random_grads(f, g)
        f.grads.copy_(grads.to(device))
        lr = base_lr(kind) / (it + 1)
        o.set_lr(lr)
        o.step()
        for q, p, off, a in zip(p64, f.params, f.offsets, active):
            q.grad = gscale * grads[0, off:off + p.numel()].double() if (a or it == 0) else None
        topt.param_groups[0]["lr"] = lr
        topt.step()
    for q, p, off, a in zip(p64, f.params, f.offsets, active):
        n = p.numel()
        if a:
            torch.testing.assert_close(p.detach().cpu().double(), q.detach(), atol=OPT_TOL, rtol=OPT_TOL)
        else:
            assert f.grads[0, off:off + n].abs().min() > 0 and o.weight_decay > 0
            for now, then in zip([f.data] + state, frozen):
                assert torch.equal(now[off:off + n], then[off:off + n])
                assert then[off:off + n].abs().max() > 0   # the first step did fill it
            # and it still equals the reference, which skipped it
            torch.testing.assert_close(p.detach().cpu().double(), q.detach(), atol=OPT_TOL, rtol=OPT_TOL)
