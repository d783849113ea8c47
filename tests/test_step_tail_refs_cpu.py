"""CPU checks of the float64 references that ``test_gpu_step_tail.py`` holds
the HIP kernels to (``tests/_step_tail.py``).

* The float64 KD / DKD transcriptions reproduce the reference project's stored
  ``kd`` / ``dkd`` cases (``tests/fixtures/ref_losses.safetensors``), value and
  gradient, at the tolerance of ``test_parity_reference.py``, and agree with
  ``kd_loss_ref`` / ``dkd_loss_ref`` on benign inputs.
* The float64 DOT transcription agrees with ``FlatDOT._step_torch``.
* The project's fp32 PyTorch backend is inside the GPU tests' tolerances
  against the float64 references on every case the GPU file runs, so the
  reference alone does not use the tolerance up.  The one exception is named:
  DKD with a confident student, where ``dkd_loss_ref`` evaluates log(0).
* ``FlatOptimizer.set_active`` on the PyTorch backend.
"""
import math

import pytest
import torch

from tests import _fixtures as FX
from tests import _step_tail as R
from mdistiller_ddp_amd.ops import losses as L
from mdistiller_ddp_amd.ops.backend import use_backend

F32, BF16 = R.F32, R.BF16


@pytest.mark.parametrize("key", ["kd", "dkd", "dkd64"])
def test_float64_refs_reproduce_reference_fixtures(key):
    c = FX.case("ref_losses", key)
    s = c["in0"].double().requires_grad_(True)
    if key == "kd":
        loss = R.kd64(s, c["in1"], 4.0)
    else:
        loss = R.dkd64(s, c["in1"], c["target"], 1.0, 8.0, 4.0)
    g, = torch.autograd.grad(loss, s)
    torch.testing.assert_close(loss, c["loss"].double().reshape(()), atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(g, c["grad0"].double(), atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("B,C", [(7, 2), (33, 100), (5, 1000)])
def test_float64_refs_agree_with_project_refs_on_benign_inputs(B, C):
    s, t, y = R.loss_inputs(B, C)
    s64 = s.double().requires_grad_(True)
    s32 = s.clone().requires_grad_(True)
    for a, b in ((R.kd64(s64, t, 4.0), L.kd_loss_ref(s32, t, 4.0)),
                 (R.dkd64(s64, t, y, 1.0, 8.0, 4.0), L.dkd_loss_ref(s32, t, y, 1.0, 8.0, 4.0)),
                 (R.ce64(s64, y), L.cross_entropy(s32, y))):
        ga, = torch.autograd.grad(a, s64)
        gb, = torch.autograd.grad(b, s32)
        torch.testing.assert_close(a, b.double(), atol=1e-5, rtol=1e-4)
        torch.testing.assert_close(ga, gb.double(), atol=1e-5, rtol=1e-4)


def test_float64_dkd_is_finite_for_one_hot_student_and_teacher():
    for where in R.EXTREME_WHERE + ["teacher"]:
        for B, C, gap, T in R.EXTREME:
            s, t, y = R.loss_inputs(B, C, gap=gap, where=where)
            hp = dict(R.HP["dkd"], T=T)
            assert all(torch.isfinite(v).all() for v in R.ref_all("dkd", s, t, y, hp))


def test_float64_dot_agrees_with_flat_dot_step_torch():
    """All four mask values, the ``first`` step and three later ones."""
    with use_backend("torch"):
        worst = R.run_flat_vs_torch64("dot", "cpu", (300, 37, 640, 100))
    assert worst <= 1.0, worst


# ---- the fp32 PyTorch backend against float64, every case of the GPU file ----

def _torch_backend_errors(kind, s, t, y, hp):
    ref = R.ref_all(kind, s, t, y, hp)
    got = R.torch_backend_all(kind, s, t, y, hp)
    return R.rel_errors(got, ref, R.grad_unit(hp, s.shape[0]))


@pytest.mark.parametrize("kind", ["kd", "dkd"])
def test_torch_backend_inside_tolerance_grid_mixed_limit(kind):
    cases = [R.loss_inputs(B, C, ds) for B, C in R.GRID for ds in (F32, BF16)]
    cases += [R.loss_inputs(*R.MIXED_SHAPE, ds, dt) for ds, dt in R.MIXED]
    cases += [R.loss_inputs(*R.LIMIT)] + [R.loss_inputs(B, C) for B, C in R.FALLBACK]
    cases += [R.loss_inputs(B, 100) for B in R.COUNTER_BS]
    worst = max(max(_torch_backend_errors(kind, s, t, y, R.HP[kind])) for s, t, y in cases)
    print(f"{kind}: torch fp32 vs float64, worst error / scale = {worst:.3g}")
    assert worst <= 0.1 * R.TOL[F32], worst


@pytest.mark.parametrize("kind", ["kd", "dkd"])
@pytest.mark.parametrize("where", R.EXTREME_WHERE)
def test_torch_backend_on_extreme_logits(kind, where):
    for B, C, gap, T in R.EXTREME:
        s, t, y = R.loss_inputs(B, C, gap=gap, where=where)
        hp = dict(R.HP[kind], T=T)
        err = _torch_backend_errors(kind, s, t, y, hp)
        print(f"{kind} {where} gap={gap} T={T}: {max(err):.3g}")
        if kind == "dkd":
            # dkd_loss_ref takes the log of a probability that underflows (to 0,
            # or to a denormal at the smaller gap): no usable fp32 PyTorch value
            # here, only the float64 one
            continue
        assert max(err) <= 0.1 * R.TOL[F32], err


def test_torch_backend_ce_inside_tolerance():
    for B, C in R.CE_SHAPES:
        for ds in (F32, BF16):
            s, _, y = R.loss_inputs(B, C, ds)
            s64 = s.double().requires_grad_(True)
            s32 = s.float().requires_grad_(True)
            a, b = 0.7 * R.ce64(s64, y), 0.7 * L.cross_entropy(s32, y)
            ga, = torch.autograd.grad(a, s64)
            gb, = torch.autograd.grad(b, s32)
            assert (a - b).abs().item() <= 0.1 * R.TOL[F32] * max(1.0, a.abs().item())
            assert (ga - gb).abs().max().item() <= 0.1 * R.TOL[F32] * ga.abs().max().item()


@pytest.mark.parametrize("kind", R.OPT_KINDS)
def test_torch_backend_optimizers_inside_tolerance_large_buffer(kind):
    with use_backend("torch"):
        worst = R.run_flat_vs_torch64(kind, "cpu", R.BIG)
    print(f"{kind}: torch fp32 flat vs float64, worst error / tolerance = {worst:.3g}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("pattern", sorted(R.ACTIVE_PATTERNS))
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_set_active_torch_backend(kind, pattern):
    with use_backend("torch"):
        R.check_set_active(kind, pattern, "cpu")
