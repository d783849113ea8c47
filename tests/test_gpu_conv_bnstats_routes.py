"""mda_conv_fwd_bnstats on every route its launch can take: the number of
per-block partial rows the BN finalize reads comes from the planned route, so
each kernel family (and the split-K fallback through mda_bn_stats2) must give
the batch statistics of the output it stored."""
import pytest
import torch
import torch.nn.functional as F

from mdistiller_ddp_amd.ops import _ext, hip_train

pytestmark = pytest.mark.gpu

GLDS, REG, HALO, HALO1 = 0, 1, 2, 3
FIELDS = ["rc", "stream1x1", "family", "bm", "bn", "mode", "ring", "flip", "grid_x", "grid_y",
          "grid_z", "steps_per_split", "splits", "combine_blocks", "nblk"]
N = 2

CASES = [
    # name, Cin, H, Cout, stride, tile, splits (0 = planned), expected family, split over K
    ("halo1", 64, 16, 64, 1, 64064, 1, HALO1, False),
    ("halo", 128, 16, 64, 1, 64064, 1, HALO, False),
    ("halo_demoted", 64, 4, 64, 1, 0, 0, GLDS, True),   # 252-row patch, planned splits > 1
    ("glds", 64, 16, 64, 2, 64064, 1, GLDS, False),
    ("split_k", 128, 8, 64, 1, 0, 0, HALO, True),
]


def _route(Cin, H, Ho, Cout, stride, Kp, tile, splits):
    out = torch.zeros(len(FIELDS), dtype=torch.int64)
    _ext.call("mda_conv_route", 1, N, H, H, Cin, Ho, Ho, Cout, 3, 3, stride, 1, Kp, 1, tile, splits, 0, out)
    return dict(zip(FIELDS, out.tolist()))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bnstats_matches_fp32_on_route(case):
    name, Cin, H, Cout, stride, tile, splits, family, split_k = case
    torch.manual_seed(0)
    Ho = (H + 2 - 3) // stride + 1
    M = N * Ho * Ho
    w = (torch.randn(Cout, Cin, 3, 3, device="cuda") / (Cin * 9) ** 0.5).to(torch.bfloat16).float()
    x = torch.randn(N, Cin, H, H, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wf, _, Kp, _ = hip_train.pack_weights(w, False)

    r = _route(Cin, H, Ho, Cout, stride, Kp, tile, splits)
    assert r["rc"] == 0 and r["family"] == family, r
    assert (r["splits"] > 1) == split_k, r
    if name == "halo_demoted":
        # eligible for the halo kernels (a forced single split takes halo1), demoted as planned
        assert _route(Cin, H, Ho, Cout, stride, Kp, 64064, 1)["family"] == HALO1
    if not split_k:
        assert r["nblk"] == r["grid_x"] == -(-M // r["bm"]), r

    y = torch.empty(N, Cout, Ho, Ho, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    part = torch.empty(r["splits"] * M * Cout, device="cuda") if r["splits"] > 1 else None
    bn_partial = torch.zeros(2 * 2048 * 512, device="cuda")
    gamma, beta = torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda")
    rmean, rvar = torch.zeros(Cout, device="cuda"), torch.ones(Cout, device="cuda")
    stats = torch.zeros(4, Cout, device="cuda")
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    eps = 1e-5
    _ext.call("mda_conv_fwd_bnstats", x, wf, y, part, bn_partial, bn_partial.numel(), N, H, H, Cin, Ho,
              Ho, Cout, 3, 3, stride, 1, Kp, tile, splits, gamma, beta, rmean, rvar, stats[0], stats[1],
              stats[2], stats[3], 0.1, eps, nbt)
    torch.cuda.synchronize()

    ref = F.conv2d(x.float(), w, stride=stride, padding=1)
    rb = ref.to(torch.bfloat16).float()
    mean = rb.mean(dim=(0, 2, 3))
    rstd = (rb.var(dim=(0, 2, 3), unbiased=False) + eps).rsqrt()
    # tolerances of the BN assertions in test_gpu_train_layers.py: 4e-2 for
    # activations, 1e-3 for (running) means, 1e-2 for (running) variances
    torch.testing.assert_close(y.float(), ref, atol=4e-2, rtol=4e-2)
    torch.testing.assert_close(stats[0], mean, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(stats[1], rstd, atol=1e-2, rtol=1e-2)
