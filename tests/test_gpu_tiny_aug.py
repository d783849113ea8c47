"""HIP rotate/flip/normalise kernel (Tiny-ImageNet augmentation) vs the
fixed-point PyTorch reference: hand-built batches, the grid-stride loop and
the loader's HIP path."""
import numpy as np
import pytest
import torch

from mdistiller_ddp_amd.data.cifar100 import DeviceImageLoader, rotate_coef, rotate_flip_ref
from mdistiller_ddp_amd.data.synthetic import TINY_MEAN, TINY_STD
from mdistiller_ddp_amd.ops import _ext
from mdistiller_ddp_amd.ops.backend import use_backend

pytestmark = pytest.mark.gpu

ANGLES = [0.0, 20.0, -20.0, 45.0, 90.0]


def _data(n, h, w, c, seed=0):
    """uint8 [n, h, w, c] whose 8 neighbours of every pixel all differ from it
    (by >= 1/255 after ToTensor), so one wrong source pixel is a visible error;
    rows differ from each other so a wrong gather is one too."""
    rng = np.random.default_rng(seed)
    i = np.arange(n).reshape(n, 1, 1)
    y = np.arange(h).reshape(1, h, 1)
    x = np.arange(w).reshape(1, 1, w)
    a = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    if c == 1:
        assert h * w <= 256
        a[..., 0] = (y * w + x + 13 * i) % 256
    else:
        assert 3 * max(h, w) <= 256
        a[..., 0] = (3 * x + 5 * i + 0 * y) % 256
        a[..., 1] = (3 * y + 11 * i + 0 * x) % 256
    return torch.from_numpy(a).cuda()


def _run(x, idx, coef, flip, mean, std, dtype):
    b = idx.shape[0]
    _, h, w, c = x.shape
    m = torch.tensor(mean[:c], dtype=torch.float32, device="cuda")
    inv = 1.0 / torch.tensor(std[:c], dtype=torch.float32, device="cuda")
    out = torch.empty(b, h, w, c, dtype=dtype, device="cuda")
    _ext.call("mda_rotate_flip_norm", x, idx, coef, flip, m, inv, out,
              0 if dtype == torch.float32 else 1, b, h, w, c)
    return out.permute(0, 3, 1, 2)


def _check(out, ref, dtype):
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    torch.testing.assert_close(out.float(), ref, atol=tol, rtol=tol)
    assert out.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(5, 64, 64, 3), (3, 8, 12, 3), (2, 16, 16, 1), (2, 6, 7, 3)])
def test_rotate_kernel(shape, dtype):
    b, h, w, c = shape
    x = _data(7, h, w, c)
    idx = torch.tensor([5, 2, 6, 2, 1][:b], device="cuda")  # non-monotone, a repeat, never row 0
    deg = torch.tensor(([45.0, -20.0, 90.0] if b == 3 else ANGLES)[:b], device="cuda")
    flip = torch.tensor([1, 0, 1, 1, 0][:b], dtype=torch.uint8, device="cuda")
    coef = rotate_coef(deg, h, w)
    ref = rotate_flip_ref(x, idx, coef, flip, TINY_MEAN, TINY_STD)
    out = _run(x, idx, coef, flip, TINY_MEAN, TINY_STD, dtype)
    _check(out, ref, dtype)
    # the cases are not degenerate: rotated samples have fill pixels, and differ from the gather
    fill = (-torch.tensor(TINY_MEAN[:c]) / torch.tensor(TINY_STD[:c])).cuda().view(1, c, 1, 1)
    if b >= 2:
        assert ((ref[1:2] - fill).abs().amax(1) < 1e-6).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rotate_kernel_grid_stride(dtype):
    """300 x 64 x 64 = 1.23 M pixels: more than the 4096 x 256 threads (2048 x
    256 pixel pairs for bf16) one launch starts, so every thread loops."""
    b = 300
    x = _data(40, 64, 64, 3, seed=1)
    g = torch.Generator(device="cuda").manual_seed(3)
    idx = torch.randint(1, 40, (b,), generator=g, device="cuda")
    deg = (torch.rand(b, generator=g, device="cuda") * 2 - 1) * 20
    flip = torch.randint(0, 2, (b,), generator=g, device="cuda", dtype=torch.uint8)
    coef = rotate_coef(deg, 64, 64)
    ref = rotate_flip_ref(x, idx, coef, flip, TINY_MEAN, TINY_STD)
    out = _run(x, idx, coef, flip, TINY_MEAN, TINY_STD, dtype)
    _check(out, ref, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rotate_loader_hip_path(dtype):
    x = _data(100, 64, 64, 3, seed=2)
    y = np.arange(100) % 10
    ld = DeviceImageLoader(x, y, 16, "cuda", train=True, out_dtype=dtype, mean=TINY_MEAN, std=TINY_STD,
                           pad=0, rotate=20)
    idx = torch.arange(16, device="cuda") * 5 + 1
    gen_state = ld.gen.get_state()
    with use_backend("hip"):
        out = ld._make(idx)
    ld.gen.set_state(gen_state)
    deg = (torch.rand(16, generator=ld.gen, device="cuda") * 2 - 1) * 20
    flip = torch.randint(0, 2, (16,), generator=ld.gen, device="cuda", dtype=torch.uint8)
    assert deg.abs().max() <= 20 and deg.abs().max() > 5 and 0 < int(flip.sum()) < 16
    ref = rotate_flip_ref(ld.x, idx, rotate_coef(deg, 64, 64), flip, TINY_MEAN, TINY_STD)
    _check(out, ref, dtype)
    with use_backend("torch"):
        ld.gen.set_state(gen_state)
        torch.testing.assert_close(ld._make(idx).float(), ref.to(dtype).float(), atol=0, rtol=0)
