"""Device-resident Tiny-ImageNet on CPU: the fixed-point rotate/flip reference
(identity, flip, agreement with PIL's rotation), the one-time pack of the
folder tree and its cache, the get_dataset dispatch and the per-epoch
determinism of the augmentation stream."""
import numpy as np
import pytest
import torch

from mdistiller_ddp_amd.config import get_cfg
from mdistiller_ddp_amd.data import get_dataset
from mdistiller_ddp_amd.data.cifar100 import DeviceImageLoader
from mdistiller_ddp_amd.data.synthetic import TINY_MEAN, TINY_STD
from mdistiller_ddp_amd.data.tiny_imagenet import (load_tiny_imagenet, rotate_coef, rotate_flip_ref,
                                                   rotate_flip_u8_ref)


def _images(n, seed=0, hw=64, c=3):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, hw, hw, c), dtype=np.uint8))


def test_identity_and_flip():
    x = _images(6)
    idx = torch.tensor([4, 1, 1, 5])
    coef = rotate_coef(torch.zeros(4), 64, 64)
    assert coef.dtype == torch.int32 and coef.shape == (4, 6)
    no = torch.zeros(4, dtype=torch.uint8)
    out = rotate_flip_u8_ref(x, idx, coef, no)
    assert out.dtype == torch.uint8 and torch.equal(out, x[idx])
    fl = torch.tensor([1, 0, 1, 1], dtype=torch.uint8)
    out = rotate_flip_u8_ref(x, idx, coef, fl)
    assert torch.equal(out[0], x[4].flip(1)) and torch.equal(out[1], x[1])
    assert torch.equal(out[2], x[1].flip(1)) and torch.equal(out[3], x[5].flip(1))
    ref = (x[idx].permute(0, 3, 1, 2).float() / 255
           - torch.tensor(TINY_MEAN).view(1, 3, 1, 1)) / torch.tensor(TINY_STD).view(1, 3, 1, 1)
    torch.testing.assert_close(rotate_flip_ref(x, idx, coef, no, TINY_MEAN, TINY_STD), ref)


def test_rotation_matches_pil():
    """The folder path rotates with PIL (nearest, no expand, fill 0); the
    fixed-point formula must pick the same source pixel in all but 0.5 % of an
    image's pixels (measured with PIL 12.2 over 1000 random angles: at most
    0.17 %, 7 of 4096; a wrong sign, centre or flip order differs in tens of
    percent)."""
    from PIL import Image
    rng = np.random.default_rng(5)
    angles = [20.0, -20.0, 0.37, -0.37] + rng.uniform(-20, 20, 30).tolist()
    x = _images(len(angles), seed=1)
    idx = torch.arange(len(angles))
    coef = rotate_coef(torch.tensor(angles), 64, 64)
    out = rotate_flip_u8_ref(x, idx, coef, torch.zeros(len(angles), dtype=torch.uint8)).numpy()
    for i, deg in enumerate(angles):
        pil = np.asarray(Image.fromarray(x[i].numpy()).rotate(deg, Image.NEAREST, expand=False,
                                                              fillcolor=0))
        differ = (pil != out[i]).any(axis=2).mean()
        print(f"deg {deg:+8.3f}: {100 * differ:.4f} % of pixels differ from PIL")
        assert differ <= 0.005, (deg, differ)
        if abs(deg) == 20.0:
            for cy, cx in ((0, 0), (0, 63), (63, 0), (63, 63)):
                assert (out[i, cy, cx] == 0).all() and (pil[cy, cx] == 0).all(), (deg, cy, cx)
    # and the flip is applied to the ROTATED image
    fl = rotate_flip_u8_ref(x, idx, coef, torch.ones(len(angles), dtype=torch.uint8)).numpy()
    assert np.array_equal(fl, out[:, :, ::-1])


# ----------------------------------------------------------------------------
def _tree(root, per_class=3, split="train", seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    d = root / "tiny-imagenet-200" / split
    for c in ("n01", "n02", "n03"):
        (d / c / "images").mkdir(parents=True)
        for i in range(per_class):
            if c == "n02" and i == 1:  # the real set has grayscale files
                Image.fromarray(rng.integers(0, 256, (64, 64), dtype=np.uint8), "L").save(
                    d / c / "images" / f"{c}_{i}.png")
            else:
                Image.fromarray(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)).save(
                    d / c / "images" / f"{c}_{i}.png")
    return d


def _decode_all(split_dir):
    from PIL import Image
    from mdistiller_ddp_amd.data.imagefolder import scan_folder
    samples, classes = scan_folder(str(split_dir))
    x = np.stack([np.asarray(Image.open(p).convert("RGB")) for p, _ in samples])
    return x, np.asarray([t for _, t in samples]), classes


def test_pack_and_cache(tmp_path, monkeypatch):
    from PIL import Image
    d = _tree(tmp_path)
    x, y, classes = load_tiny_imagenet(str(tmp_path), "train")
    rx, ry, rclasses = _decode_all(d)
    assert x.dtype == np.uint8 and x.shape == (9, 64, 64, 3) and y.dtype == np.int64
    assert np.array_equal(x, rx) and np.array_equal(y, ry) and classes == rclasses == ["n01", "n02", "n03"]
    assert (x[4, :, :, 0] == x[4, :, :, 1]).all()  # the grayscale file, replicated to RGB
    base = tmp_path / "tiny-imagenet-200"
    assert (base / "train_u8.npy").exists() and (base / "train_u8.json").exists()
    assert sorted(p.name for p in base.iterdir()) == ["train", "train_u8.json", "train_u8.npy"]

    real_open = Image.open

    def no_open(*a, **k):
        raise AssertionError("the cache must be read without opening an image")

    monkeypatch.setattr(Image, "open", no_open)
    x2, y2, _ = load_tiny_imagenet(str(tmp_path), "train")
    assert np.array_equal(x2, rx) and np.array_equal(y2, ry)
    # a truncated array is not trusted
    raw = (base / "train_u8.npy").read_bytes()
    (base / "train_u8.npy").write_bytes(raw[: len(raw) // 2])
    with pytest.raises(AssertionError, match="without opening"):
        load_tiny_imagenet(str(tmp_path), "train")
    monkeypatch.setattr(Image, "open", real_open)
    x3, _, _ = load_tiny_imagenet(str(tmp_path), "train")
    assert np.array_equal(x3, rx)

    # a new file makes the sidecar stale: rebuilt, in scan order
    Image.fromarray(np.full((64, 64, 3), 7, np.uint8)).save(d / "n01" / "images" / "n01_9.png")
    monkeypatch.setattr(Image, "open", no_open)
    with pytest.raises(AssertionError, match="without opening"):
        load_tiny_imagenet(str(tmp_path), "train")
    monkeypatch.setattr(Image, "open", real_open)
    x4, y4, _ = load_tiny_imagenet(str(tmp_path), "train")
    rx4, ry4, _ = _decode_all(d)
    assert x4.shape[0] == 10 and np.array_equal(x4, rx4) and np.array_equal(y4, ry4)
    assert (x4[3] == 7).all()

    # a file of another size is an error that names it
    Image.fromarray(np.zeros((32, 32, 3), np.uint8)).save(d / "n03" / "images" / "small.png")
    with pytest.raises(ValueError, match="small.png"):
        load_tiny_imagenet(str(tmp_path), "train")


# ----------------------------------------------------------------------------
def _cfg(root, gpu_aug=True, crd=False):
    cfg = get_cfg()
    cfg.DATASET.TYPE = "tiny_imagenet"
    cfg.DATASET.ROOT = str(root)
    cfg.DATASET.GPU_AUG = gpu_aug
    cfg.DATASET.NUM_WORKERS = 0
    cfg.SOLVER.BATCH_SIZE = 4
    cfg.DATASET.TEST.BATCH_SIZE = 4
    cfg.CRD.NCE.K = 5
    if crd:
        cfg.DISTILLER.TYPE = "CRD"
        cfg.SOLVER.TRAINER = "crd"
    return cfg


@pytest.fixture(scope="module")
def tiny_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("tiny")
    _tree(root, split="train")
    _tree(root, per_class=2, split="val", seed=1)
    return root


def test_dispatch_device_loaders(tiny_root):
    tr, va, n, nc = get_dataset(_cfg(tiny_root), "cpu")
    assert isinstance(tr, DeviceImageLoader) and isinstance(va, DeviceImageLoader)
    assert n == 9 and nc == 200 and tr.rotate == 20.0 and tr.pad == 0 and va.rotate == 0.0
    seen = []
    for b in tr:
        assert set(b) == {"image", "target", "index"}
        k = b["index"].shape[0]
        assert b["image"].shape == (k, 3, 64, 64) and b["image"].dtype == torch.float32
        assert b["image"].is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(b["target"], tr.y[b["index"]])
        seen.append(b["index"])
    assert sorted(torch.cat(seen).tolist()) == list(range(9))
    # validation is the plain normalise of the packed rows, in folder order
    img, tgt = next(iter(va))
    rx, ry, _ = _decode_all(tiny_root / "tiny-imagenet-200" / "val")
    ref = (torch.from_numpy(rx[:4]).permute(0, 3, 1, 2).float() / 255
           - torch.tensor(TINY_MEAN).view(1, 3, 1, 1)) / torch.tensor(TINY_STD).view(1, 3, 1, 1)
    torch.testing.assert_close(img, ref)
    assert tgt.tolist() == ry[:4].tolist()


def test_dispatch_crd_and_folder_path(tiny_root):
    tr, _, _, _ = get_dataset(_cfg(tiny_root, crd=True), "cpu")
    assert isinstance(tr, DeviceImageLoader) and tr.crd.mode == "exact" and tr.crd.replace
    for b in tr:
        k = b["index"].shape[0]
        assert b["contrastive_index"].shape == (k, 6)
        assert torch.equal(b["contrastive_index"][:, 0], b["index"])
        neg = b["contrastive_index"][:, 1:]
        assert (tr.y[neg] != b["target"].view(-1, 1)).all()
    tr, va, n, _ = get_dataset(_cfg(tiny_root, gpu_aug=False), "cpu")
    assert isinstance(tr, torch.utils.data.DataLoader) and isinstance(va, torch.utils.data.DataLoader)
    assert n == 9
    img, tgt, idx = next(iter(tr))
    assert img.shape == (4, 3, 64, 64) and idx.shape == (4,)


def test_pad_with_rotate_is_refused():
    x = _images(4)
    with pytest.raises(ValueError):
        DeviceImageLoader(x, np.zeros(4), 2, "cpu", train=True, pad=4, rotate=20)
    with pytest.raises(ValueError):
        DeviceImageLoader(x, np.zeros(4), 2, "cpu", train=True, rotate=20)  # pad defaults to 4


def test_rotation_stream_is_a_function_of_seed_and_epoch():
    x = _images(24, seed=3)
    y = np.arange(24) % 5

    def epoch(ld, e):
        ld.set_epoch(e)
        return [(b["image"].clone(), b["index"].clone()) for b in ld]

    a = DeviceImageLoader(x, y, 8, "cpu", train=True, pad=0, rotate=20, seed=11)
    b = DeviceImageLoader(x, y, 8, "cpu", train=True, pad=0, rotate=20, seed=11)
    list(a)  # a has run an epoch already (a resumed run has not): the stream must not depend on it
    ea, eb = epoch(a, 3), epoch(b, 3)
    assert len(ea) == 3
    for (xa, ia), (xb, ib) in zip(ea, eb):
        assert torch.equal(ia, ib) and torch.equal(xa, xb)
    e4 = epoch(b, 4)
    assert any(not torch.equal(p[0], q[0]) for p, q in zip(eb, e4))
    # the angles themselves change with the epoch, not only the shuffle
    b.gen.manual_seed(b._epoch_seed(3))
    d3 = torch.rand(8, generator=b.gen)
    b.gen.manual_seed(b._epoch_seed(4))
    assert not torch.equal(d3, torch.rand(8, generator=b.gen))
    # rotated batches really are rotated: some corner pixel is fill (raw 0 -> -mean/std)
    fill = -torch.tensor(a._mean) / torch.tensor(a._std)
    corners = torch.cat([p[0] for p in ea])[:, :, 0, 0]
    assert (corners - fill).abs().max(dim=1).values.min() < 1e-6
