"""Tiny-ImageNet as a device-resident loader.

Reference: ``dataset/tiny_imagenet.py`` -- ``ImageFolderInstance`` /
``ImageFolderInstanceSample`` over ``tiny-imagenet-200/{train,val}``
(``:14-71``), train transform RandomRotation(20) + HFlip + ToTensor +
Normalize (``:76-81``), test ToTensor + Normalize.

MI355X design: the train set is 100000 x 64 x 64 x 3 uint8 = 1.23 GB, under
half a percent of HBM, so the CIFAR design (``cifar100.py``) carries over.
The folder tree is decoded ONCE into a uint8 array cached next to the split
folder (:func:`load_tiny_imagenet`); the array is uploaded once and each batch
is a gather + rotate + flip + normalise done by one HIP kernel
(``ops/csrc/aug.hip::mda_rotate_flip_norm``) straight into the NHWC layout
the convs read.  The rotation is nearest neighbour with fill 0 like the
reference's, evaluated in 16.16 fixed point at pixel centres as PIL does.
``DATASET.GPU_AUG False`` keeps the PIL worker path of ``imagefolder.py``.
"""
from __future__ import annotations

import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .cifar100 import (DeviceImageLoader, rotate_coef, rotate_flip_ref,  # noqa: F401 (re-exported)
                       rotate_flip_u8_ref)
from .common import CRDSampler, data_root
from .imagefolder import scan_folder
from .synthetic import TINY_MEAN, TINY_STD

TINY_HW = 64
TINY_ROTATE = 20.0
_PACK_THREADS = 16  # a job's CPU share, not the machine's core count


def _tree_hash(split_dir: str, samples) -> str:
    """Hash of the relative paths and file sizes of ``samples`` (scan order)."""
    h = hashlib.sha256()
    for path, _ in samples:
        h.update(f"{os.path.relpath(path, split_dir)}\0{os.path.getsize(path)}\n".encode())
    return h.hexdigest()


def _decode(path: str) -> np.ndarray:
    from PIL import Image
    with open(path, "rb") as f:
        a = np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8)
    if a.shape != (TINY_HW, TINY_HW, 3):
        raise ValueError(f"{path}: expected a {TINY_HW}x{TINY_HW} image, got {a.shape[1]}x{a.shape[0]}")
    return a


def _read_cache(npy: str, side: str, n: int, classes, digest: str):
    """The cached array when the sidecar matches the tree as scanned now, else None."""
    try:
        with open(side) as f:
            meta = json.load(f)
        if meta.get("n") != n or meta.get("classes") != list(classes) or meta.get("hash") != digest:
            return None
        x = np.load(npy, allow_pickle=False)
    except (OSError, ValueError, EOFError):
        return None  # missing, truncated or not an array file: rebuild
    if x.dtype != np.uint8 or x.shape != (n, TINY_HW, TINY_HW, 3):
        return None
    return x


def _write_atomic(path: str, write) -> None:
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            write(f)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _pack(samples, npy: str, side: str, classes, digest: str) -> np.ndarray:
    x = np.empty((len(samples), TINY_HW, TINY_HW, 3), dtype=np.uint8)

    def one(i):
        x[i] = _decode(samples[i][0])

    with ThreadPoolExecutor(max_workers=_PACK_THREADS) as ex:
        list(ex.map(one, range(len(samples)), chunksize=256))
    meta = {"n": len(samples), "classes": list(classes), "hash": digest}
    # the sidecar goes last: it vouches for an array that is already in place
    if os.path.exists(side):
        os.remove(side)
    _write_atomic(npy, lambda f: np.save(f, x, allow_pickle=False))
    _write_atomic(side, lambda f: f.write(json.dumps(meta).encode()))
    return x


def load_tiny_imagenet(root: str, split: str):
    """-> (uint8 [N, 64, 64, 3] NHWC, int64 [N], classes) of
    ``<root>/tiny-imagenet-200/<split>/<class>/...``.

    Sample order and class indices are :func:`~.imagefolder.scan_folder`'s, so
    they equal ``ImageFolderInstance``'s.  The first call decodes every file
    with PIL and writes ``<split>_u8.npy`` and the sidecar ``<split>_u8.json``
    (sample count, class list, hash of relative paths and file sizes) next to
    the split folder; later calls load the array without opening an image as
    long as the sidecar matches a fresh scan.  With several ranks, rank 0
    packs while the others wait on the process group, then every rank loads.
    """
    from ..parallel import dist as D
    base = os.path.join(root, "tiny-imagenet-200")
    split_dir = os.path.join(base, split)
    if not os.path.isdir(split_dir):
        raise FileNotFoundError(
            f"Tiny-ImageNet not found under {root} (expected tiny-imagenet-200/{split}/<class>/...); "
            "there is no download in this framework -- place the files there or set DATASET.SYNTHETIC")
    samples, classes = scan_folder(split_dir)
    if not samples:
        raise FileNotFoundError(f"no images under {split_dir}")
    labels = np.asarray([t for _, t in samples], dtype=np.int64)
    digest = _tree_hash(split_dir, samples)
    npy = os.path.join(base, f"{split}_u8.npy")
    side = os.path.join(base, f"{split}_u8.json")
    x, err = None, None
    if D.is_master():
        try:
            x = _read_cache(npy, side, len(samples), classes, digest)
            if x is None:
                x = _pack(samples, npy, side, classes, digest)
        except Exception as e:  # release the waiting ranks before failing
            err = e
    D.barrier()
    if err is not None:
        raise err
    if x is None:
        x = _read_cache(npy, side, len(samples), classes, digest)
        if x is None:
            raise RuntimeError(f"rank {D.get_rank()}: no valid cache at {npy} after rank 0 packed {split_dir}")
    return x, labels, classes


def get_tiny_device_loaders(cfg, device, crd: bool):
    """(train, val, num_data): device-resident Tiny-ImageNet, rotate(20) + flip on train."""
    root = data_root(cfg)
    xtr, ytr, classes = load_tiny_imagenet(root, "train")
    xva, yva, _ = load_tiny_imagenet(root, "val")
    # the folder path's CRD sampling (imagefolder.get_folder_dataloaders)
    sampler = (CRDSampler(ytr, len(classes), cfg.CRD.NCE.K, mode="exact", replace=True,
                          seed=max(cfg.EXPERIMENT.SEED, 0)) if crd else None)
    train = DeviceImageLoader(xtr, ytr, cfg.SOLVER.BATCH_SIZE, device, train=True, mean=TINY_MEAN,
                              std=TINY_STD, pad=0, rotate=TINY_ROTATE, crd=sampler,
                              seed=max(cfg.EXPERIMENT.SEED, 0))
    val = DeviceImageLoader(xva, yva, cfg.DATASET.TEST.BATCH_SIZE, device, train=False,
                            mean=TINY_MEAN, std=TINY_STD, pad=0)
    return train, val, len(ytr)
