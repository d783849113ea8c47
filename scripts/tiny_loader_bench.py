#!/usr/bin/env python
"""Tiny-ImageNet data delivery: PIL folder loader vs the device-resident loader.

    python scripts/tiny_loader_bench.py [--images 4096] [--batch 256] [--workers 16]
                                        [--rank-workers 2] [--out FILE.md]

Writes random 64x64 JPEGs into a temporary ``tiny-imagenet-200/{train,val}``
class-folder tree and measures, on one GPU,

* passes at ``--batch`` through the folder loader (``DATASET.GPU_AUG False``,
  ``NUM_WORKERS`` = ``--workers``, then ``--rank-workers``), every batch copied
  to the device;
* the one-time pack of the tree, the cached reload, and one pass through the
  device loader (``DATASET.GPU_AUG True``);
* ``mda_rotate_flip_norm`` alone at B = ``--batch`` next to
  ``mda_crop_flip_norm`` at the same shape (graph-replayed, device events).

The table goes to ``--out`` (default ``profiles/tiny_device_loader.md``).
Loader workers are started by a fork server, so they never share the parent's
open GPU.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

README_FASTEST_TINY_MS = 14.31  # DOT R18 -> ShuffleV2, batch 256 (README table)


def write_tree(root, n_train, n_val, n_classes):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    for split, n in (("train", n_train), ("val", n_val)):
        for c in range(n_classes):
            os.makedirs(os.path.join(root, "tiny-imagenet-200", split, f"n{c:04d}", "images"))
        for i in range(n):
            # smooth noise (about 2 kB a file), not incompressible static
            a = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
            img = Image.fromarray(a).resize((64, 64), Image.BICUBIC)
            c = i % n_classes
            img.save(os.path.join(root, "tiny-imagenet-200", split, f"n{c:04d}", "images",
                                  f"n{c:04d}_{i}.JPEG"), quality=90)


def cfg_for(root, gpu_aug, batch, workers):
    from mdistiller_ddp_amd.config import get_cfg
    cfg = get_cfg()
    cfg.DATASET.TYPE = "tiny_imagenet"
    cfg.DATASET.ROOT = root
    cfg.DATASET.GPU_AUG = gpu_aug
    cfg.DATASET.NUM_WORKERS = workers
    cfg.SOLVER.BATCH_SIZE = batch
    cfg.DATASET.TEST.BATCH_SIZE = batch
    cfg.EXPERIMENT.SEED = 0
    return cfg


def one_pass(loader, dev):
    """(seconds, batches, images) for one epoch, every batch resident on ``dev`` at the end."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nb = ni = 0
    for b in loader:
        img = b["image"] if isinstance(b, dict) else b[0]
        img = img.to(dev, non_blocking=True)
        nb += 1
        ni += img.shape[0]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, nb, ni


def kernel_us(fn, iters=400):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(20):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters // 20):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def time_kernels(batch):
    import torch
    from mdistiller_ddp_amd.data.cifar100 import rotate_coef
    from mdistiller_ddp_amd.ops import _ext
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    n, h, w, c = 8192, 64, 64, 3
    x = torch.randint(0, 256, (n, h, w, c), generator=g, device=dev, dtype=torch.uint8)
    idx = torch.randint(0, n, (batch,), generator=g, device=dev)
    flip = torch.randint(0, 2, (batch,), generator=g, device=dev, dtype=torch.uint8)
    offs = torch.randint(0, 9, (batch, 2), generator=g, device=dev, dtype=torch.int32)
    coef = rotate_coef((torch.rand(batch, generator=g, device=dev) * 2 - 1) * 20, h, w)
    mean = torch.tensor([0.4802, 0.4481, 0.3975], device=dev)
    inv = 1.0 / torch.tensor([0.2302, 0.2265, 0.2262], device=dev)
    rows = []
    for dt, name, size in ((1, "bf16", 2), (0, "fp32", 4)):
        out = torch.empty(batch, h, w, c, device=dev, dtype=torch.bfloat16 if dt else torch.float32)
        rot = kernel_us(lambda: _ext.call("mda_rotate_flip_norm", x, idx, coef, flip, mean, inv, out,
                                          dt, batch, h, w, c))
        crop = kernel_us(lambda: _ext.call("mda_crop_flip_norm", x, idx, offs, flip, mean, inv, out,
                                           dt, batch, h, w, c, 4))
        moved = batch * h * w * c * (1 + size)  # uint8 in, out_dtype out
        rows.append((name, rot, crop, moved))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--val-images", type=int, default=512)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--rank-workers", type=int, default=2,
                    help="second folder-loader row: the workers one rank of eight gets from 16 CPUs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiny_device_loader.md"))
    args = ap.parse_args()

    import torch
    import torch.multiprocessing as mp
    mp.set_start_method("forkserver", force=True)
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    from mdistiller_ddp_amd.data import get_dataset
    from mdistiller_ddp_amd.data.tiny_imagenet import load_tiny_imagenet
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_tree(root, args.images, args.val_images, args.classes)
        print(f"wrote {args.images}+{args.val_images} JPEGs in {time.perf_counter() - t0:.1f} s", flush=True)

        # folder path: the first pass also starts the workers; the later ones are steady state
        folder = []
        for nw in (args.workers, args.rank_workers):
            tr, _, n, _ = get_dataset(cfg_for(root, False, args.batch, nw), dev)
            first = one_pass(tr, dev)
            steady = sorted(one_pass(tr, dev) for _ in range(5))
            del tr
            folder.append((nw, first, steady[0], steady[-1]))
            print(f"folder loader, {nw} workers: first pass {first[0]:.2f} s, steady "
                  f"{steady[0][0]:.3f}-{steady[-1][0]:.3f} s ({first[2]} images, {first[1]} batches)",
                  flush=True)

        # device path: pack once, reload from the cache, then passes of the loader
        t0 = time.perf_counter()
        load_tiny_imagenet(root, "train")
        t_pack = time.perf_counter() - t0
        t0 = time.perf_counter()
        load_tiny_imagenet(root, "train")
        t_cached = time.perf_counter() - t0
        tr, _, n, _ = get_dataset(cfg_for(root, True, args.batch, 0), dev)
        one_pass(tr, dev)  # warm-up: code objects, allocator
        passes = []
        for e in range(1, 6):
            tr.set_epoch(e)
            passes.append(one_pass(tr, dev))
        d_best = min(passes, key=lambda p: p[0])
        d_worst = max(passes, key=lambda p: p[0])
        print(f"device loader: pack {t_pack:.2f} s, cached load {t_cached:.3f} s, pass "
              f"{d_best[0] * 1e3:.2f}-{d_worst[0] * 1e3:.2f} ms ({d_best[2]} images)", flush=True)

    rows = time_kernels(args.batch)
    for name, rot, crop, moved in rows:
        print(f"kernel {name}: rotate {rot:.2f} us, crop {crop:.2f} us", flush=True)

    def ms(p):
        return p[0] * 1e3 / p[1]

    d_ms, d_ms_worst = ms(d_best), ms(d_worst)
    verdict = ("below" if d_ms_worst < README_FASTEST_TINY_MS else "NOT below")
    need = 256 / README_FASTEST_TINY_MS * 1e3
    lines = [
        "# Tiny-ImageNet data delivery: folder loader vs device-resident loader",
        "",
        f"`python scripts/tiny_loader_bench.py --images {args.images} --batch {args.batch} "
        f"--workers {args.workers} --rank-workers {args.rank_workers}` on one MI355X, "
        f"torch {torch.__version__}.",
        "",
        f"{args.images} random 64x64 JPEGs in {args.classes} class folders; one pass = "
        f"{d_best[1]} batches of {args.batch}, every batch on the device at the end "
        "(host clock around a device synchronise). Steady rows are the best and the slowest of 5 "
        "passes after a first one.",
        "",
        "| path | ms / batch (best - slowest) | img/s (best) | note |",
        "|---|---:|---:|---|",
    ]
    for nw, first, best, worst in folder:
        lines += [
            f"| folder loader, {nw} PIL workers, steady | {ms(best):.2f} - {ms(worst):.2f} | "
            f"{best[2] / best[0]:,.0f} | fp32 batches, pinned host -> device copy |",
            f"| folder loader, {nw} PIL workers, first pass | {ms(first):.2f} | "
            f"{first[2] / first[0]:,.0f} | includes starting the workers |"]
    lines += [
        f"| device loader (`mda_rotate_flip_norm`), steady | {d_ms:.3f} - {d_ms_worst:.3f} | "
        f"{d_best[2] / d_best[0]:,.0f} | fp32 NHWC batches: index upload + draws + kernel |",
        "",
        f"One-time pack of the {args.images}-image tree (PIL decode, 16 threads): {t_pack:.2f} s "
        f"({args.images / t_pack:,.0f} img/s); reload from the cache: {t_cached * 1e3:.0f} ms.",
        "",
        f"The fastest Tiny-ImageNet step in the README is {README_FASTEST_TINY_MS} ms at batch 256 "
        f"({need:,.0f} img/s per GPU). The device loader's per-batch time is **{verdict}** it "
        f"({d_ms_worst:.3f} ms at worst, {README_FASTEST_TINY_MS / d_ms_worst:.0f}x margin). The "
        "folder rates are recorded for the comparison only: "
        + "; ".join(f"{nw} workers deliver {best[2] / best[0] / need:.2f}x the rate that step consumes"
                    for nw, _, best, _ in folder)
        + f". {args.workers} workers is one rank with a 16-CPU job to itself, {args.rank_workers} is "
        "the share of one rank of eight.",
        "",
        f"## Kernels alone, B = {args.batch}, 64x64x3 (graph replay of 20 launches, device events)",
        "",
        "| out dtype | `mda_rotate_flip_norm` us | `mda_crop_flip_norm` (pad 4) us | bytes moved | rotate GB/s |",
        "|---|---:|---:|---:|---:|",
    ]
    for name, rot, crop, moved in rows:
        lines.append(f"| {name} | {rot:.2f} | {crop:.2f} | {moved / 1e6:.1f} MB | {moved / rot / 1e3:,.0f} |")
    lines += ["",
              "The time is that of one launch in a replayed graph of 20, so it includes the gap "
              "between graph nodes; bytes are the uint8 pixels read plus the batch written.",
              "",
              "## Notes",
              "",
              "- The workers are not pinned to CPUs. On a host with more cores than the job's share the "
              "folder rows are an upper bound for that path.",
              "- The rotate kernel does more integer work per pixel than the crop (a 64-bit affine map "
              "against two adds) and, for bf16 with C = 3, writes 12 contiguous bytes per lane where the "
              "crop writes three 2-byte values. Which of the two explains each difference above was not "
              "profiled.",
              ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
