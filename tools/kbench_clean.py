#!/usr/bin/env python3
"""Kernel timing: dpa_mask_clean (csrc/mask_clean.hip) on realistic masks, beside the host reference.

Per batch size a batch of masks at the source size: an ellipse with a window hole, XOR speckle at `--speckle`
(default 0.05 % of the pixels), a different seed per image.  The device result is compared with
`ops.kernels.clean_reference` first; then `largest`, `fill` and `largest+fill` are warmed up and timed (HIP events
around `--inner` back-to-back calls, workspace allocation included as in `Predictor.post`), and the median, the
fastest and the slowest round are printed per call and per image.  The host arms -- `clean_reference` and, where it
is installed, scipy.ndimage (`label` with a 3 x 3 structure + `binary_fill_holes`) -- run on one core over the same
masks.

Usage: python tools/kbench_clean.py [--size 1280x1918] [--batches 4 16] [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from distributedpytorch_amd.ops import kernels as K  # noqa: E402


def realistic_mask(H, W, seed, speckle):
    y, x = np.mgrid[:H, :W]
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    m = ((y - cy) / (0.35 * H)) ** 2 + ((x - cx) / (0.4 * W)) ** 2 <= 1.0
    m &= ~((abs(y - cy + H / 8.0) <= H / 14.0) & (abs(x - cx) <= W / 8.0))           # the window
    m ^= np.random.default_rng(seed).random((H, W)) < speckle
    return m.astype(np.uint8) * 255


def scipy_clean(ndi, m):
    lab, n = ndi.label(m != 0, structure=np.ones((3, 3)))
    keep = lab == int(np.argmax(np.bincount(lab.ravel())[1:])) + 1 if n else lab > 0
    return ndi.binary_fill_holes(keep)


def bench(H, W, B, reps, warmup, inner, speckle):
    host = np.stack([realistic_mask(H, W, 100 + b, speckle) for b in range(B)])
    masks = torch.from_numpy(host).cuda()
    t0 = time.perf_counter()
    refs = [K.clean_reference(m) for m in host]
    t_ref = (time.perf_counter() - t0) / B
    got, st = K.mask_clean(masks, True, True)
    assert np.array_equal(got.cpu().numpy(), np.stack([r[0] for r in refs])), "mask_clean differs from clean_reference"
    assert st.cpu().numpy().tolist() == [r[1].tolist() for r in refs]
    stats = np.stack([r[1] for r in refs])
    print(f"size {H}x{W} batch {B}: per image {stats[:, 0].mean():.0f} components, {stats[:, 1].mean():.0f} pixels "
          f"removed, {stats[:, 2].mean():.0f} filled; the device result equals clean_reference")
    print(f"  clean_reference (numpy, one core)   {t_ref * 1e3:8.1f} ms per image")
    try:
        import scipy.ndimage as ndi
        t0 = time.perf_counter()
        sp = [scipy_clean(ndi, m) for m in host]
        t_sp = (time.perf_counter() - t0) / B
        assert all(np.array_equal(s, r[0] != 0) for s, r in zip(sp, refs))
        print(f"  scipy.ndimage (one core)            {t_sp * 1e3:8.1f} ms per image")
    except ImportError:
        print("  scipy is not installed: no scipy arm")
    arms = {"largest": (True, False), "fill": (False, True), "largest+fill": (True, True)}
    for _ in range(warmup):
        for flags in arms.values():
            K.mask_clean(masks, *flags)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {k: [] for k in arms}
    for _ in range(reps):
        for k, flags in arms.items():
            s.record()
            for _ in range(inner):
                K.mask_clean(masks, *flags)
            e.record()
            torch.cuda.synchronize()
            ts[k].append(s.elapsed_time(e) * 1e3 / inner)
    for k, v in ts.items():
        med = float(np.median(v))
        print(f"  mask_clean {k:13s} median {med:8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  "
              f"{med / B:7.1f} us per image  x{t_ref * 1e6 / (med / B):.0f} against clean_reference", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x1918", help="HxW")
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--speckle", type=float, default=0.0005)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_clean.py times GPU kernels: no GPU found"
    H, W = (int(v) for v in a.size.split("x"))
    for B in a.batches:
        bench(H, W, B, a.reps, a.warmup, a.inner, a.speckle)


if __name__ == "__main__":
    main()
