#!/usr/bin/env python3
"""Batch-kernel timing: dpa_batch_augment_u8 (csrc/augment.hip) against dpa_batch_gather_u8 (csrc/data_prep.hip),
which writes the same float32 batch, at the same shape in one process.

Per shape a resident set of --items random uint8 images is gathered by a random index batch.  The arms -- the plain
gather, then the augment kernel with identity matrices and with matrices drawn at the default magnitudes, each
without and with per-item tone tables -- are warmed up and then timed interleaved (every arm once per round, HIP
events around five back-to-back launches), and the median, the fastest and the slowest round are printed with
the output bytes per second and the ratio to the plain gather.  The results are compared before they are timed.

Usage: python tools/kbench_augment.py [--shapes 512x512x256 640x960x128] [--reps 50]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from distributedpytorch_amd.data.augment import AugmentSpec, affine_matrices, color_luts  # noqa: E402
from distributedpytorch_amd.ops import kernels as K  # noqa: E402


def bench_shape(H, W, B, items, reps, warmup, inner=5):
    g = torch.Generator().manual_seed(H + W + B)
    images = torch.randint(0, 256, (items, 3, H, W), dtype=torch.uint8, generator=g).cuda()
    masks = torch.randint(0, 2, (items, H, W), dtype=torch.uint8, generator=g).cuda()
    base = torch.randint(0, items, (B,), generator=g)
    idx = base.cuda()
    spec = AugmentSpec.parse("hflip+affine+color")
    ident = torch.tensor([[65536, 0, 0, 0, 65536, 0]] * B, dtype=torch.int32).cuda()
    drawn = torch.from_numpy(affine_matrices(spec, 42, 0, base.numpy(), H, W)).cuda()
    luts = torch.from_numpy(color_luts(spec, 42, 0, base.numpy())).cuda()
    out = (torch.empty(B, 3, H, W, device="cuda"), torch.empty(B, 1, H, W, device="cuda"))
    arms = {
        "gather (plain)": lambda: K.batch_gather_u8(images, masks, idx, None),
        "augment identity": lambda: K.batch_augment_u8(images, masks, idx, ident, None, out=out),
        "augment identity+luts": lambda: K.batch_augment_u8(images, masks, idx, ident, luts, out=out),
        "augment default": lambda: K.batch_augment_u8(images, masks, idx, drawn, None, out=out),
        "augment default+luts": lambda: K.batch_augment_u8(images, masks, idx, drawn, luts, out=out),
    }
    pi, pt = arms["gather (plain)"]()
    ai, at = arms["augment identity"]()
    assert torch.equal(pi, ai) and torch.equal(pt, at), "identity warp differs from the plain gather"
    del pi, pt
    for _ in range(warmup):
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            s.record()
            for _ in range(inner):           # back to back: the host's launch latency hides behind the first
                f()
            e.record()
            torch.cuda.synchronize()
            ts[k].append(s.elapsed_time(e) * 1e3 / inner)
    out_bytes = B * 4 * H * W * 4
    ref = float(np.median(ts["gather (plain)"]))
    print(f"shape {H}x{W} batch {B}: {out_bytes / 1e9:.3f} GB float32 written per launch, {items} resident items, "
          f"{reps} interleaved rounds of {inner} launches")
    for k, v in ts.items():
        med = float(np.median(v))
        print(f"  {k:24s} median {med:8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  "
              f"{out_bytes / med / 1e3:7.1f} GB/s written  x{med / ref:.2f} of the plain gather", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["512x512x256", "640x960x128"], help="HxWxB")
    ap.add_argument("--items", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_augment.py times GPU kernels: no GPU found"
    for shape in a.shapes:
        H, W, B = (int(v) for v in shape.split("x"))
        bench_shape(H, W, B, a.items, a.reps, a.warmup)


if __name__ == "__main__":
    main()
