#!/usr/bin/env python3
"""Kernel timing: dpa_prob_score (csrc/predict_post.hip) against the composition it replaces, at one shape in one
process.

Per shape a batch of random probabilities at the network size and a blob ground truth at the source size.  The
arms, for T = 1 and T = 8 thresholds:

  prob_score  one launch: resize, compare with every threshold and with the truth, count; no mask exists
  unfused     per threshold dpa_prob_to_mask_u8 into a [B, H, W] mask, then torch: count_nonzero of the mask and
              of mask & truth per image (the truth's own comparison and count once per call)

are warmed up and then timed interleaved (every arm once per round, HIP events around `--inner` back-to-back
calls), and the median, the fastest and the slowest round are printed with the ratio to prob_score at the same T.
The results are compared before they are timed.

Usage: python tools/kbench_score.py [--shapes 640x960:1280x1918x32] [--reps 30]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from distributedpytorch_amd.ops import kernels as K  # noqa: E402


def unfused(probs, truth, cut, thresholds, mask):
    tb = truth > cut.view(-1, 1, 1).to(torch.uint8)
    cols = [torch.count_nonzero(tb, dim=(1, 2))]
    for t in thresholds:
        assert K.prob_to_mask_u8(probs, mask, t, 255)
        cols += [torch.count_nonzero(mask, dim=(1, 2)), torch.count_nonzero(mask.bool() & tb, dim=(1, 2))]
    return torch.stack(cols, 1)


def bench_shape(h, w, H, W, B, reps, warmup, inner):
    g = torch.Generator().manual_seed(h + W + B)
    probs = torch.rand(B, h, w, generator=g).cuda()
    truth = (torch.rand(B, (H * W + 4) // 5, generator=g) < 0.4).repeat_interleave(5, dim=1)[:, :H * W]
    truth = (truth.view(B, H, W).to(torch.uint8) * 255).cuda()
    cut = torch.full((B,), 127, dtype=torch.int32).cuda()
    mask = torch.empty(B, H, W, dtype=torch.uint8, device="cuda")
    sets = {1: [0.5], 8: [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]}
    arms = {}
    for T, thr in sets.items():
        arms[f"prob_score T={T}"] = lambda thr=thr: K.prob_score(probs, truth, cut, thr)
        arms[f"unfused    T={T}"] = lambda thr=thr: unfused(probs, truth, cut, thr, mask)
        a, b = arms[f"prob_score T={T}"](), arms[f"unfused    T={T}"]()
        assert a is not None and torch.equal(a, b), f"T={T}: prob_score differs from the unfused composition"
        assert bool((a[:, 2] > 0).all()) and bool((a[:, 2] < torch.minimum(a[:, 0], a[:, 1])).all())
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
    read = B * (h * w * 4 + H * W)
    print(f"shape {h}x{w} -> {H}x{W} batch {B}: prob_score reads {read / 1e6:.1f} MB (float32 probabilities + truth "
          f"bytes), a mask is {B * H * W / 1e6:.1f} MB; {reps} interleaved rounds of {inner} calls")
    for k, v in ts.items():
        med = float(np.median(v))
        ref = float(np.median(ts["prob_score T=" + k.split("=")[1]]))
        print(f"  {k:16s} median {med:8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  x{med / ref:.2f} of prob_score "
              f"at that T", flush=True)
    one, eight = (float(np.median(ts[f"prob_score T={T}"])) for T in (1, 8))
    print(f"  seven more thresholds cost prob_score {eight - one:+.1f} us ({eight / one:.2f}x of T=1)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["640x960:1280x1918x32"], help="hxw:HxWxB")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_score.py times GPU kernels: no GPU found"
    for shape in a.shapes:
        src, dst = shape.split(":")
        h, w = (int(v) for v in src.split("x"))
        H, W, B = (int(v) for v in dst.split("x"))
        bench_shape(h, w, H, W, B, a.reps, a.warmup, a.inner)


if __name__ == "__main__":
    main()
