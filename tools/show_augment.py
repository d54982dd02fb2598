#!/usr/bin/env python3
"""Contact sheet of augmented training items: the first batch of epoch 0 of the resident folder dataset under an
--augment spec, each image with the edge of ITS mask drawn over it -- how a person checks that image and mask move
together.  Runs on the GPU when there is one (the batch kernel), else on the CPU (the same arithmetic); PIL only.

Usage: python tools/show_augment.py --data-dir data --img-size 512 512 --augment hflip+affine+color -n 8 --out sheet.png
       (--data-dir holds train_hq/ and train_masks/, like train.py's)"""
import argparse
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from distributedpytorch_amd.data import DeviceFolderDataset, device_folder_loaders  # noqa: E402
from distributedpytorch_amd.data.augment import MAGNITUDES, AugmentSpec  # noqa: E402


def mask_edge(m: np.ndarray) -> np.ndarray:
    """True on mask pixels with a 4-neighbour outside the mask."""
    inside = m > 0
    p = np.pad(inside, 1, mode="edge")
    return inside & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--img-size", type=int, nargs="+", default=[512, 512], help="H [W]")
    ap.add_argument("--augment", default="hflip+affine+color")
    ap.add_argument("-n", type=int, default=8, help="items on the sheet (the batch size)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--device", default=None)
    ap.add_argument("--out", default="sheet.png")
    for m in MAGNITUDES:
        ap.add_argument(f"--aug-{m}", type=float, default=None)
    a = ap.parse_args(argv)
    h, w = (a.img_size[0], a.img_size[0]) if len(a.img_size) == 1 else a.img_size[:2]
    try:
        spec = AugmentSpec.parse(a.augment, **{m: getattr(a, f"aug_{m}") for m in MAGNITUDES})
    except ValueError as e:
        ap.error(str(e))
    device = a.device or ("cuda" if torch.cuda.is_available() else "cpu")
    ds = DeviceFolderDataset(os.path.join(a.data_dir, "train_hq"), os.path.join(a.data_dir, "train_masks"),
                             newsize=(w, h), mask_suffix="_mask", device=device)
    loader, _, sampler = device_folder_loaders(ds, ds, a.n, seed=a.seed, augment=spec)
    sampler.set_epoch(0)
    img, tgt = next(iter(loader))
    img = (img.cpu().numpy() * 255.0).round().clip(0, 255).astype(np.uint8)           # [B, C, H, W]
    tgt = tgt.cpu().numpy()[:, 0]
    n = img.shape[0]
    cols = min(4, n)
    rows = -(-n // cols)
    sheet = Image.new("RGB", (cols * w, rows * h))
    for k in range(n):
        rgb = np.repeat(img[k], 3, axis=0) if img.shape[1] == 1 else img[k]
        tile = np.ascontiguousarray(rgb.transpose(1, 2, 0))
        tile[mask_edge(tgt[k])] = (255, 0, 255)
        sheet.paste(Image.fromarray(tile), ((k % cols) * w, (k // cols) * h))
    sheet.save(a.out)
    print(f"{a.out}: {n} items of epoch 0, augment {spec.describe()}, {h}x{w} on {device}")
    return a.out


if __name__ == "__main__":
    main()
