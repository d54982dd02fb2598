"""Prediction: a trained checkpoint and image files in, full-size masks and run-length lists out.

The reference has no predict script; a Carvana-layout project is expected to deliver one mask per
input image at the SOURCE resolution plus the run-length CSV the dataset is scored with.

:class:`Predictor` runs the eval-mode forward exactly as ``evaluate.py`` does (``TrainConfig`` +
``SingleDevice``, ``compute.probs`` under ``no_grad``).  :meth:`Predictor.predict_files` decodes the files with a
bounded thread pool and, on a GPU, keeps everything behind the decode on the device:

* the source image is uploaded and resized to the network size by ``dpa_resize_bicubic_u8`` and converted
  through ``unit_table`` -- the training preprocessing, bit for bit (``data/device_folder.py``);
* one ``probs`` call per batch;
* per group of equal source sizes one ``dpa_prob_to_mask_u8`` launch (PIL's mode-``F`` bilinear resize to the
  source size and the strict ``> threshold``, bit-equal to PIL) and one ``dpa_mask_rle`` launch; only the run
  counts and the used prefixes of the run lists are downloaded (a few kilobytes against 2.4 MB for a 1918x1280
  mask), the masks themselves only when the caller wants them.

The host path -- PIL ``resize(BILINEAR)`` of the float32 probabilities, ``> threshold``, ``rle_reference`` --
defines the result.  It serves a CPU device, ``host_post=True`` (A/B comparison, debugging), a source size the
resize kernel refuses (down-scaling beyond 4x) and a run list that overflows its capacity; ``host_finished``
counts the files it finished.  Nothing is timed or synchronised per image: the downloads are per batch.
"""
from __future__ import annotations

import argparse
import csv
import logging
import os
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Iterator, Optional, Sequence

import numpy as np
import torch

from .data.folder import BasicDataset, _load_image

log = logging.getLogger(__name__)

_IMAGE_MODES = ("L", "RGB")       # what dpa_resize_bicubic_u8 covers (data/device_folder.py)


def host_mask(prob: np.ndarray, size, threshold: float = 0.5, value: int = 255) -> np.ndarray:
    """The definition of the full-size mask: float32 probabilities ``[h, w]`` resized by PIL (mode ``F``,
    BILINEAR) to ``size = (Hs, Ws)``, compared ``> float32(threshold)`` -> uint8 ``[Hs, Ws]`` of 0 / ``value``."""
    from PIL import Image
    Hs, Ws = size
    p = np.ascontiguousarray(prob, dtype=np.float32)
    r = np.asarray(Image.fromarray(p).resize((Ws, Hs), resample=Image.BILINEAR))      # float32 -> mode F
    return (r > np.float32(threshold)).astype(np.uint8) * np.uint8(value)


class Predictor:
    """Eval-mode forward of ``model`` at ``img_size = (H, W)`` plus the post-processing to source-size masks.

    ``host_post`` forces the host post-processing; ``rle_cap`` is the capacity of one device run list (default
    ``4 * source height``; a list that overflows it is finished on the host)."""

    def __init__(self, model, device, img_size, dtype: Optional[str] = None, backend: str = "auto",
                 threshold: float = 0.5, host_post: bool = False, rle_cap: Optional[int] = None):
        from .config import TrainConfig
        from .trainer import SingleDevice
        self.device = torch.device(device)
        self.on_gpu = self.device.type == "cuda"
        self.h, self.w = int(img_size[0]), int(img_size[-1])
        self.dtype = dtype or ("bf16" if self.on_gpu else "fp32")
        cfg = TrainConfig(backend=backend, img_size=(self.h, self.w), dtype=self.dtype)
        self.strat = SingleDevice(cfg, model, self.device)
        self.strat.set_train(False)
        self.channels = int(model.cfg.in_channels)
        self.threshold = float(threshold)
        self.host_post = bool(host_post) or not self.on_gpu
        self.rle_cap = None if rle_cap is None else int(rle_cap)
        assert self.rle_cap is None or self.rle_cap >= 1, "rle_cap must be positive"
        self.host_finished = 0          # files whose mask / run list the host path produced

    # ---- decode (worker threads) ------------------------------------------------------------------------
    def _decode(self, path):
        """((Hs, Ws), array, raw): the full-size uint8 ``[Hs, Ws, C]`` source for the resize kernel (``raw``), or
        the float32 ``[C, h, w]`` result of ``BasicDataset.preprocess`` on the CPU."""
        img = _load_image(Path(path))
        size = (img.size[1], img.size[0])
        if len(img.getbands()) != self.channels:
            raise ValueError(f"{path}: {len(img.getbands())} channels (mode {img.mode}), the model takes {self.channels}")
        if self.on_gpu and img.mode in _IMAGE_MODES:
            a = np.array(img)
            return size, (a if a.ndim == 3 else a[:, :, None]), True
        return size, self._cpu_image(img), False

    def _cpu_image(self, pil_img) -> np.ndarray:
        return BasicDataset.preprocess(pil_img, (self.w, self.h), is_mask=False).astype(np.float32)

    # ---- one batch ----------------------------------------------------------------------------------------
    def _inputs(self, items) -> torch.Tensor:
        """float32 ``[B, C, h, w]`` on the device: the training preprocessing of the decoded files."""
        B = len(items)
        x = torch.empty(B, self.channels, self.h, self.w, dtype=torch.float32, device=self.device)
        raw = [i for i, (_, _, r) in enumerate(items) if r]
        if raw:
            from .ops import kernels as K
            u8 = torch.empty(len(raw), self.channels, self.h, self.w, dtype=torch.uint8, device=self.device)
            kept = []
            for j, i in enumerate(raw):
                arr = items[i][1]
                if K.resize_bicubic_u8(torch.from_numpy(arr).to(self.device, non_blocking=True), u8[j]):
                    kept.append((j, i))
                else:                       # extreme down-scaling: PIL on the CPU, as DeviceFolderDataset does
                    from PIL import Image
                    pil = Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr)
                    items[i] = (items[i][0], self._cpu_image(pil), False)
            if kept:
                js = torch.tensor([j for j, _ in kept], device=self.device)
                dst = torch.tensor([i for _, i in kept], device=self.device)
                x[dst] = K.unit_table(self.device)[u8[js].long()]
        for i, (_, arr, r) in enumerate(items):
            if not r:
                x[i].copy_(torch.from_numpy(arr))
        return x

    @torch.no_grad()
    def probs(self, x: torch.Tensor) -> torch.Tensor:
        """float32 ``[B, h, w]`` probabilities of a preprocessed batch."""
        p = self.strat.compute.probs(x)
        assert p.dim() == 4 and p.shape[1] == 1, f"probs: expected [B, 1, h, w], got {tuple(p.shape)}"
        return p.to(torch.float32).reshape(p.shape[0], p.shape[2], p.shape[3]).contiguous()

    def _host_finish(self, prob: np.ndarray, size, want_masks: bool, want_rle: bool):
        from .ops.kernels import rle_reference
        self.host_finished += 1
        m = host_mask(prob, size, self.threshold)
        return (m if want_masks else None), (rle_reference(m) if want_rle else None)

    def post(self, probs: torch.Tensor, sizes: Sequence, want_masks: bool = True, want_rle: bool = True):
        """``probs`` float32 ``[B, h, w]`` -> per image ``(mask uint8 [Hs, Ws] or None, runs int32 [n, 2] or
        None)`` at ``sizes[i] = (Hs, Ws)``."""
        B = probs.shape[0]
        assert len(sizes) == B
        out = [None] * B
        if self.host_post:
            host = probs.cpu().numpy()
            return [self._host_finish(host[i], sizes[i], want_masks, want_rle) for i in range(B)]
        from .ops import kernels as K
        groups = {}
        for i, s in enumerate(sizes):
            groups.setdefault(tuple(s), []).append(i)
        todo, launched = [], []            # images for the host; (indices, masks, runs, counts) per group
        for (Hs, Ws), idx in groups.items():
            sel = probs if len(idx) == B else probs.index_select(0, torch.tensor(idx, device=probs.device))
            masks = torch.empty(len(idx), Hs, Ws, dtype=torch.uint8, device=probs.device)
            if not K.prob_to_mask_u8(sel, masks, self.threshold, 255):
                todo += idx
                continue
            runs = counts = None
            if want_rle:
                runs, counts = K.mask_rle(masks, self.rle_cap or 4 * Hs)
            launched.append((idx, masks, runs, counts))
        if want_rle and launched:
            # two small downloads for the whole batch: the counts, then the used prefixes of the run lists
            counts = torch.cat([c for _, _, _, c in launched]).cpu().numpy()
            parts, k = [], 0
            for idx, _, runs, _ in launched:
                for j in range(len(idx)):
                    n = int(counts[k + j])
                    if n <= runs.shape[1]:
                        parts.append(runs[j, :n])
                k += len(idx)
            flat = torch.cat(parts).cpu().numpy() if parts else np.zeros((0, 2), np.int32)
            k = pos = 0
            for idx, _, runs, _ in launched:
                for j, i in enumerate(idx):
                    n = int(counts[k + j])
                    if n <= runs.shape[1]:
                        out[i] = [None, flat[pos:pos + n].copy()]
                        pos += n
                    else:                   # overflow: nothing behind cap was written; the host encodes
                        todo.append(i)
                k += len(idx)
        for idx, masks, _, _ in launched:
            host = masks.cpu().numpy() if want_masks else None
            for j, i in enumerate(idx):
                if i in todo:
                    continue
                if out[i] is None:
                    out[i] = [None, None]
                if want_masks:
                    out[i][0] = host[j]
        if todo:
            sel = probs.index_select(0, torch.tensor(sorted(todo), device=probs.device)).cpu().numpy()
            for j, i in enumerate(sorted(todo)):
                out[i] = self._host_finish(sel[j], sizes[i], want_masks, want_rle)
        return [tuple(o) for o in out]

    # ---- files --------------------------------------------------------------------------------------------
    def predict_files(self, paths, batch_size: int = 4, workers: int = 0, want_masks: bool = True,
                      want_rle: bool = True) -> Iterator:
        """Yields ``(path, (Hs, Ws), mask uint8 [Hs, Ws] or None, runs int32 [n, 2] or None)`` per file, in input
        order.  ``workers``: decode threads; 0 means ``min(8, os.cpu_count())``; never more than 16."""
        paths = list(paths)
        batch_size = max(1, int(batch_size))
        workers = max(1, min(16, int(workers) if workers else min(8, os.cpu_count() or 1)))
        pending = deque()
        with ThreadPoolExecutor(workers) as pool:
            nxt = 0
            for b0 in range(0, len(paths), batch_size):
                chunk = paths[b0:b0 + batch_size]
                items = []
                for _ in chunk:
                    while nxt < len(paths) and len(pending) < max(2 * workers, batch_size):   # bounded: full-size sources
                        pending.append(pool.submit(self._decode, paths[nxt]))
                        nxt += 1
                    items.append(pending.popleft().result())
                sizes = [s for s, _, _ in items]
                res = self.post(self.probs(self._inputs(items)), sizes, want_masks, want_rle)
                for p, s, (m, r) in zip(chunk, sizes, res):
                    yield p, s, m, r


def list_inputs(inputs) -> list:
    """Files of ``--input``: a directory is listed sorted with dot-files skipped; files are taken as given."""
    out = []
    for p in inputs:
        if os.path.isdir(p):
            out += [os.path.join(p, f) for f in sorted(os.listdir(p))
                    if not f.startswith(".") and os.path.isfile(os.path.join(p, f))]
        else:
            out.append(p)
    return out


def rle_string(runs) -> str:
    return " ".join(str(int(v)) for v in np.asarray(runs).reshape(-1))


def main(argv=None):
    from .models.unet import build_model
    from .utils import load_model_state

    ap = argparse.ArgumentParser(description="Predict full-size masks and the run-length CSV from a UNet checkpoint")
    ap.add_argument("--checkpoint", "-c", default=None, help="checkpoints/<NAME>.pth")
    ap.add_argument("--load", "-l", default=None, help="explicit .pth path")
    ap.add_argument("--input", "-i", nargs="+", required=True, help="a directory (listed sorted, dot-files skipped) or files")
    ap.add_argument("--output", "-o", default=None, metavar="DIR", help="write DIR/<stem>_mask.png (mode L, 0/255, source size)")
    ap.add_argument("--rle", default=None, metavar="FILE.csv", help="write the run-length CSV (img,rle_mask)")
    ap.add_argument("--batch-size", "-b", type=int, default=4)
    ap.add_argument("--img-size", type=int, nargs="+", default=[640, 960])
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--num-workers", type=int, default=0, help="decode threads (0: min(8, cpus); at most 16)")
    ap.add_argument("--host-post", action="store_true",
                    help="post-process on the host (PIL + numpy): the fallback made selectable, for comparison")
    ap.add_argument("--out-dir", default=".", help="where checkpoints/ lives")
    ap.add_argument("--model", default="unet")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"])
    ap.add_argument("--dtype", default=None, choices=["bf16", "fp32"],
                    help="compute dtype (default bf16 on a GPU, fp32 on CPU; on a GPU fp32 runs the fp32 HIP engine)")
    a = ap.parse_args(argv)
    if not a.output and not a.rle:
        ap.error("nothing to write: give --output DIR and / or --rle FILE.csv")
    path = a.load or (os.path.join(a.out_dir, "checkpoints", f"{a.checkpoint}.pth") if a.checkpoint else None)
    if not path:
        ap.error("no checkpoint: give -c NAME or -l PATH")
    if not os.path.isfile(path):
        ap.error(f"checkpoint not found: {path}")
    files = list_inputs(a.input)
    if not files:
        ap.error(f"no input file found in {' '.join(a.input)}")
    missing = [f for f in files if not os.path.isfile(f)]
    if missing:
        ap.error(f"input file not found: {missing[0]}")

    model = build_model(a.model)
    load_model_state(model, path)
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    pred = Predictor(model, dev, (a.img_size[0], a.img_size[-1]), dtype=a.dtype, backend=a.backend,
                     threshold=a.threshold, host_post=a.host_post)
    if a.output:
        os.makedirs(a.output, exist_ok=True)
    rows = []
    t0 = time.perf_counter()
    for p, _, mask, runs in pred.predict_files(files, a.batch_size, a.num_workers, want_masks=bool(a.output),
                                               want_rle=bool(a.rle)):
        if a.output:
            from PIL import Image
            Image.fromarray(mask).save(os.path.join(a.output, Path(p).stem + "_mask.png"))
        if a.rle:
            rows.append((os.path.basename(p), rle_string(runs)))
    if a.rle:
        os.makedirs(os.path.dirname(os.path.abspath(a.rle)), exist_ok=True)
        with open(a.rle, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(("img", "rle_mask"))
            w.writerows(rows)
    dt = time.perf_counter() - t0
    print(f"predicted {len(files)} files in {dt:.2f} s: {len(files) / dt:.1f} img/s, {pred.host_finished} finished on "
          f"the host (backend {pred.strat.compute.name}, dtype {pred.dtype}, post-processing "
          f"{'host' if pred.host_post else 'device'})")
    return len(files), pred.host_finished


if __name__ == "__main__":
    main()
