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

:meth:`Predictor.score_files` compares those full-size masks with mask files, which is how the dataset is scored:
the mean over the images of the Dice coefficient at the source resolution.  The decode threads load the mask next
to the image; per group of equal source sizes one ``dpa_prob_score`` launch resizes, thresholds (up to 8
thresholds at once) and counts truth, predicted and common pixels in registers, so no mask exists on the device
and a few integers per image come back.  ``ops.kernels.score_reference`` (PIL + numpy) defines the counts and is
the host path.

``clean`` (``--clean``: ``largest``, ``fill`` or ``largest+fill``) cleans every mask between the threshold and the
run lengths: the largest 8-connected component, then the holes of what is kept filled.  ``dpa_mask_clean``
(csrc/mask_clean.hip) labels the full-size masks on the device, so still only run lists, three stats per image and
the requested masks come back; scoring then goes mask -> clean -> ``dpa_mask_score`` per threshold, since a cleaned
mask cannot be counted in registers straight from the probabilities.  ``ops.kernels.clean_reference`` (numpy) defines
the result and is the host path.  With ``none`` nothing of this runs.

``tta`` (``--tta``: ``hflip``, ``vflip``, ``hvflip`` joined by ``+``) and ``extra_models`` (``--ensemble``) average
the probabilities of the mirrored views and of several checkpoints before any of the above sees them
(:meth:`Predictor.merged_probs`): one forward of the batch per view and checkpoint, ``dpa_tta_views_f32`` (all views
from the resized bytes in one launch) in front and one ``dpa_tta_accum`` behind each (csrc/tta.hip).
``ops.kernels.tta_merge_reference`` (numpy) defines the average and is the host path.  Without either, nothing of
this runs.
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
    ``4 * source height``; a list that overflows it is finished on the host); ``clean`` is a ``--clean`` spec
    (``ops.kernels.parse_clean``): masks, run lists and scores are then those of the cleaned masks, and
    ``clean_stats`` sums (components before cleaning, pixels removed, pixels filled) over the files; ``tta`` is a
    ``--tta`` spec (``ops.kernels.parse_tta``) and ``extra_models`` further models of the same ``in_channels``
    (``ValueError`` otherwise): the probabilities are then the average over the views and the models."""

    def __init__(self, model, device, img_size, dtype: Optional[str] = None, backend: str = "auto",
                 threshold: float = 0.5, host_post: bool = False, rle_cap: Optional[int] = None,
                 clean: str = "none", tta: str = "none", extra_models: Sequence = ()):
        from .config import TrainConfig
        from .ops.kernels import parse_tta, tta_codes
        from .trainer import SingleDevice
        self.device = torch.device(device)
        self.on_gpu = self.device.type == "cuda"
        self.h, self.w = int(img_size[0]), int(img_size[-1])
        self.dtype = dtype or ("bf16" if self.on_gpu else "fp32")
        self.channels = int(model.cfg.in_channels)
        self.tta = parse_tta(tta)
        self.tta_codes = tta_codes(self.tta)
        extra_models = list(extra_models)
        for k, m in enumerate(extra_models):
            if int(m.cfg.in_channels) != self.channels:
                raise ValueError(f"extra_models[{k}] takes {int(m.cfg.in_channels)} input channels, the first model "
                                 f"{self.channels}")
        cfg = TrainConfig(backend=backend, img_size=(self.h, self.w), dtype=self.dtype)
        self.strat = SingleDevice(cfg, model, self.device)
        self.strat.set_train(False)
        self.strats = [self.strat]          # the ensemble, first member first
        for m in extra_models:
            self.strats.append(SingleDevice(cfg, m, self.device))
            self.strats[-1].set_train(False)
        self.threshold = float(threshold)
        self.host_post = bool(host_post) or not self.on_gpu
        self.rle_cap = None if rle_cap is None else int(rle_cap)
        assert self.rle_cap is None or self.rle_cap >= 1, "rle_cap must be positive"
        self.host_finished = 0          # files whose mask / run list the host path produced
        from .ops.kernels import parse_clean
        self.clean = parse_clean(clean)
        self.largest, self.fill = (n in self.clean.split("+") for n in ("largest", "fill"))
        # over the files finished: (components before cleaning, pixels removed, pixels filled); the files that lost
        # a component and the components they lost
        self.clean_stats = np.zeros(3, np.int64)
        self.clean_files = self.clean_removed = 0

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
    def _resize_raw(self, items):
        """The device resize of the full-size sources among ``items``: (uint8 ``[R, C, h, w]``, [(row, item)] of
        the items it resized), or (None, []) when there is none.  An item the kernel refuses becomes a CPU item."""
        raw = [i for i, (_, _, r) in enumerate(items) if r]
        if not raw:
            return None, []
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
        return u8, kept

    def _inputs(self, items, resized=None) -> torch.Tensor:
        """float32 ``[B, C, h, w]`` on the device: the training preprocessing of the decoded files.  ``resized``:
        what ``_resize_raw(items)`` returned, when the caller ran it already."""
        B = len(items)
        x = torch.empty(B, self.channels, self.h, self.w, dtype=torch.float32, device=self.device)
        u8, kept = self._resize_raw(items) if resized is None else resized
        if u8 is not None:
            from .ops import kernels as K
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

    @property
    def members(self) -> int:
        """Forward passes averaged per image: views x checkpoints."""
        return len(self.tta_codes) * len(self.strats)

    @torch.no_grad()
    def merged_probs(self, items) -> torch.Tensor:
        """float32 ``[B, h, w]`` probabilities of a decoded batch: the average over the mirrored views (``tta``) and
        the checkpoints (``extra_models``) as ``ops.kernels.tta_merge_reference`` defines it, members
        checkpoint-major; one forward of the B images per member, the views built once and shared by the
        checkpoints.  With one member this is ``probs(_inputs(items))`` and nothing else.  On a GPU
        ``dpa_tta_views_f32`` makes the views from the resized bytes and ``dpa_tta_accum`` adds each member up
        behind its forward; the host path (``host_post``, a CPU device) flips with torch and merges with numpy."""
        if self.members == 1:
            return self.probs(self._inputs(items))
        from .ops import kernels as K
        codes, B = self.tta_codes, len(items)
        views = None
        if not self.host_post:
            u8, kept = resized = self._resize_raw(items)
            if len(kept) == B:              # every file took the device resize: row j of u8 is item j
                views = K.tta_views(u8, codes)
        else:
            resized = None
        if views is None:
            x = self._inputs(items, resized)
            views = [x if c == 0 else torch.flip(x, [d for d, bit in ((3, 1), (2, 2)) if c & bit]) for c in codes]
        N = self.members
        scale = float(np.float32(1.0 / N))
        acc = None if self.host_post else torch.empty(B, self.h, self.w, dtype=torch.float32, device=self.device)
        got, k = [], 0
        for strat in self.strats:
            for v, c in enumerate(codes):
                p = strat.compute.probs(views[v])
                assert p.dim() == 4 and p.shape[1] == 1, f"probs: expected [B, 1, h, w], got {tuple(p.shape)}"
                if self.host_post:
                    got.append(p.to(torch.float32).reshape(B, self.h, self.w).cpu().numpy())
                else:
                    if p.dtype not in (torch.bfloat16, torch.float32):
                        p = p.to(torch.float32)
                    K.tta_accum(acc, p.contiguous(), c, k == 0, k == N - 1, scale)
                k += 1
        if self.host_post:
            return torch.from_numpy(K.tta_merge_reference(got, codes * len(self.strats))).to(self.device)
        return acc

    def _add_clean_stats(self, stats) -> None:
        stats = np.asarray(stats, np.int64).reshape(-1, 3)
        self.clean_stats += stats.sum(0)
        self.clean_files += int((stats[:, 1] > 0).sum())
        self.clean_removed += int(np.maximum(stats[:, 0] - 1, 0).sum())

    def _host_clean(self, m: np.ndarray, count: bool = True) -> np.ndarray:
        """``clean_reference`` by the predictor's spec; ``count``: add the stats to ``clean_stats``."""
        if self.clean == "none":
            return m
        from .ops.kernels import clean_reference
        m, stats = clean_reference(m, self.largest, self.fill, 255)
        if count:
            self._add_clean_stats(stats)
        return m

    def _host_finish(self, prob: np.ndarray, size, want_masks: bool, want_rle: bool):
        from .ops.kernels import rle_reference
        self.host_finished += 1
        m = self._host_clean(host_mask(prob, size, self.threshold))
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
            stats = None
            if self.clean != "none":
                cleaned = K.mask_clean(masks, self.largest, self.fill, 255)
                if cleaned is None:         # a size the clean launcher refuses: the host finishes these
                    todo += idx
                    continue
                masks, stats = cleaned
            runs = counts = None
            if want_rle:
                runs, counts = K.mask_rle(masks, self.rle_cap or 4 * Hs)
            launched.append((idx, masks, runs, counts, stats))
        if want_rle and launched:
            # two small downloads for the whole batch: the counts, then the used prefixes of the run lists
            counts = torch.cat([c for _, _, _, c, _ in launched]).cpu().numpy()
            parts, k = [], 0
            for idx, _, runs, _, _ in launched:
                for j in range(len(idx)):
                    n = int(counts[k + j])
                    if n <= runs.shape[1]:
                        parts.append(runs[j, :n])
                k += len(idx)
            flat = torch.cat(parts).cpu().numpy() if parts else np.zeros((0, 2), np.int32)
            k = pos = 0
            for idx, _, runs, _, _ in launched:
                for j, i in enumerate(idx):
                    n = int(counts[k + j])
                    if n <= runs.shape[1]:
                        out[i] = [None, flat[pos:pos + n].copy()]
                        pos += n
                    else:                   # overflow: nothing behind cap was written; the host encodes
                        todo.append(i)
                k += len(idx)
        if self.clean != "none" and launched:
            stats = torch.cat([s for _, _, _, _, s in launched]).cpu().numpy()
            keep = [i not in todo for idx, _, _, _, _ in launched for i in idx]     # the host counts its own
            self._add_clean_stats(stats[keep])
        for idx, masks, _, _, _ in launched:
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

    def score(self, probs: torch.Tensor, truths: Sequence, cuts: Sequence, thresholds: Sequence,
              count_host: bool = True) -> np.ndarray:
        """``probs`` float32 ``[B, h, w]`` against per image a truth array uint8 ``[Hs, Ws]`` (a pixel is truth
        where its byte ``> cuts[i]``) -> int64 ``[B, 1 + 2T]`` = (truth, pred_0, inter_0, ...) as
        ``ops.kernels.score_reference`` defines them.  On a GPU one ``dpa_prob_score`` launch per group of equal
        source sizes and one download of the counts; no mask is materialised.  ``count_host=False``: the files
        finished on the host are not added to ``host_finished`` (``post`` counted them already)."""
        from .ops import kernels as K
        B, T = probs.shape[0], len(thresholds)
        assert len(truths) == len(cuts) == B and 1 <= T <= K.SCORE_TMAX
        if self.clean != "none":
            return self._score_cleaned(probs, truths, cuts, thresholds, count_host)
        out = np.empty((B, 1 + 2 * T), np.int64)
        todo, launched = list(range(B)), []
        if not self.host_post:
            groups = {}
            for i, t in enumerate(truths):
                groups.setdefault(tuple(t.shape), []).append(i)
            todo = []
            for idx in groups.values():
                sel = probs if len(idx) == B else probs.index_select(0, torch.tensor(idx, device=probs.device))
                truth = torch.from_numpy(np.stack([truths[i] for i in idx])).to(probs.device, non_blocking=True)
                cut = torch.tensor([int(cuts[i]) for i in idx], dtype=torch.int32).to(probs.device, non_blocking=True)
                counts = K.prob_score(sel, truth, cut, thresholds)
                if counts is None:
                    todo += idx
                else:
                    launched.append((idx, counts))
            if launched:
                out[[i for idx, _ in launched for i in idx]] = torch.cat([c for _, c in launched]).cpu().numpy()
        if todo:
            todo = sorted(todo)
            host = (probs if len(todo) == B else
                    probs.index_select(0, torch.tensor(todo, device=probs.device))).cpu().numpy()
            for j, i in enumerate(todo):
                out[i] = K.score_reference(host[j], truths[i], int(cuts[i]), thresholds)
            if count_host:
                self.host_finished += len(todo)
        return out

    def _score_cleaned(self, probs, truths, cuts, thresholds, count_host: bool) -> np.ndarray:
        """``score`` of the CLEANED masks.  A cleaned mask cannot be counted in registers straight from the
        probabilities, so per group of equal source sizes and per threshold: ``dpa_prob_to_mask_u8`` ->
        ``dpa_mask_clean`` -> ``dpa_mask_score``; still only the counts come back.  The host path is ``host_mask``
        -> ``clean_reference`` -> numpy counts.  ``count_host`` (``post`` did not run on these files): the files the
        host finishes are counted, and ``clean_stats`` takes the stats of the first threshold."""
        from .ops import kernels as K
        B, T = probs.shape[0], len(thresholds)
        out = np.empty((B, 1 + 2 * T), np.int64)
        todo, launched = list(range(B)), []
        if not self.host_post:
            groups = {}
            for i, t in enumerate(truths):
                groups.setdefault(tuple(t.shape), []).append(i)
            todo = []
            for (Hs, Ws), idx in groups.items():
                sel = probs if len(idx) == B else probs.index_select(0, torch.tensor(idx, device=probs.device))
                truth = torch.from_numpy(np.stack([truths[i] for i in idx])).to(probs.device, non_blocking=True)
                cut = torch.tensor([int(cuts[i]) for i in idx], dtype=torch.int32).to(probs.device, non_blocking=True)
                masks = torch.empty(len(idx), Hs, Ws, dtype=torch.uint8, device=probs.device)
                per_t, stats0 = [], None
                for t, thr in enumerate(thresholds):
                    cleaned = K.mask_clean(masks, self.largest, self.fill, 255) \
                        if K.prob_to_mask_u8(sel, masks, float(thr), 255) else None
                    counts = None if cleaned is None else K.mask_score(cleaned[0], truth, cut)
                    if counts is None:      # refused for this size at the first threshold already
                        break
                    per_t.append(counts)
                    stats0 = cleaned[1] if t == 0 else stats0
                if len(per_t) < T:
                    todo += idx
                else:
                    launched.append((idx, torch.cat([per_t[0][:, :1]] + [c[:, 1:] for c in per_t], 1), stats0))
            if launched:
                out[[i for idx, _, _ in launched for i in idx]] = torch.cat([c for _, c, _ in launched]).cpu().numpy()
                if count_host:
                    self._add_clean_stats(torch.cat([s for _, _, s in launched]).cpu().numpy())
        if todo:
            todo = sorted(todo)
            host = (probs if len(todo) == B else
                    probs.index_select(0, torch.tensor(todo, device=probs.device))).cpu().numpy()
            for j, i in enumerate(todo):
                truth = np.asarray(truths[i]) > int(cuts[i])
                out[i, 0] = int(truth.sum())
                for t, thr in enumerate(thresholds):
                    m = self._host_clean(host_mask(host[j], truth.shape, float(thr)), count=count_host and t == 0) != 0
                    out[i, 1 + 2 * t], out[i, 2 + 2 * t] = int(m.sum()), int((m & truth).sum())
            if count_host:
                self.host_finished += len(todo)
        return out

    # ---- files --------------------------------------------------------------------------------------------
    def _decode_pair(self, pair):
        """``_decode`` of the image plus the truth of the mask file next to it: uint8 ``[Hs, Ws]`` and ``cut``."""
        size, arr, raw = self._decode(pair[0])
        truth, cut = load_truth(pair[1], size, pair[0])
        return size, arr, raw, truth, cut

    def _batches(self, jobs, decode, batch_size: int, workers: int) -> Iterator:
        """``(jobs of one batch, their decoded items)`` in input order, decoded by a bounded thread pool."""
        jobs = list(jobs)
        batch_size = max(1, int(batch_size))
        workers = max(1, min(16, int(workers) if workers else min(8, os.cpu_count() or 1)))
        pending = deque()
        with ThreadPoolExecutor(workers) as pool:
            nxt = 0
            for b0 in range(0, len(jobs), batch_size):
                chunk = jobs[b0:b0 + batch_size]
                items = []
                for _ in chunk:
                    while nxt < len(jobs) and len(pending) < max(2 * workers, batch_size):   # bounded: full-size sources
                        pending.append(pool.submit(decode, jobs[nxt]))
                        nxt += 1
                    items.append(pending.popleft().result())
                yield chunk, items

    def predict_files(self, paths, batch_size: int = 4, workers: int = 0, want_masks: bool = True,
                      want_rle: bool = True) -> Iterator:
        """Yields ``(path, (Hs, Ws), mask uint8 [Hs, Ws] or None, runs int32 [n, 2] or None)`` per file, in input
        order.  ``workers``: decode threads; 0 means ``min(8, os.cpu_count())``; never more than 16."""
        for chunk, items in self._batches(paths, self._decode, batch_size, workers):
            sizes = [s for s, _, _ in items]
            res = self.post(self.merged_probs(items), sizes, want_masks, want_rle)
            for p, s, (m, r) in zip(chunk, sizes, res):
                yield p, s, m, r

    def run_files(self, pairs, batch_size: int = 4, workers: int = 0, want_masks: bool = False,
                  want_rle: bool = False, thresholds: Optional[Sequence] = None) -> Iterator:
        """``predict_files`` and ``score_files`` from one forward pass: ``pairs`` of (image path, mask path) ->
        ``(image path, (Hs, Ws), mask or None, runs or None, counts int64 [1 + 2T])`` per pair, in input order."""
        thresholds = [self.threshold] if thresholds is None else [float(t) for t in thresholds]
        post = want_masks or want_rle
        for chunk, items in self._batches(pairs, self._decode_pair, batch_size, workers):
            sizes = [it[0] for it in items]
            probs = self.merged_probs([it[:3] for it in items])
            res = self.post(probs, sizes, want_masks, want_rle) if post else [(None, None)] * len(items)
            counts = self.score(probs, [it[3] for it in items], [it[4] for it in items], thresholds,
                                count_host=not post)
            for (p, _), s, (m, r), c in zip(chunk, sizes, res, counts):
                yield p, s, m, r, c

    def score_files(self, pairs, batch_size: int = 4, workers: int = 0,
                    thresholds: Optional[Sequence] = None) -> Iterator:
        """Yields ``(image path, (Hs, Ws), counts int64 [1 + 2T])`` per (image path, mask path) pair, in input
        order: what the Dice coefficient of the full-size mask against the mask file is made of
        (``ops.kernels.dice_iou``), for every threshold (default: the predictor's own)."""
        for p, s, _, _, c in self.run_files(pairs, batch_size, workers, thresholds=thresholds):
            yield p, s, c


def load_truth(mask_path, size, image_path=None):
    """The ground truth of one mask file at its own size, by the rule of ``BasicDataset.preprocess(mask,
    mask.size, is_mask=True)``: the first channel; ``> 127`` when the maximum exceeds 1, else non-zero.  Returns
    ``(uint8 [Hs, Ws], cut)`` with truth = ``array > cut``: a uint8 file as it is with ``cut`` 127 or 0, anything
    else normalised to 0/1 with ``cut`` 0.  ``size = (Hs, Ws)`` is the image's."""
    m = _load_image(Path(mask_path))
    if (m.size[1], m.size[0]) != tuple(size):
        raise ValueError(f"{image_path or mask_path}: the image is {size[1]}x{size[0]}, its mask {mask_path} "
                         f"{m.size[0]}x{m.size[1]}")
    a = np.asarray(m)
    if a.ndim == 3:
        a = a[..., 0]
    big = bool(a.max(initial=0) > 1)
    if a.dtype != np.uint8:
        return ((a > 127) if big else (a > 0)).astype(np.uint8), 0
    return np.ascontiguousarray(a), (127 if big else 0)


def match_masks(files, masks_dir, suffix: str = "_mask") -> list:
    """``(image, mask)`` per image file: the one file in ``masks_dir`` whose stem is the image's stem + ``suffix``.
    Raises ``ValueError`` naming the stem when there is none or more than one."""
    by_stem = {}
    for f in sorted(os.listdir(masks_dir)):
        if not f.startswith(".") and os.path.isfile(os.path.join(masks_dir, f)):
            by_stem.setdefault(os.path.splitext(f)[0], []).append(os.path.join(masks_dir, f))
    pairs = []
    for p in files:
        stem = Path(p).stem
        m = by_stem.get(stem + suffix, [])
        if len(m) != 1:
            raise ValueError(f"{'no mask' if not m else 'several masks'} for {stem} in {masks_dir} "
                             f"(looked for {stem + suffix}.*){': ' + ', '.join(m) if m else ''}")
        pairs.append((p, m[0]))
    return pairs


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


def _clean_spec(text: str) -> str:
    """``--clean``: the canonical spec string (``fill+largest`` -> ``largest+fill``)."""
    from .ops.kernels import parse_clean
    try:
        return parse_clean(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def _tta_spec(text: str) -> str:
    """``--tta``: the canonical spec string (``vflip+hflip`` -> ``hflip+vflip``)."""
    from .ops.kernels import parse_tta
    try:
        return parse_tta(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def ensemble_path(entry: str, out_dir: str) -> str:
    """``--ensemble``: an entry without a path separator and without a ``.pth`` ending names
    ``<out_dir>/checkpoints/<entry>.pth``; anything else is a path."""
    if os.sep in entry or (os.altsep and os.altsep in entry) or entry.endswith(".pth"):
        return entry
    return os.path.join(out_dir, "checkpoints", f"{entry}.pth")


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
    ap.add_argument("--clean", type=_clean_spec, default="none", metavar="SPEC",
                    help="clean every mask after the threshold: none, or largest (keep the largest 8-connected "
                         "component) and fill (fill enclosed holes) joined by +; masks, run lists and scores are "
                         "those of the cleaned masks")
    ap.add_argument("--tta", type=_tta_spec, default="none", metavar="SPEC",
                    help="average the probabilities over mirrored views: none, or hflip, vflip and hvflip joined by "
                         "+ (the image itself always counts); one forward per view")
    ap.add_argument("--ensemble", nargs="+", default=[], metavar="CKPT",
                    help="further checkpoints of the same --model whose probabilities are averaged with the first "
                         "(-c / -l): NAME means <out-dir>/checkpoints/NAME.pth, anything with a path separator or "
                         "ending in .pth is a path")
    ap.add_argument("--out-dir", default=".", help="where checkpoints/ lives")
    ap.add_argument("--model", default="unet")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"])
    ap.add_argument("--dtype", default=None, choices=["bf16", "fp32"],
                    help="compute dtype (default bf16 on a GPU, fp32 on CPU; on a GPU fp32 runs the fp32 HIP engine)")
    ap.add_argument("--score", default=None, metavar="MASKS_DIR",
                    help="score the full-size masks against MASKS_DIR/<stem><suffix>.*: mean per-image Dice and IoU")
    ap.add_argument("--mask-suffix", default="_mask", help="what a mask's stem adds to its image's")
    ap.add_argument("--score-thresholds", type=float, nargs="+", default=None, metavar="T",
                    help="score at these thresholds, at most 8 (default: --threshold)")
    ap.add_argument("--score-csv", default=None, metavar="FILE",
                    help="write img,height,width,threshold,truth,pred,inter,dice,iou per image and threshold")
    a = ap.parse_args(argv)
    if not a.output and not a.rle and not a.score:
        ap.error("nothing to write: give --output DIR and / or --rle FILE.csv (or --score MASKS_DIR)")
    if (a.score_thresholds or a.score_csv) and not a.score:
        ap.error("--score-thresholds and --score-csv need --score MASKS_DIR")
    thresholds = a.score_thresholds or [a.threshold]
    if len(thresholds) > 8:
        ap.error(f"--score-thresholds takes at most 8 values, got {len(thresholds)}")
    path = a.load or (os.path.join(a.out_dir, "checkpoints", f"{a.checkpoint}.pth") if a.checkpoint else None)
    if not path:
        ap.error("no checkpoint: give -c NAME or -l PATH")
    if not os.path.isfile(path):
        ap.error(f"checkpoint not found: {path}")
    more = [ensemble_path(e, a.out_dir) for e in a.ensemble]
    for p in more:
        if not os.path.isfile(p):
            ap.error(f"--ensemble: checkpoint not found: {p}")
    files = list_inputs(a.input)
    if not files:
        ap.error(f"no input file found in {' '.join(a.input)}")
    missing = [f for f in files if not os.path.isfile(f)]
    if missing:
        ap.error(f"input file not found: {missing[0]}")
    pairs = None
    if a.score:
        if not os.path.isdir(a.score):
            ap.error(f"--score: no such directory: {a.score}")
        try:
            pairs = match_masks(files, a.score, a.mask_suffix)
        except ValueError as e:
            ap.error(str(e))

    model = build_model(a.model)
    load_model_state(model, path)
    extra = []
    for p in more:
        extra.append(build_model(a.model))
        load_model_state(extra[-1], p)
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    pred = Predictor(model, dev, (a.img_size[0], a.img_size[-1]), dtype=a.dtype, backend=a.backend,
                     threshold=a.threshold, host_post=a.host_post, clean=a.clean, tta=a.tta, extra_models=extra)
    if a.output:
        os.makedirs(a.output, exist_ok=True)
    rows, scored = [], []
    t0 = time.perf_counter()
    if pairs is None:
        results = ((p, s, m, r, None) for p, s, m, r in
                   pred.predict_files(files, a.batch_size, a.num_workers, want_masks=bool(a.output), want_rle=bool(a.rle)))
    else:
        results = pred.run_files(pairs, a.batch_size, a.num_workers, want_masks=bool(a.output), want_rle=bool(a.rle),
                                 thresholds=thresholds)
    for p, size, mask, runs, counts in results:
        if counts is not None:
            scored.append((os.path.basename(p), size, counts))
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
    if pred.members > 1:
        print(f"merged (tta {pred.tta}): {len(pred.tta_codes)} views x {len(pred.strats)} checkpoints")
    if pred.clean != "none":
        print(f"cleaned ({pred.clean}): {pred.clean_removed} components removed "
              f"from {pred.clean_files} files, {int(pred.clean_stats[2])} pixels filled")
    if pairs is None:
        return len(files), pred.host_finished
    return len(files), pred.host_finished, report_scores(scored, thresholds, a.score_csv)


def report_scores(scored, thresholds, csv_path=None):
    """``scored``: ``(name, (Hs, Ws), counts int64 [1 + 2T])`` per image.  Prints per threshold the mean over the
    images of the per-image Dice coefficient and IoU (the Carvana score is the Dice column) and marks the
    threshold with the best mean Dice; writes one CSV row per (image, threshold) when asked.  Returns
    ``(mean dice [T], mean iou [T])``."""
    from .ops.kernels import dice_iou
    dice, iou = dice_iou(np.stack([c for _, _, c in scored]))                 # [N, T]
    if csv_path:
        os.makedirs(os.path.dirname(os.path.abspath(csv_path)), exist_ok=True)
        with open(csv_path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(("img", "height", "width", "threshold", "truth", "pred", "inter", "dice", "iou"))
            for i, (name, (Hs, Ws), c) in enumerate(scored):
                for t, thr in enumerate(thresholds):
                    w.writerow((name, Hs, Ws, repr(float(thr)), int(c[0]), int(c[1 + 2 * t]), int(c[2 + 2 * t]),
                                repr(float(dice[i, t])), repr(float(iou[i, t]))))
    md, mi = dice.mean(0), iou.mean(0)
    best = int(np.argmax(md))
    for t, thr in enumerate(thresholds):
        print(f"score threshold {float(thr):g}: dice {md[t]:.6f} iou {mi[t]:.6f} ({len(scored)} images)"
              f"{'  <- best' if t == best and len(thresholds) > 1 else ''}")
    return md, mi


if __name__ == "__main__":
    main()
