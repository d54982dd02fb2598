"""HBM-resident folder dataset: every file decoded once, resized once on the GPU, batches gathered there.

:class:`.folder.CarvanaDataset` decodes and bicubic-resizes every image on the CPU, every epoch, inside the
``DataLoader`` (the reference's ``utils/dataloading.py:54-73``); a training step consumes images two orders of
magnitude faster than one core produces them.  The resized Carvana set is 3.9 GB as uint8 at 640x960 and a
GPU has 288 GB, so (opt-in, ``--device-folder-data``):

* :class:`DeviceFolderDataset` - ``BasicDataset``'s pairing and errors; each file is decoded ONCE by a thread
  pool (PIL: there is no GPU JPEG decoder here), uploaded, resized by ``csrc/data_prep.hip`` -- PIL's BICUBIC for
  the image and NEAREST + the 0/255 -> 0/1 rule for the mask, both bit-equal to PIL -- and stored as uint8
  (``images [N,C,H,W]``, ``masks [N,H,W]``).  Files the kernels do not cover (image modes other than L / RGB,
  mask modes other than L / P, a down-scaling so extreme that the launcher refuses it) go through
  ``BasicDataset.preprocess`` on the CPU and are uploaded.  Items are equal to ``CarvanaDataset``'s.  On a CPU
  device the same class holds the PIL results, so it and its loader run without a GPU.
* :class:`DeviceFolderLoader` / :func:`device_folder_loaders` - the samplers and batches of
  ``device.device_loaders`` (epoch-seeded shuffle, ``DistributedSampler``, ``random_split`` subsets); a batch is
  ONE launch of ``dpa_batch_gather_u8``: gather by index, optional horizontal flip, uint8 -> float32
  ``(images [B,C,H,W], targets [B,1,H,W])``, bit-equal to the host path's ``arr / 255.0``.
* ``augment="hflip"`` (training loader): item ``i`` of epoch ``e`` is mirrored, image and mask together, when
  :func:`flip_flags` -- a fixed integer hash of ``(seed, e, base index i)`` -- is odd: a pure function, so a
  resumed run replays it and every pipeline stage agrees.
* ``augment`` with ``affine`` or ``color`` (:class:`.augment.AugmentSpec`: names from ``hflip``, ``affine``,
  ``color`` joined by ``+``, canonically in that order): the batch is ONE launch of ``dpa_batch_augment_u8``
  (csrc/augment.hip) instead -- per item an inverse affine map (random zoom, rotation, shift and the mirror;
  bilinear for the image, nearest for the mask, clamp-to-edge) and a 256-entry tone table (brightness, contrast,
  gamma), both built on the host per batch from hashes of ``(seed, e, i, stream)`` and uploaded (B x 6 int32 and
  B x 256 float32).  Integer arithmetic, specified in ``augment.py``: the kernel, the CPU path
  (``augment_reference``) and the tests agree bit for bit.

With DDP or ``-t MP`` every rank loads the FULL resized set: the shards change per epoch and the stages of a
pipeline pair their batches by order.  Sharding the load is out of scope here.
"""
from __future__ import annotations

import logging
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, Optional

import numpy as np
import torch
from torch.utils.data import BatchSampler, Subset

from .augment import AugmentSpec, affine_matrices, augment_reference, color_luts
from .folder import BasicDataset, _load_image

log = logging.getLogger(__name__)

_IMAGE_MODES = ("L", "RGB")       # what dpa_resize_bicubic_u8 covers: 8-bit, 1 or 3 interleaved channels
_MASK_MODES = ("L", "P")          # single-channel 8-bit: grey levels or palette indices (GIF)


def flip_flags(seed: int, epoch: int, base_idx) -> np.ndarray:
    """uint8 ``[n]``: 1 where item ``base_idx[k]`` is mirrored in ``epoch`` -- the low bit of a 32-bit integer
    hash (lowbias32) of ``(seed, epoch, index)``.  Fixed: changing it changes every augmented run."""
    x = np.asarray(base_idx, dtype=np.int64).astype(np.uint64)
    x = (x * np.uint64(0x9E3779B1) + np.uint64(int(epoch) & 0xFFFFFFFF) * np.uint64(0x85EBCA6B)
         + np.uint64(int(seed) & 0xFFFFFFFF) * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return (x & np.uint64(1)).astype(np.uint8)


def _unit_table(device) -> torch.Tensor:
    from ..ops.kernels import unit_table
    return unit_table(device)


class DeviceFolderDataset(BasicDataset):
    """The folder dataset, resized once and resident on ``device`` (see the module docstring).

    ``workers``: decode threads; 0 means ``min(8, os.cpu_count())``; never more than 16."""

    def __init__(self, images_dir, masks_dir, newsize=(960, 640), mask_suffix: str = "", device="cuda",
                 workers: int = 0):
        super().__init__(images_dir, masks_dir, newsize, mask_suffix)
        self.device = torch.device(device)
        self.w, self.h = self.newsize
        self.workers = max(1, min(16, int(workers) if workers else min(8, os.cpu_count() or 1)))
        self.on_gpu = self.device.type == "cuda"
        first = _load_image(self._pairs[0][0])
        self.channels = len(first.getbands())
        n = len(self.ids)
        log.info("loading %d folder images as %dx%d into %s: %.2f GiB (uint8 images + masks), %d decode threads",
                 n, self.h, self.w, self.device, n * (self.channels + 1) * self.h * self.w / 2 ** 30, self.workers)
        self.images = torch.empty(n, self.channels, self.h, self.w, dtype=torch.uint8, device=self.device)
        self.masks = torch.empty(n, self.h, self.w, dtype=torch.uint8, device=self.device)
        self.cpu_resized = 0            # files (image or mask) that took the CPU path
        self._scratch = torch.empty(1, dtype=torch.int32, device=self.device) if self.on_gpu else None
        pending = deque()
        with ThreadPoolExecutor(self.workers) as pool:
            nxt = 0
            for i in range(n):
                while nxt < n and len(pending) < 2 * self.workers:      # bounded: sources are full-size
                    pending.append(pool.submit(self._decode, nxt))
                    nxt += 1
                self._store(i, *pending.popleft().result())

    # ---- decode (worker threads) ------------------------------------------------------------------------
    def _cpu_image(self, pil_img, path) -> np.ndarray:
        """``BasicDataset.preprocess`` on the CPU, back as the uint8 ``[C,h,w]`` it divided by 255."""
        x = self.preprocess(pil_img, self.newsize, is_mask=False)
        u8 = np.rint(x * 255.0)
        if not (u8.min(initial=0) >= 0 and u8.max(initial=0) <= 255 and np.array_equal(u8 / 255.0, x)):
            raise ValueError(f"{path}: not an 8-bit image (mode {pil_img.mode}); the resident dataset stores uint8")
        return u8.astype(np.uint8)

    def _cpu_mask(self, pil_img, path) -> np.ndarray:
        m = np.asarray(self.preprocess(pil_img, self.newsize, is_mask=True))
        if m.dtype == np.bool_:
            m = m.astype(np.uint8)
        if not (np.issubdtype(m.dtype, np.integer) and m.min(initial=0) >= 0 and m.max(initial=0) <= 255):
            raise ValueError(f"{path}: not an 8-bit mask (mode {pil_img.mode}); the resident dataset stores uint8")
        return m.astype(np.uint8)

    def _decode(self, idx):
        """(image, mask): a full-size uint8 source array for the kernels (``ndim`` 3 / source-shaped), or the
        resized uint8 result of the CPU path -- told apart by the second element of each pair."""
        img_path, mask_path = self._pairs[idx]
        img = _load_image(img_path)
        mask = _load_image(mask_path)
        assert img.size == mask.size, \
            f"Image and mask {self.ids[idx]} should be the same size, but are {img.size} and {mask.size}"
        if self.on_gpu and img.mode in _IMAGE_MODES:
            a = np.array(img)
            image = (a if a.ndim == 3 else a[:, :, None], True)
        else:
            image = (self._cpu_image(img, img_path), False)
        if self.on_gpu and mask.mode in _MASK_MODES:
            mk = (np.array(mask), True)
        else:
            mk = (self._cpu_mask(mask, mask_path), False)
        return image, mk

    # ---- upload + resize (constructing thread) ----------------------------------------------------------
    def _store(self, i, image, mask):
        from ..ops import kernels as K
        img_path, mask_path = self._pairs[i]
        arr, raw = image
        if raw:
            if arr.shape[2] != self.channels:
                raise ValueError(f"{img_path}: {arr.shape[2]} channels, the dataset's first image has {self.channels}")
            src = torch.from_numpy(arr).to(self.device)
            if not K.resize_bicubic_u8(src, self.images[i]):
                from PIL import Image
                arr = self._cpu_image(Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr), img_path)
                raw = False
        if not raw:
            if arr.shape[0] != self.channels:
                raise ValueError(f"{img_path}: {arr.shape[0]} channels, the dataset's first image has {self.channels}")
            self.images[i].copy_(torch.from_numpy(arr))
            self.cpu_resized += 1
        arr, raw = mask
        if raw:
            K.resize_nearest_u8(torch.from_numpy(arr).to(self.device), self.masks[i], mask_rule=True,
                                scratch=self._scratch)
        else:
            self.masks[i].copy_(torch.from_numpy(arr))
            self.cpu_resized += 1

    # ---- dataset interface ------------------------------------------------------------------------------
    @property
    def nbytes(self) -> int:
        return self.images.numel() + self.masks.numel()

    def to_float(self, img_u8: torch.Tensor) -> torch.Tensor:
        """uint8 -> float32, bit-equal to the host path's ``arr / 255.0`` (float64) cast to float32."""
        return _unit_table(self.device)[img_u8.long()]

    def __getitem__(self, idx):
        return {"image": self.to_float(self.images[idx]), "mask": self.masks[idx].long()}


def _base(ds):
    """(resident dataset, index map) through nested ``Subset`` wrappers (``random_split``)."""
    idx = None
    while isinstance(ds, Subset):
        sub = torch.as_tensor(ds.indices, dtype=torch.int64)
        idx = sub if idx is None else sub[idx]
        ds = ds.dataset
    assert isinstance(ds, DeviceFolderDataset), type(ds)
    return ds, idx


class DeviceFolderLoader:
    """Batches assembled on the device; yields ``(images, targets)`` like ``loaders.DeviceBatcher``.

    ``augment="hflip"`` mirrors the items :func:`flip_flags` selects for the sampler's current epoch
    (``set_epoch``); ``last_flags`` holds the flags of the batch yielded last (None without ``hflip``).
    ``augment`` is a spec string or an :class:`.augment.AugmentSpec` (which carries the magnitudes); with
    ``affine`` or ``color`` in it every batch is warped and toned by ``dpa_batch_augment_u8``, and ``last_params``
    holds the host ``(mats int32 [B,6], luts float32 [B,256] or None)`` of the batch yielded last."""

    def __init__(self, dataset, batch_size: int, sampler=None, drop_last: bool = False, augment="none",
                 seed: int = 0):
        self.spec = AugmentSpec.parse(augment)                  # ValueError names the valid ones
        augment = self.spec.name
        self.base, idx = _base(dataset)
        self.n = len(dataset)
        self.index_map = idx                                   # host: the flip hash is on base indices
        self.sampler = sampler if sampler is not None else range(self.n)
        self.batches = BatchSampler(self.sampler, batch_size, drop_last)
        self.augment, self.seed = augment, int(seed)
        self.last_flags: Optional[np.ndarray] = None
        self.last_params = None

    def __len__(self):
        return len(self.batches)

    def __iter__(self) -> Iterator:
        base, dev = self.base, self.base.device
        epoch = int(getattr(self.sampler, "epoch", 0))
        for b in self.batches:
            i = torch.as_tensor(b, dtype=torch.int64)
            if self.index_map is not None:
                i = self.index_map.index_select(0, i)
            assert int(i.min()) >= 0 and int(i.max()) < len(base), "sampler index outside the dataset"
            flags = flip_flags(self.seed, epoch, i.numpy()) if self.spec.hflip else None
            self.last_flags = flags
            if self.spec.warps:
                luts = color_luts(self.spec, self.seed, epoch, i.numpy())
                mats = torch.from_numpy(affine_matrices(self.spec, self.seed, epoch, i.numpy(), base.h, base.w))
                luts = None if luts is None else torch.from_numpy(luts)
                self.last_params = (mats, luts)
                if base.on_gpu:
                    from ..ops import kernels as K
                    yield K.batch_augment_u8(base.images, base.masks, i.to(dev, non_blocking=True),
                                             mats.to(dev, non_blocking=True),
                                             None if luts is None else luts.to(dev, non_blocking=True))
                else:
                    yield augment_reference(base.images, base.masks, i, mats, luts)
                continue
            if base.on_gpu:
                from ..ops import kernels as K
                f = None if flags is None else torch.from_numpy(flags).to(dev, non_blocking=True)
                yield K.batch_gather_u8(base.images, base.masks, i.to(dev, non_blocking=True), f)
                continue
            img = base.to_float(base.images.index_select(0, i))
            tgt = base.masks.index_select(0, i).to(torch.float32).unsqueeze(1)
            if flags is not None:
                f = torch.from_numpy(flags).bool().view(-1, 1, 1, 1)
                img = torch.where(f, img.flip(-1), img)
                tgt = torch.where(f, tgt.flip(-1), tgt)
            yield img, tgt


def device_folder_loaders(train_set, val_set, batch_size: int, *, rank: int = 0, world_size: int = 1, seed: int = 0,
                          drop_last: bool = False, augment="none"):
    """``loaders.build_loaders`` for a resident folder dataset (same samplers, same batches); ``augment`` (a
    spec string or an ``AugmentSpec``) applies to the training loader only."""
    from torch.utils.data.distributed import DistributedSampler
    from .loaders import EpochShuffleSampler
    val_sampler: Optional[object] = None
    if world_size > 1:
        train_sampler = DistributedSampler(train_set, num_replicas=world_size, rank=rank, shuffle=True, seed=seed,
                                           drop_last=drop_last)
        if len(val_set) >= world_size:
            val_sampler = DistributedSampler(val_set, num_replicas=world_size, rank=rank, shuffle=False,
                                             drop_last=True)
    else:
        train_sampler = EpochShuffleSampler(len(train_set), seed)
    return (DeviceFolderLoader(train_set, batch_size, train_sampler, drop_last, augment=augment, seed=seed),
            DeviceFolderLoader(val_set, batch_size, val_sampler, False), train_sampler)
