"""Training augmentation of the resident folder dataset: what to draw, and the arithmetic that applies it.

``--augment`` names a subset of ``hflip``, ``affine`` and ``color`` joined by ``+`` (:class:`AugmentSpec`):

* ``affine``: a random zoom, rotation and shift, applied jointly to image (bilinear) and mask (nearest);
* ``color``: brightness, contrast and gamma on the image, one 256-entry table per item shared by its channels
  (no hue shift);
* ``hflip``: the mirror :func:`.device_folder.flip_flags` decides, unchanged; alone it keeps the plain batch
  kernel, with ``affine`` or ``color`` it is folded into the item's matrix.

Every draw is a pure integer hash of ``(seed, epoch, base index, stream)`` (:func:`aug_uniform`), like
``flip_flags``: a resumed run replays it, and every pipeline stage or DDP rank that assembles an item gets the
same pixels.  An item's table is ``float32(clip((k/255 - 0.5) contrast + 0.5 + brightness, 0, 1) ** gamma)`` in
float64, with one exception: where contrast is exactly 1 and brightness exactly 0 the line is ``k/255`` itself,
not ``(k/255 - 0.5) + 0.5``, which differs from it in the last bit for some ``k``; so zero magnitudes give
``unit_table`` exactly.  A draw hits that case only when both magnitudes are 0.  The host builds, per batch, ``mats`` int32 ``[B, 6]`` (the inverse affine map in Q16) and ``luts``
float32 ``[B, 256]``; ``dpa_batch_augment_u8`` (csrc/augment.hip) applies them while it writes the batch.

The arithmetic is integer and fully specified, so the kernel, the CPU path and the tests agree bit for bit.  For
output pixel ``(x, y)`` of item ``b`` with ``M = mats[b]``, in int64::

    sx = M0*x + M1*y + M2          sy = M3*x + M4*y + M5       (Q16 source pixel-index coordinates)
    x0 = sx >> 16   fx = (sx & 0xFFFF) >> 8     y0 = sy >> 16   fy = (sy & 0xFFFF) >> 8
    p00, p01, p10, p11 = image taps at (y0 | y0+1, x0 | x0+1), each index clamped to its axis
    v  = ((256-fx)*(256-fy)*p00 + fx*(256-fy)*p01 + (256-fx)*fy*p10 + fx*fy*p11 + 32768) >> 16
    img[b, c, y, x] = lut_b[v]
    tgt[b, 0, y, x] = float(masks[n, clamp((sy+32768) >> 16), clamp((sx+32768) >> 16)])

Clamp-to-edge for image and mask alike, so the two stay consistent at the rim.  The identity matrix without a
table reproduces the plain batch, ``[-65536, 0, (W-1) << 16, 0, 65536, 0]`` the ``hflip`` batch, and an integer
shift a clamped index shift, all exactly.  :func:`augment_reference` is these lines in torch.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

NAMES = ("hflip", "affine", "color")                 # canonical order
AFFINE_MAGNITUDES = ("scale", "rotate", "shift")
COLOR_MAGNITUDES = ("brightness", "contrast", "gamma")
MAGNITUDES = AFFINE_MAGNITUDES + COLOR_MAGNITUDES
# hash streams of aug_uniform; 0 is flip_flags' own input.  The shift draws one number per axis.
STREAM_SCALE, STREAM_ROTATE, STREAM_SHIFT_X, STREAM_SHIFT_Y, STREAM_BRIGHTNESS, STREAM_CONTRAST, STREAM_GAMMA = range(1, 8)
Q = 1 << 16


@dataclass(frozen=True)
class AugmentSpec:
    """Which augmentations run, and how strong they are.

    ``scale``: zoom log-uniform in ``[1/(1+s), 1+s]``; ``rotate``: degrees, uniform in +-r; ``shift``: fraction of
    W and of H, uniform in +-f; ``brightness``: additive in the unit range, uniform in +-b; ``contrast``: factor
    about 0.5, uniform in ``[1-c, 1+c]``; ``gamma``: exponent log-uniform in ``[1/(1+g), 1+g]``."""
    hflip: bool = False
    affine: bool = False
    color: bool = False
    scale: float = 0.25
    rotate: float = 10.0
    shift: float = 0.10
    brightness: float = 0.2
    contrast: float = 0.2
    gamma: float = 0.2

    @classmethod
    def parse(cls, text, **magnitudes) -> "AugmentSpec":
        """From ``none`` or names joined by ``+`` in any order; ``magnitudes`` that are None keep their default."""
        if isinstance(text, cls):
            return text
        names = [t.strip() for t in str(text).split("+")]
        if names == ["none"]:
            names = []
        bad = [t for t in names if t not in NAMES]
        if bad:
            raise ValueError(f"unknown augment {text!r}: use none, or names from hflip, affine and color joined "
                             f"by + (each once)")
        twice = sorted({t for t in names if names.count(t) > 1}, key=NAMES.index)
        if twice:
            raise ValueError(f"augment {text!r} names {' and '.join(twice)} more than once: use none, or names from "
                             f"hflip, affine and color joined by +, each once")
        given = {k: float(v) for k, v in magnitudes.items() if v is not None}
        for k, v in given.items():
            if k not in MAGNITUDES:
                raise ValueError(f"unknown augment magnitude {k!r}; choose from {MAGNITUDES}")
            if not (v >= 0.0 and np.isfinite(v)):
                raise ValueError(f"augment magnitude {k}={v} must be finite and not negative")
        return cls(**{n: n in names for n in NAMES}, **given)

    @property
    def name(self) -> str:
        """The canonical spec string: ``none`` or the names in the order hflip+affine+color."""
        return "+".join(n for n in NAMES if getattr(self, n)) or "none"

    @property
    def warps(self) -> bool:
        """True when batches need ``dpa_batch_augment_u8``; ``none`` and ``hflip`` keep the plain gather."""
        return self.affine or self.color

    def describe(self) -> str:
        mags = [m for m in MAGNITUDES if getattr(self, "affine" if m in AFFINE_MAGNITUDES else "color")]
        return " ".join([self.name] + [f"{m}={getattr(self, m):g}" for m in mags])

    def __str__(self) -> str:
        return self.name


def canonical(text) -> str:
    return AugmentSpec.parse(text).name


def aug_uniform(seed: int, epoch: int, base_idx, stream: int) -> np.ndarray:
    """float64 ``[n]`` in ``[0, 1)``: the top 24 bits of the lowbias32 hash of ``flip_flags``' input plus
    ``stream * 0x27D4EB2F``.  Stream 0 is ``flip_flags``' own input and is never drawn here; the augmentations
    use seven streams, one per drawn number: 1 scale, 2 rotate, 3 shift along x, 4 shift along y (the shift needs
    a number per axis), 5 brightness, 6 contrast, 7 gamma (the ``STREAM_*`` constants).  The hash and this
    numbering are frozen: changing either changes every augmented run."""
    x = np.asarray(base_idx, dtype=np.int64).astype(np.uint64)
    x = (x * np.uint64(0x9E3779B1) + np.uint64(int(epoch) & 0xFFFFFFFF) * np.uint64(0x85EBCA6B)
         + np.uint64(int(seed) & 0xFFFFFFFF) * np.uint64(0xC2B2AE35)
         + np.uint64(int(stream) & 0xFFFFFFFF) * np.uint64(0x27D4EB2F)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return (x >> np.uint64(8)).astype(np.float64) / float(1 << 24)


def _signed(seed, epoch, base_idx, stream) -> np.ndarray:
    return 2.0 * aug_uniform(seed, epoch, base_idx, stream) - 1.0


def affine_matrices(spec: AugmentSpec, seed: int, epoch: int, base_idx, H: int, W: int) -> np.ndarray:
    """int32 ``[n, 6]``: per item the inverse of ``dst = c + s R(theta) F (src - c) + t`` (F the mirror
    ``flip_flags`` selects, c the image centre), about pixel centres: ``src_idx = A (dst_idx + 0.5 - c) + c - A t -
    0.5`` with ``A = F R(-theta) / s``, built in float64, times 65536, rounded to nearest.  Without ``affine``
    the zoom is 1 and angle and shift are 0: the identity or the flip matrix, exactly."""
    from .device_folder import flip_flags
    base_idx = np.asarray(base_idx, dtype=np.int64)
    n = base_idx.shape[0]
    if spec.affine:
        s = np.exp(_signed(seed, epoch, base_idx, STREAM_SCALE) * np.log1p(spec.scale))
        th = np.deg2rad(_signed(seed, epoch, base_idx, STREAM_ROTATE) * spec.rotate)
        tx = _signed(seed, epoch, base_idx, STREAM_SHIFT_X) * spec.shift * W
        ty = _signed(seed, epoch, base_idx, STREAM_SHIFT_Y) * spec.shift * H
    else:
        s, th, tx, ty = np.ones(n), np.zeros(n), np.zeros(n), np.zeros(n)
    f = np.where(flip_flags(seed, epoch, base_idx) != 0, -1.0, 1.0) if spec.hflip else np.ones(n)
    return to_q16(inverse_affine(s, th, tx, ty, f, H, W))


def inverse_affine(s, th, tx, ty, f, H: int, W: int) -> np.ndarray:
    """float64 ``[n, 6]``: output pixel index -> source pixel index for zoom ``s``, angle ``th`` (radians), shift
    ``(tx, ty)`` in pixels and mirror sign ``f`` (-1 mirrored, 1 not), arrays of one length; see
    :func:`affine_matrices`."""
    s, th, tx, ty, f = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (s, th, tx, ty, f))
    n = s.shape[0]
    cos, sin = np.cos(th) / s, np.sin(th) / s
    # A = F R(-theta) / s with R(theta) = [[cos, -sin], [sin, cos]] and F = diag(f, 1)
    a00, a01, a10, a11 = f * cos, f * sin, -sin, cos
    cx, cy = W / 2.0, H / 2.0
    m = np.empty((n, 6), np.float64)
    m[:, 0], m[:, 1] = a00, a01
    m[:, 2] = a00 * (0.5 - cx) + a01 * (0.5 - cy) + cx - (a00 * tx + a01 * ty) - 0.5
    m[:, 3], m[:, 4] = a10, a11
    m[:, 5] = a10 * (0.5 - cx) + a11 * (0.5 - cy) + cy - (a10 * tx + a11 * ty) - 0.5
    return m


def to_q16(m: np.ndarray) -> np.ndarray:
    """float64 matrices -> int32 Q16, rounded to nearest (saturating)."""
    lim = np.iinfo(np.int32)
    return np.clip(np.rint(np.asarray(m, dtype=np.float64) * Q), lim.min, lim.max).astype(np.int32)


def color_luts(spec: AugmentSpec, seed: int, epoch: int, base_idx) -> Optional[np.ndarray]:
    """float32 ``[n, 256]``: ``clip((k/255 - 0.5) contrast + 0.5 + brightness, 0, 1) ** gamma`` per item, in
    float64, then float32; None without ``color`` (nothing to upload).  The one exception to the formula: an item
    whose contrast is exactly 1 and whose brightness is exactly 0 takes ``k/255`` itself as the clipped line, so
    that zero magnitudes give ``unit_table`` bit for bit (see the module docstring)."""
    if not spec.color:
        return None
    base_idx = np.asarray(base_idx, dtype=np.int64)
    br = (_signed(seed, epoch, base_idx, STREAM_BRIGHTNESS) * spec.brightness)[:, None]
    ct = (1.0 + _signed(seed, epoch, base_idx, STREAM_CONTRAST) * spec.contrast)[:, None]
    gm = np.exp(_signed(seed, epoch, base_idx, STREAM_GAMMA) * np.log1p(spec.gamma))[:, None]
    k = (np.arange(256, dtype=np.float64) / 255.0)[None, :]
    # an untouched line stays k / 255 to the bit ((k/255 - 0.5) + 0.5 rounds below 0.25)
    lin = np.where((ct == 1.0) & (br == 0.0), k, (k - 0.5) * ct + 0.5 + br)
    return (np.clip(lin, 0.0, 1.0) ** gm).astype(np.float32)


def augment_reference(images: torch.Tensor, masks: torch.Tensor, idx: torch.Tensor, mats: torch.Tensor,
                      luts: Optional[torch.Tensor] = None):
    """The module docstring's arithmetic in torch on the CPU, vectorised over the batch: ``images`` uint8
    ``[N, C, H, W]``, ``masks`` uint8 ``[N, H, W]``, ``idx`` int64 ``[B]`` in ``[0, N)``, ``mats`` int32 ``[B, 6]``,
    ``luts`` float32 ``[B, 256]`` or None (``unit_table``) -> float32 ``([B, C, H, W], [B, 1, H, W])``.
    The tests' reference, and the loader's path for a dataset resident on the CPU."""
    from ..ops.kernels import unit_table
    N, C, H, W = images.shape
    idx = idx.to(torch.int64).cpu()
    B = idx.numel()
    assert tuple(masks.shape) == (N, H, W) and tuple(mats.shape) == (B, 6) and mats.dtype == torch.int32
    assert B > 0 and int(idx.min()) >= 0 and int(idx.max()) < N, "index outside the dataset"
    m = mats.cpu().to(torch.int64).view(B, 6, 1, 1)
    x = torch.arange(W, dtype=torch.int64).view(1, 1, W)
    y = torch.arange(H, dtype=torch.int64).view(1, H, 1)
    sx = m[:, 0] * x + m[:, 1] * y + m[:, 2]                       # [B, H, W]
    sy = m[:, 3] * x + m[:, 4] * y + m[:, 5]
    x0, fx = sx >> 16, (sx & 0xFFFF) >> 8
    y0, fy = sy >> 16, (sy & 0xFFFF) >> 8
    xa, xb = x0.clamp(0, W - 1), (x0 + 1).clamp(0, W - 1)
    ya, yb = y0.clamp(0, H - 1) * W, (y0 + 1).clamp(0, H - 1) * W
    src = images.cpu().index_select(0, idx).reshape(B, C, H * W).to(torch.int64)

    def tap(off):
        return src.gather(2, off.view(B, 1, H * W).expand(B, C, H * W))

    w = [w.view(B, 1, H * W) for w in ((256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy)]
    v = (w[0] * tap(ya + xa) + w[1] * tap(ya + xb) + w[2] * tap(yb + xa) + w[3] * tap(yb + xb) + 32768) >> 16
    if luts is None:
        table = unit_table("cpu").view(1, 256).expand(B, 256)
    else:
        assert luts.dtype == torch.float32 and tuple(luts.shape) == (B, 256)
        table = luts.cpu()
    img = table.gather(1, v.view(B, C * H * W)).view(B, C, H, W)
    mo = ((sy + 32768) >> 16).clamp(0, H - 1) * W + ((sx + 32768) >> 16).clamp(0, W - 1)
    tgt = masks.cpu().index_select(0, idx).reshape(B, H * W).gather(1, mo.view(B, H * W))
    return img.contiguous(), tgt.to(torch.float32).view(B, 1, H, W)


def spec_from_config(cfg) -> AugmentSpec:
    """The run's spec: ``cfg.augment`` with the ``--aug-*`` magnitudes that were given."""
    return AugmentSpec.parse(cfg.augment, **{m: getattr(cfg, f"aug_{m}", None) for m in MAGNITUDES})


__all__ = ["AugmentSpec", "NAMES", "MAGNITUDES", "aug_uniform", "affine_matrices", "inverse_affine", "to_q16",
           "color_luts", "augment_reference",
           "canonical", "spec_from_config"]
