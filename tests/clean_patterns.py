"""Masks for the cleaning tests (``clean_reference`` / ``dpa_mask_clean``): every pattern at every size.

The device labeller works on tiles of 16 x 64 pixels: (130, 259) spans 9 x 5 of them with ragged edges, (5, 4099)
has rows longer and (2051, 3) columns taller than any tile."""
import numpy as np

SIZES = [(1, 1), (3, 5), (37, 53), (64, 96), (130, 259), (5, 4099), (2051, 3)]
DENSITIES = (0.30, 0.50, 0.59)                   # around the 8- and 4-connectivity percolation thresholds


def _corner(H, W, k):
    m = np.zeros((H, W), np.uint8)
    m[(0, 0, H - 1, H - 1)[k], (0, W - 1, 0, W - 1)[k]] = 255
    return m


def _checker(H, W, phase=0):
    y, x = np.mgrid[:H, :W]
    return (((y + x + phase) & 1) == 0).astype(np.uint8) * 255


def _frame(H, W):
    m = np.zeros((H, W), np.uint8)
    m[0], m[-1], m[:, 0], m[:, -1] = 255, 255, 255, 255
    return m


def _rings(H, W):
    """Concentric one-pixel rectangles two pixels apart: nested components inside holes."""
    y, x = np.mgrid[:H, :W]
    d = np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x))
    return ((d % 3) == 0).astype(np.uint8) * 255


def _snake(H, W):
    """Even rows full, odd rows one pixel alternately at the right and the left end: one component through
    every tile."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 255
    m[1::4, W - 1] = 255
    m[3::4, 0] = 255
    return m


def _random(H, W, density):
    rng = np.random.default_rng(int(density * 100) * 7919 + H * 131 + W)
    return (rng.random((H, W)) < density).astype(np.uint8) * 255


def _rects(H, W, shift):
    """Two rectangles of equal area side by side (``shift``: the right one starts a row higher): the tie rule."""
    m = np.zeros((H, W), np.uint8)
    h, w = max(1, H // 3), max(1, W // 5)
    top = min(H - h, max(1, H // 3))
    m[top:top + h, W // 10:W // 10 + w] = 255
    m[top - shift:top - shift + h, W // 2 + 1:W // 2 + 1 + w] = 255
    return m


def _bytes(H, W):
    rng = np.random.default_rng(H * 1009 + W)
    return np.array([0, 1, 7, 255], np.uint8)[rng.integers(0, 4, (H, W))]


PATTERNS = {
    "zeros": lambda H, W: np.zeros((H, W), np.uint8),
    "ones": lambda H, W: np.full((H, W), 255, np.uint8),
    "corner0": lambda H, W: _corner(H, W, 0),
    "corner1": lambda H, W: _corner(H, W, 1),
    "corner2": lambda H, W: _corner(H, W, 2),
    "corner3": lambda H, W: _corner(H, W, 3),
    "checker": _checker,
    "checker_inv": lambda H, W: _checker(H, W, 1),
    "frame": _frame,
    "rings": _rings,
    "snake": _snake,
    "random30": lambda H, W: _random(H, W, 0.30),
    "random50": lambda H, W: _random(H, W, 0.50),
    "random59": lambda H, W: _random(H, W, 0.59),
    "rects": lambda H, W: _rects(H, W, 0),
    "rects_shifted": lambda H, W: _rects(H, W, 1),
    "bytes": _bytes,
}
CASES = [(name, size) for name in PATTERNS for size in SIZES]
FLAGS = [(True, False), (False, True), (True, True)]          # (largest, fill)


def pattern(name, size):
    m = PATTERNS[name](*size)
    assert m.shape == tuple(size) and m.dtype == np.uint8
    return np.ascontiguousarray(m)


def blob_with_speckle(H, W, seed=0, holes=True):
    """An ellipse with a window hole, XOR sparse speckle: what a thresholded prediction looks like."""
    y, x = np.mgrid[:H, :W]
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    m = ((y - cy) / (0.35 * H + 0.5)) ** 2 + ((x - cx) / (0.4 * W + 0.5)) ** 2 <= 1.0
    if holes:
        m &= ~((abs(y - cy) <= H / 12.0) & (abs(x - cx) <= W / 10.0))
    rng = np.random.default_rng(seed)
    m ^= rng.random((H, W)) < 0.02
    return m.astype(np.uint8) * 255
