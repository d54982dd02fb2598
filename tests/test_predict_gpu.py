"""csrc/predict_post.hip and predict.py on the GPU: ``dpa_prob_to_mask_u8`` against PIL's mode-F bilinear resize +
strict threshold (bit for bit), ``dpa_mask_rle`` against the numpy oracle (exact, overflow included), the
launchers' argument checks, and ``Predictor.predict_files`` against the host post-processing of the same
probabilities."""
import ctypes

import numpy as np
import pytest
import torch

from distributedpytorch_amd.ops import _lib

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

from test_device_folder_cpu import write_tree  # noqa: E402
from test_predict_cpu import edge_masks  # noqa: E402

INVALID = 1   # hipErrorInvalidValue
gpu = pytest.mark.gpu
FILL = 77

# (h, w) -> (H, W)
SHAPES = [((16, 24), (37, 53)),         # ragged up-scale
          ((64, 96), (128, 191)),       # the Carvana ratio with its odd width
          ((32, 24), (32, 48)),         # vertical pass skipped
          ((8, 8), (8, 8)),             # identity
          ((48, 16), (20, 31)),         # down-scale (ksize 7) on one axis, up-scale on the other
          ((7, 5), (3, 11))]            # tiny, down-scale plus up-scale


@pytest.fixture(scope="module")
def K(hip_lib):
    from distributedpytorch_amd.ops import kernels
    return kernels


def _pil_mask(p, H, W, thr, value=255):
    r = np.asarray(Image.fromarray(p).resize((W, H), resample=Image.BILINEAR))
    return torch.from_numpy((r > np.float32(thr)).astype(np.uint8) * np.uint8(value))


def _inputs(shape, seed):
    """Uniform floats, and {0, 0.5, 1}: many interpolated values sit exactly at or next to the threshold."""
    rng = np.random.default_rng(seed)
    return rng.random(shape, dtype=np.float32), rng.choice(np.float32([0, 0.5, 1]), size=shape)


# ---- prob_to_mask_u8 ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_prob_to_mask_equals_pil(K, src, dst, thr):
    for p in _inputs(src, src[0] + dst[1]):
        out = torch.full((1,) + dst, FILL, dtype=torch.uint8, device="cuda")
        assert K.prob_to_mask_u8(torch.from_numpy(p)[None].cuda(), out, thr)
        ref = _pil_mask(p, *dst, thr)
        assert 0 < int(ref.count_nonzero()) < ref.numel() or src == (7, 5)
        assert torch.equal(out[0].cpu(), ref)


@gpu
def test_prob_to_mask_batch_and_value(K):
    """B = 3 with distinct content per image, from a destination that is not 4-byte aligned, value 1."""
    (h, w), (H, W) = (16, 24), (37, 53)
    ps = [p for s in (1, 2) for p in _inputs((h, w), s)][:3]
    probs = torch.from_numpy(np.stack(ps)).cuda()
    buf = torch.full((3 * H * W + 8,), FILL, dtype=torch.uint8, device="cuda")
    for off, value in ((0, 255), (1, 1)):
        buf.fill_(FILL)
        out = buf[off:off + 3 * H * W].view(3, H, W)
        assert K.prob_to_mask_u8(probs, out, 0.5, value)
        for b in range(3):
            assert torch.equal(out[b].cpu(), _pil_mask(ps[b], H, W, 0.5, value)), (off, b)
        assert (buf[:off] == FILL).all() and (buf[off + 3 * H * W:] == FILL).all()


@gpu
def test_prob_to_mask_refuses_beyond_4x(K):
    """40 -> 8 rows is 5x: ksize 11.  The wrapper returns False and nothing is launched."""
    p = torch.rand(1, 40, 8, device="cuda")
    out = torch.full((1, 8, 8), FILL, dtype=torch.uint8, device="cuda")
    assert K.prob_to_mask_u8(p, out) is False
    torch.cuda.synchronize()
    assert (out == FILL).all()
    assert K.prob_to_mask_u8(torch.rand(1, 32, 8, device="cuda"), out) is True      # 4x: ksize 9 is accepted
    assert (out != FILL).all()


# ---- mask_rle ----------------------------------------------------------------------------------------------------
def _check_rle(K, masks, cap):
    runs, counts = K.mask_rle(torch.from_numpy(masks).cuda(), cap)
    assert runs.dtype == counts.dtype == torch.int32 and tuple(runs.shape) == (len(masks), cap, 2)
    runs, counts = runs.cpu().numpy(), counts.cpu().numpy()
    for b, m in enumerate(masks):
        ref = K.rle_reference(m)
        assert counts[b] == len(ref), (b, counts[b], len(ref))
        assert np.array_equal(runs[b, :len(ref)], ref), b


@gpu
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (37, 53), (5, 4099), (64, 96)])
def test_mask_rle_equals_reference(K, size):
    """(5, 4099): rows longer than a tile, no multiple of the wave size; (64, 96): the 16-byte load path, two tiles."""
    named = edge_masks(*size, seed=size[1])
    cap = size[0] * size[1] // 2 + 1                              # alternating pixels: the maximum run count
    for name, m in named.items():
        _check_rle(K, m[None], cap)
    _check_rle(K, np.stack([named["blobs"], named["zero"], named["alternate"]]), cap)     # B = 3, different counts


@gpu
def test_mask_rle_unaligned_images(K):
    """Images of 37 * 53 bytes: the second and third start at an odd address (byte-load path)."""
    rng = np.random.default_rng(4)
    _check_rle(K, (rng.random((3, 37, 53)) > 0.6).astype(np.uint8), 1000)


@gpu
def test_mask_rle_overflow(K):
    """cap below the run count: counts stay exact, the first cap runs are right, nothing is written behind them."""
    m = edge_masks(37, 53, seed=9)
    masks = torch.from_numpy(np.stack([m["alternate"], m["row_end"], m["blobs"]])).cuda()
    cap, L = 5, _lib.lib()
    runs = torch.full((3, cap + 3, 2), -FILL, dtype=torch.int32, device="cuda")          # 3 guard runs per image...
    tiles = L.dpa_mask_rle_tiles(ctypes.c_int(37), ctypes.c_int(53))
    assert tiles == 1
    work = torch.zeros(3 * tiles, dtype=torch.int32, device="cuda")
    counts = torch.full((4,), -FILL, dtype=torch.int32, device="cuda")
    # ...by launching each image on its own with the guarded buffer as a [1, cap, 2] list
    for b in range(3):
        err = L.dpa_mask_rle(_lib.ptr(masks[b]), ctypes.c_int(1), ctypes.c_int(37), ctypes.c_int(53), _lib.ptr(runs[b]),
                             ctypes.c_int(cap), _lib.ptr(counts[b:]), _lib.ptr(work), ctypes.c_longlong(tiles),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert err == 0
    runs, counts = runs.cpu().numpy(), counts.cpu().numpy()
    assert counts[3] == -FILL
    for b, name in enumerate(("alternate", "row_end", "blobs")):
        ref = K.rle_reference(m[name])
        assert counts[b] == len(ref)
        n = min(len(ref), cap)
        assert np.array_equal(runs[b, :n], ref[:n])
        assert (runs[b, n:] == -FILL).all(), name
    assert counts[0] > cap and counts[1] == 1 and counts[2] > cap
    # the wrapper: same counts
    _, c = K.mask_rle(masks, cap)
    assert c.cpu().tolist() == counts[:3].tolist()


# ---- host-side contracts: every launcher returns before it touches the device (no GPU needed) ----------------
needs_lib = pytest.mark.skipif(not _lib.LIB_PATH.exists(), reason="HIP library not built")
P = ctypes.c_void_p(0x1000)      # never dereferenced: the host checks return first
i32 = ctypes.c_int


def _p2m(L, B=1, h=16, w=24, H=37, W=53, kh=3, kv=3, value=255, probs=P, dst=P, hb=P, hc=P, vb=P, vc=P):
    return L.dpa_prob_to_mask_u8(probs, i32(B), i32(h), i32(w), dst, i32(H), i32(W), hb, hc, i32(kh), vb, vc, i32(kv),
                                 ctypes.c_float(0.5), i32(value), None)


def _rle(L, B=1, H=37, W=53, cap=8, work_elems=1, masks=P, runs=P, counts=P, work=P):
    return L.dpa_mask_rle(masks, i32(B), i32(H), i32(W), runs, i32(cap), counts, work, ctypes.c_longlong(work_elems), None)


P2M_BAD = [dict(B=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=-3), dict(probs=None), dict(dst=None), dict(hb=None),
           dict(hc=None), dict(vb=None), dict(vc=None), dict(kh=1), dict(kv=5), dict(kh=9), dict(value=256),
           dict(h=40, w=8, H=8, W=8, kh=1, kv=11),             # matching tables, 5x down: beyond the kernel's taps
           dict(H=16, kv=3), dict(H=65536, W=65536)]
RLE_BAD = [dict(B=0), dict(H=0), dict(W=-1), dict(cap=0), dict(cap=-4), dict(masks=None), dict(runs=None),
           dict(counts=None), dict(work=None), dict(work_elems=0), dict(H=65536, W=32768), dict(B=3)]


@needs_lib
@pytest.mark.parametrize("kw", P2M_BAD)
def test_prob_to_mask_launcher_rejects(kw):
    """24 -> 53 and 16 -> 37 are up-scales: ksize 3; equal sizes carry the identity table, ksize 1."""
    assert _p2m(_lib.lib(), **kw) == INVALID


@needs_lib
@pytest.mark.parametrize("kw", RLE_BAD)
def test_mask_rle_launcher_rejects(kw):
    """2^31 pixels, a scratch smaller than B * tiles (B=3 with one tile's worth), cap < 1, null pointers."""
    assert _rle(_lib.lib(), **kw) == INVALID


@needs_lib
def test_mask_rle_tiles():
    L = _lib.lib()
    t = lambda H, W: L.dpa_mask_rle_tiles(i32(H), i32(W))  # noqa: E731
    assert (t(1, 1), t(1, 4095), t(1, 4096), t(64, 64), t(1280, 1918)) == (1, 1, 2, 2, 600)
    assert t(0, 5) == 0 and t(65536, 32768) == 0


@gpu
def test_launchers_reject_without_writing(K):
    """The same bad arguments with real buffers: the return value is 1 and every output keeps its fill."""
    L = _lib.lib()
    probs = torch.rand(1, 16, 24, device="cuda")
    dst = torch.full((1, 37, 53), FILL, dtype=torch.uint8, device="cuda")
    hb, hc, _ = K._bilinear_device_table(24, 53, "cuda")
    vb, vc, _ = K._bilinear_device_table(16, 37, "cuda")
    good = dict(probs=_lib.ptr(probs), dst=_lib.ptr(dst), hb=_lib.ptr(hb), hc=_lib.ptr(hc), vb=_lib.ptr(vb), vc=_lib.ptr(vc))
    for kw in P2M_BAD:
        if kw.get("H", 0) > 37 or kw.get("h", 0) > 16:
            continue                                            # sizes beyond these buffers: host-only above
        assert _p2m(L, **{**good, **kw}) == INVALID, kw
    masks = torch.ones(1, 37, 53, dtype=torch.uint8, device="cuda")
    runs = torch.full((1, 8, 2), -FILL, dtype=torch.int32, device="cuda")
    counts = torch.full((1,), -FILL, dtype=torch.int32, device="cuda")
    work = torch.full((1,), -FILL, dtype=torch.int32, device="cuda")
    good = dict(masks=_lib.ptr(masks), runs=_lib.ptr(runs), counts=_lib.ptr(counts), work=_lib.ptr(work))
    for kw in RLE_BAD:
        if kw.get("H", 0) > 37:
            continue
        assert _rle(L, **{**good, **kw}) == INVALID, kw
    torch.cuda.synchronize()
    assert (dst == FILL).all() and (runs == -FILL).all() and (counts == -FILL).all() and (work == -FILL).all()
    with pytest.raises(AssertionError):                          # the Python wrappers assert before they launch
        K.prob_to_mask_u8(probs.cpu(), dst)
    with pytest.raises(AssertionError):
        K.mask_rle(masks, 0)


# ---- end to end ------------------------------------------------------------------------------------------------
@gpu
def test_predict_files_equals_host_post(tmp_path, hip_lib):
    """5 files of two source sizes, batch size 2: device masks and run lists equal PIL + numpy on the SAME
    downloaded probabilities; a run-list capacity of 1 sends the overflowing files to the host, same result."""
    from distributedpytorch_amd.models.unet import build_model
    from distributedpytorch_amd.ops import kernels as K
    from distributedpytorch_amd.predict import Predictor, host_mask
    imgs, _ = write_tree(tmp_path / "data", n=5)
    files = sorted(str(p) for p in imgs.iterdir())
    torch.manual_seed(3)
    model = build_model("unet")
    with torch.no_grad():                           # a random net's output hugs 0.5: spread it over the threshold
        for p in model.parameters():
            p.mul_(3.0)
    pred = Predictor(model, "cuda:0", (64, 96), threshold=0.5, rle_cap=1000)      # 37 * 53 / 2 < 1000: no overflow
    assert pred.strat.compute.name.startswith("hip") and not pred.host_post

    seen = []
    real_probs = pred.probs

    def spy(x):
        p = real_probs(x)
        seen.append(p.cpu().numpy())
        return p

    pred.probs = spy
    recs = list(pred.predict_files(files, batch_size=2, workers=2))
    assert [r[0] for r in recs] == files and pred.host_finished == 0
    host = np.concatenate(seen)
    assert host.shape == (5, 64, 96) and host.dtype == np.float32
    counts = []
    for i, (path, size, mask, runs) in enumerate(recs):
        assert size == Image.open(path).size[::-1] and mask.dtype == np.uint8 and runs.dtype == np.int32
        ref = host_mask(host[i], size, 0.5)
        assert np.array_equal(mask, ref), path
        assert np.array_equal(runs, K.rle_reference(ref)), path
        counts.append(len(runs))
    assert {r[1] for r in recs} == {(32, 48), (37, 53)} and max(counts) > 1

    pred.rle_cap = 1
    again = list(pred.predict_files(files, batch_size=3, workers=2))
    assert pred.host_finished == sum(c > 1 for c in counts) > 0
    for a, b in zip(again, recs):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])

    only_rle = list(pred.predict_files(files[:3], batch_size=2, workers=1, want_masks=False))
    assert all(r[2] is None for r in only_rle)
    pred.rle_cap = None                             # the default capacity, 4 * source height
    only_rle = list(pred.predict_files(files[:3], batch_size=2, workers=1, want_masks=False))
    assert all(r[2] is None and np.array_equal(r[3], b[3]) for r, b in zip(only_rle, recs))
