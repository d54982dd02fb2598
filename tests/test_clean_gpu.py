"""``dpa_mask_clean`` and ``dpa_mask_score`` (csrc/mask_clean.hip) on the GPU: the cleaned mask and its stats against
``clean_reference`` (numpy) exactly on every pattern and size, the launchers' argument checks, and
``Predictor(clean=...)`` on the device against the host path on files."""
import ctypes

import numpy as np
import pytest
import torch

from distributedpytorch_amd.ops import _lib

PIL = pytest.importorskip("PIL")

from clean_patterns import FLAGS, PATTERNS, SIZES, blob_with_speckle, pattern  # noqa: E402
from test_device_folder_cpu import write_tree  # noqa: E402
from test_score_cpu import blob_truth  # noqa: E402

INVALID = 1   # hipErrorInvalidValue
gpu = pytest.mark.gpu
i32 = ctypes.c_int
_REF = {}


@pytest.fixture(scope="module")
def K(hip_lib):
    from distributedpytorch_amd.ops import kernels
    return kernels


def _ref(K, name, size, largest, fill):
    """``clean_reference`` of a pattern with value 255, computed once."""
    key = (name, tuple(size), largest, fill)
    if key not in _REF:
        _REF[key] = K.clean_reference(pattern(name, size), largest, fill, 255)
    return _REF[key]


@gpu
@pytest.mark.parametrize("name", list(PATTERNS))
def test_mask_clean_equals_reference(K, name):
    for size in SIZES:
        src = torch.from_numpy(pattern(name, size)).cuda()[None]
        before = src.clone()
        for largest, fill in FLAGS:
            want, wst = _ref(K, name, size, largest, fill)
            for value in (255, 1):
                got, st = K.mask_clean(src, largest, fill, value)
                assert got.dtype == torch.uint8 and got.shape == src.shape and st.dtype == torch.int32
                assert st.cpu().numpy()[0].tolist() == wst.tolist(), (name, size, largest, fill, value)
                assert np.array_equal(got.cpu().numpy()[0], want // 255 * value), (name, size, largest, fill, value)
        assert torch.equal(src, before)                      # the source is not modified


@gpu
def test_mask_clean_batch(K):
    """Three different images in one launch, one of them empty: nothing leaks between the images."""
    size = (130, 259)
    names = ["random59", "zeros", "rings"]
    src = torch.from_numpy(np.stack([pattern(n, size) for n in names])).cuda()
    for largest, fill in FLAGS:
        got, st = K.mask_clean(src, largest, fill)
        for b, n in enumerate(names):
            want, wst = _ref(K, n, size, largest, fill)
            assert np.array_equal(got[b].cpu().numpy(), want) and st[b].cpu().numpy().tolist() == wst.tolist(), (n, largest, fill)
    assert _ref(K, "random59", size, True, True)[1].min() > 0 and _ref(K, "rings", size, True, True)[1].min() > 0


def _clean_raw(L, src, dst_ptr, B, H, W, flags, value, stats, work):
    return L.dpa_mask_clean(_lib.ptr(src), i32(B), i32(H), i32(W), dst_ptr, i32(flags), i32(value), _lib.ptr(stats),
                            _lib.ptr(work), ctypes.c_longlong(work.numel()),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@gpu
def test_mask_clean_poisoned_buffers(K):
    """The workspace starts as 0x7f bytes, ``dst`` as a fill value at byte offset 1 of a larger buffer: the result is
    the reference's and the bytes around ``dst``, ``stats`` and the source are untouched."""
    L = _lib.lib()
    size = (37, 53)
    names = ["random50", "frame"]
    B, n = len(names), size[0] * size[1]
    src = torch.from_numpy(np.stack([pattern(s, size) for s in names])).cuda()
    per = L.dpa_mask_clean_work(i32(size[0]), i32(size[1]))
    assert per == 2 * n + 8
    for flags, (largest, fill) in zip((1, 2, 3), FLAGS):
        buf = torch.full((B * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        work = torch.full((B * per + 16,), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
        stats = torch.full((B * 3 + 4,), -7, dtype=torch.int32, device="cuda")
        dst_ptr = ctypes.c_void_p(buf.data_ptr() + 1)
        assert _clean_raw(L, src, dst_ptr, B, size[0], size[1], flags, 255, stats, work[:B * per]) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert got[0] == 0xA5 and (got[1 + B * n:] == 0xA5).all()
        assert (stats[B * 3:] == -7).all() and (work[B * per:] == 0x7f7f7f7f).all()
        for b, s in enumerate(names):
            want, wst = _ref(K, s, size, largest, fill)
            assert np.array_equal(got[1 + b * n:1 + (b + 1) * n].reshape(size), want), (s, flags)
            assert stats[3 * b:3 * b + 3].cpu().numpy().tolist() == wst.tolist(), (s, flags)
    assert np.array_equal(src.cpu().numpy(), np.stack([pattern(s, size) for s in names]))


@gpu
def test_mask_clean_twice_is_bit_equal(K):
    src = torch.from_numpy(np.stack([pattern("random50", (130, 259)), pattern("snake", (130, 259))])).cuda()
    a, sa = K.mask_clean(src, True, True)
    b, sb = K.mask_clean(src, True, True)
    assert torch.equal(a, b) and torch.equal(sa, sb)


@gpu
def test_mask_clean_realistic_blob(K):
    """An ellipse with a window and speckle, several tiles each way: what a thresholded prediction looks like."""
    m = blob_with_speckle(200, 331, seed=4)
    want, wst = K.clean_reference(m)
    got, st = K.mask_clean(torch.from_numpy(m).cuda()[None], True, True)
    assert np.array_equal(got.cpu().numpy()[0], want) and st.cpu().numpy()[0].tolist() == wst.tolist()
    assert wst[0] > 10 and wst[1] > 0 and wst[2] > 200


@gpu
@pytest.mark.parametrize("size", [(37, 53), (5, 4099)])
def test_mask_score_equals_numpy(K, size):
    """Blobs against ``blob_truth`` with a different ``cut`` per image: (truth, pred, inter) as numpy counts them."""
    H, W = size
    masks = np.stack([blob_with_speckle(H, W, seed=s) for s in (1, 2, 3)])
    masks[1] = masks[1] // 255 * 3                            # any non-zero byte is predicted
    truths = np.stack([blob_truth(H, W, seed=5), blob_truth(H, W, seed=6) // 255, np.full((H, W), 128, np.uint8)])
    cuts = [127, 0, 128]
    got = K.mask_score(torch.from_numpy(masks).cuda(), torch.from_numpy(truths).cuda(),
                       torch.tensor(cuts, dtype=torch.int32).cuda())
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, 3) and got.is_cuda
    got = got.cpu().numpy()
    for b in range(3):
        t, p = truths[b].astype(np.int64) > cuts[b], masks[b] != 0
        assert got[b].tolist() == [int(t.sum()), int(p.sum()), int((t & p).sum())], (size, b)
    assert 0 < got[0, 2] < min(got[0, 0], got[0, 1]) and got[2, 0] == 0 and got[2, 2] == 0
    # an unaligned view: the byte path
    flat = torch.zeros(3 * H * W + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = torch.from_numpy(masks).cuda().reshape(-1)
    again = K.mask_score(flat[1:].view(3, H, W), torch.from_numpy(truths).cuda(), torch.tensor(cuts, dtype=torch.int32).cuda())
    assert again.cpu().numpy().tolist() == got.tolist()


# ---- host-side contracts: the launchers return before they touch the device (no GPU needed) ---------------------
needs_lib = pytest.mark.skipif(not _lib.LIB_PATH.exists(), reason="HIP library not built")
P = ctypes.c_void_p(0x1000)      # never dereferenced: the host checks return first
Q = ctypes.c_void_p(0x2000)
PER = 2 * 37 * 53 + 8            # dpa_mask_clean_work(37, 53)


def _mc(L, B=1, H=37, W=53, flags=3, value=255, work_elems=PER, src=P, dst=Q, stats=P, work=P):
    return L.dpa_mask_clean(src, i32(B), i32(H), i32(W), dst, i32(flags), i32(value), stats, work,
                            ctypes.c_longlong(work_elems), None)


def _ms(L, B=1, H=37, W=53, work_elems=3, masks=P, truth=P, cut=P, counts=P, work=P):
    return L.dpa_mask_score(masks, truth, cut, i32(B), i32(H), i32(W), counts, work, ctypes.c_longlong(work_elems), None)


MC_BAD = [dict(src=None), dict(dst=None), dict(stats=None), dict(work=None),
          dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1),
          dict(flags=0), dict(flags=4), dict(flags=-1), dict(value=256), dict(value=0), dict(value=-1),
          dict(dst=P),                                          # src == dst
          dict(work=ctypes.c_void_p(0x1004)),                   # the header holds a 64-bit word
          dict(work_elems=PER - 1), dict(B=3, work_elems=3 * PER - 1),
          dict(H=65536, W=32768, work_elems=1 << 40),           # H * W = 2^31
          dict(H=32768, W=32768, work_elems=1 << 40),           # 2^30 pixels: the words per image pass int32
          dict(H=16 * 65535 + 1, W=1, work_elems=1 << 40),      # grid.y
          dict(B=65536, work_elems=1 << 40)]                    # grid.z
MS_BAD = [dict(masks=None), dict(truth=None), dict(cut=None), dict(counts=None), dict(work=None),
          dict(B=0), dict(B=-2), dict(H=0), dict(W=0), dict(H=-1), dict(W=-5),
          dict(work_elems=2), dict(B=3, work_elems=8),
          dict(H=65536, W=32768, work_elems=1 << 40),           # H * W = 2^31
          dict(B=65536, work_elems=1 << 40)]


@needs_lib
@pytest.mark.parametrize("kw", MC_BAD)
def test_mask_clean_launcher_rejects(kw):
    assert _mc(_lib.lib(), **kw) == INVALID


@needs_lib
@pytest.mark.parametrize("kw", MS_BAD)
def test_mask_score_launcher_rejects(kw):
    assert _ms(_lib.lib(), **kw) == INVALID


@needs_lib
def test_mask_clean_work_and_score_blocks():
    L = _lib.lib()
    w = lambda H, W: L.dpa_mask_clean_work(i32(H), i32(W))  # noqa: E731
    assert (w(1, 1), w(37, 53), w(1280, 1918)) == (10, PER, 2 * 1280 * 1918 + 8)
    assert w(16 * 65535, 1) == 2 * 16 * 65535 + 8 and w(16 * 65535 + 1, 1) == 0
    assert w(0, 5) == 0 and w(5, -1) == 0 and w(65536, 32768) == 0 and w(32768, 32768) == 0
    assert w(1, (1 << 30) - 5) == (1 << 31) - 2 and w(1, (1 << 30) - 4) == 0    # 2n + 8 must stay below 2^31
    t = lambda H, W: L.dpa_mask_score_blocks(i32(H), i32(W))  # noqa: E731
    assert (t(1, 1), t(64, 64), t(64, 65), t(37, 53), t(1280, 1918)) == (1, 1, 2, 1, 600)
    assert t(0, 5) == 0 and t(5, -1) == 0 and t(65536, 32768) == 0 and t(65536, 32767) == 524272


@gpu
def test_launchers_reject_without_writing(K):
    """The same bad arguments with real buffers: the return value is 1 and the outputs keep their fill."""
    L = _lib.lib()
    src = torch.from_numpy(pattern("random50", (37, 53))).cuda()[None]
    dst = torch.full((1, 37, 53), 0xA5, dtype=torch.uint8, device="cuda")
    stats = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    work = torch.full((PER,), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
    good = dict(src=_lib.ptr(src), dst=_lib.ptr(dst), stats=_lib.ptr(stats), work=_lib.ptr(work))
    for kw in MC_BAD:
        if "work" in kw and kw["work"] is not None:
            kw = dict(work=ctypes.c_void_p(work.data_ptr() + 4))
        if kw.get("dst") is P:
            kw = dict(dst=_lib.ptr(src))
        assert _mc(L, **{**good, **kw}) == INVALID, kw
    truth = torch.from_numpy(blob_truth(37, 53)).cuda()[None]
    cut = torch.zeros(1, dtype=torch.int32, device="cuda")
    counts = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    swork = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    sgood = dict(masks=_lib.ptr(src), truth=_lib.ptr(truth), cut=_lib.ptr(cut), counts=_lib.ptr(counts), work=_lib.ptr(swork))
    for kw in MS_BAD:
        assert _ms(L, **{**sgood, **kw}) == INVALID, kw
    torch.cuda.synchronize()
    assert (dst == 0xA5).all() and (stats == -7).all() and (work == 0x7f7f7f7f).all()
    assert (counts == -7).all() and (swork == -1).all()
    assert torch.equal(src.cpu(), torch.from_numpy(pattern("random50", (37, 53)))[None])
    assert _mc(L, **good) == 0 and _ms(L, **sgood) == 0          # and the good calls do write
    assert (stats.cpu() != -7).all() and (counts.cpu() != -7).all() and not (dst == 0xA5).any()
    # the wrappers: None for a size the launchers refuse is covered above; bad tensors are assertion errors
    with pytest.raises(AssertionError):
        K.mask_clean(src, False, False)
    with pytest.raises(AssertionError):
        K.mask_clean(src.cpu(), True, True)
    with pytest.raises(AssertionError):
        K.mask_score(src, truth, cut.long())


# ---- end to end ------------------------------------------------------------------------------------------------
@gpu
def test_clean_files_equals_host_post(tmp_path, hip_lib):
    """6 files of two source sizes, batch size 4 (both sizes in a batch), ``clean="largest+fill"``: masks, run lists,
    counts at two thresholds and ``clean_stats`` of the device path equal the host path's on the same probabilities;
    a source more than 4x smaller than the network size is finished on the host."""
    from distributedpytorch_amd.models.unet import build_model
    from distributedpytorch_amd.predict import Predictor, match_masks
    from PIL import Image
    imgs, masks = write_tree(tmp_path / "data", n=6)
    pairs = match_masks(sorted(str(p) for p in imgs.iterdir()), masks)
    torch.manual_seed(9)                            # a net whose masks have specks and holes (checked below)
    model = build_model("unet")
    with torch.no_grad():                           # a random net's output hugs 0.5: spread it over the threshold
        for p in model.parameters():
            p.mul_(3.0)
    pred = Predictor(model, "cuda:0", (64, 96), clean="fill+largest")
    assert pred.strat.compute.name.startswith("hip") and not pred.host_post and pred.clean == "largest+fill"
    real_probs = pred.probs
    thresholds = [0.5, 0.4]

    def run(jobs, batch_size):
        before = (pred.host_finished, pred.clean_stats.copy(), pred.clean_files, pred.clean_removed)
        res = list(pred.run_files(jobs, batch_size, 2, want_masks=True, want_rle=True, thresholds=thresholds))
        return res, (pred.host_finished - before[0], (pred.clean_stats - before[1]).tolist(),
                     pred.clean_files - before[2], pred.clean_removed - before[3])

    def both(jobs, batch_size):
        """The device path, then the host path on the SAME probabilities (replayed batch by batch)."""
        seen = []

        def spy(x):
            seen.append(real_probs(x))
            return seen[-1]

        pred.probs, pred.host_post = spy, False
        dev, dstat = run(jobs, batch_size)
        pred.probs, pred.host_post = (lambda x: seen.pop(0)), True
        host, hstat = run(jobs, batch_size)
        assert hstat[0] == len(jobs) and not seen
        pred.probs, pred.host_post = real_probs, False
        return dev, host, dstat, hstat

    dev, host, dstat, hstat = both(pairs, 4)
    assert dstat[0] == 0 and dstat[1:] == hstat[1:]
    first = hstat[1]
    assert {r[1] for r in dev[:4]} == {(32, 48), (37, 53)}
    for a, b in zip(dev, host):
        assert a[0] == b[0] and a[1] == b[1]
        assert a[2].dtype == np.uint8 and np.array_equal(a[2], b[2]) and set(np.unique(a[2]).tolist()) <= {0, 255}, a[0]
        assert a[3].dtype == np.int32 and np.array_equal(a[3], b[3]), a[0]
        assert a[4].dtype == np.int64 and a[4].tolist() == b[4].tolist(), a[0]
        assert a[4][1] == int((a[2] != 0).sum())                                  # the counts are the cleaned mask's
    # the cleaning changed these masks: components were removed and pixels filled
    assert hstat[1][0] > 6 and hstat[1][1] > 0 and hstat[1][2] > 0 and hstat[2] > 0 and hstat[3] > 0, hstat

    # 64 / 12 rows > 4x: the launch is refused, the host finishes; mixed with a normal file in one batch
    small = tmp_path / "small"
    small.mkdir()
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (12, 20, 3), dtype=np.uint8)).save(small / "s.png")
    Image.fromarray(blob_truth(12, 20)).save(small / "s_mask.png")
    got, want, dstat, hstat = both([(str(small / "s.png"), str(small / "s_mask.png")), pairs[0]], 2)
    assert dstat[0] == 1 and got[0][1] == (12, 20) and dstat[1:] == hstat[1:]
    for a, b in zip(got, want):
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4].tolist() == b[4].tolist()

    # without post(): score_files alone takes the stats of the first threshold, and the default stays dpa_prob_score
    pred.clean_stats[:] = 0
    alone = list(pred.score_files(pairs, 4, 2, thresholds=thresholds))
    assert [c.tolist() for _, _, c in alone] == [r[4].tolist() for r in dev]
    assert pred.clean_stats.tolist() == first
    plain = Predictor(model, "cuda:0", (64, 96))
    assert plain.clean == "none" and plain.clean_stats.tolist() == [0, 0, 0]
    raw = list(plain.score_files(pairs, 4, 2, thresholds=thresholds))
    assert [c.tolist() for _, _, c in raw] != [c.tolist() for _, _, c in alone]
    assert plain.clean_stats.tolist() == [0, 0, 0]
