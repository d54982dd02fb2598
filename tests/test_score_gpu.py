"""``dpa_prob_score`` (csrc/predict_post.hip) and ``Predictor.score_files`` on the GPU: the counts against
``score_reference`` (PIL + numpy) exactly, the launcher's argument checks, and the device path against the host
path on files."""
import ctypes

import numpy as np
import pytest
import torch

from distributedpytorch_amd.ops import _lib

PIL = pytest.importorskip("PIL")

from test_device_folder_cpu import write_tree  # noqa: E402
from test_predict_gpu import _inputs  # noqa: E402
from test_score_cpu import THRESHOLDS, blob_truth  # noqa: E402

INVALID = 1   # hipErrorInvalidValue
gpu = pytest.mark.gpu
GARBAGE = -0x0123456789abcdef

# (h, w) -> (H, W)
SHAPES = [((16, 24), (37, 53)),         # ragged: dead lanes and rows
          ((64, 96), (128, 191)),       # three column blocks
          ((32, 24), (32, 48)),         # vertical pass skipped
          ((8, 8), (8, 8)),             # identity
          ((48, 16), (20, 31)),         # ksize 7
          ((7, 5), (3, 11)),            # tiny
          ((16, 24), (130, 70)),        # three row blocks
          ((40, 40), (1030, 1100))]     # 306 slab rows: more than one pass of the 256-thread reducing workgroup
TINY = [(3, 11)]                        # 33 pixels: the only shape whose reference counts are not all mixed
T8 = THRESHOLDS + [0.9, 0.25, 0.1, 0.6]          # any order, one repeated


@pytest.fixture(scope="module")
def K(hip_lib):
    from distributedpytorch_amd.ops import kernels
    return kernels


def _score(K, probs, truths, cuts, thresholds):
    out = K.prob_score(torch.from_numpy(np.stack(probs)).cuda(), torch.from_numpy(np.stack(truths)).cuda(),
                       torch.tensor(cuts, dtype=torch.int32).cuda(), thresholds)
    assert out.dtype == torch.int64 and tuple(out.shape) == (len(probs), 1 + 2 * len(thresholds)) and out.is_cuda
    return out.cpu().numpy()


@gpu
@pytest.mark.parametrize("src,dst", SHAPES)
def test_prob_score_equals_reference(K, src, dst):
    truth = blob_truth(*dst, seed=dst[0])
    for n, p in enumerate(_inputs(src, src[0] + dst[1])):
        ref = K.score_reference(p, truth, 127, T8)
        for thr in (T8, THRESHOLDS, [0.5]):                       # T = 8, 4 and 1
            want = ref if thr is T8 else K.score_reference(p, truth, 127, thr)
            got = _score(K, [p], [truth], [127], thr)[0]
            print(src, dst, len(thr), got.tolist())
            assert got.tolist() == want.tolist(), (src, dst, len(thr))
        r4 = ref[:9]
        if dst not in TINY:                                      # a kernel that returns zeros, or counts one of the two
            assert all(0 < r4[2 + 2 * t] < min(r4[1 + 2 * t], r4[0]) for t in range(4)), r4
        if n == 1 and src == dst:                                # {0, 0.5, 1} unresized: 0.5 itself is not "> 0.5"
            assert r4[3] > r4[5] and r4[3] - r4[5] == int((p == 0.5).sum())


@gpu
def test_prob_score_batch_mixed_cut(K):
    """B = 3: a 0/1 truth with cut 0, an all-zero and an all-255 truth with cut 127; the output starts as garbage."""
    (h, w), (H, W) = (16, 24), (37, 53)
    ps = [p for s in (1, 2) for p in _inputs((h, w), s)][:3]
    truths = [blob_truth(H, W, seed=5) // 255, np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)]
    cuts = [0, 127, 127]
    L = _lib.lib()
    probs, truth = torch.from_numpy(np.stack(ps)).cuda(), torch.from_numpy(np.stack(truths)).cuda()
    hb, hc, kh = K._bilinear_device_table(w, W, "cuda")
    vb, vc, kv = K._bilinear_device_table(h, H, "cuda")
    cut = torch.tensor(cuts, dtype=torch.int32).cuda()
    blocks = L.dpa_prob_score_blocks(i32(H), i32(W))
    assert blocks == 1
    for thr in ([0.5], THRESHOLDS, T8):
        n = 1 + 2 * len(thr)
        counts = torch.full((3 * n + 2,), GARBAGE, dtype=torch.int64, device="cuda")
        work = torch.full((3 * blocks * n,), -1, dtype=torch.int32, device="cuda")
        err = L.dpa_prob_score(_lib.ptr(probs), i32(3), i32(h), i32(w), _lib.ptr(truth), _lib.ptr(cut), i32(H),
                               i32(W), _lib.ptr(hb), _lib.ptr(hc), i32(kh), _lib.ptr(vb), _lib.ptr(vc), i32(kv),
                               (ctypes.c_float * len(thr))(*thr), i32(len(thr)), _lib.ptr(counts), _lib.ptr(work),
                               ctypes.c_longlong(work.numel()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert err == 0
        got = counts.cpu().numpy()
        assert (got[3 * n:] == GARBAGE).all()                      # nothing behind [B][n]
        for b in range(3):
            ref = K.score_reference(ps[b], truths[b], cuts[b], thr)
            assert got[b * n:(b + 1) * n].tolist() == ref.tolist(), (len(thr), b)
        got = got[:3 * n].reshape(3, n)
        assert got[1, 0] == 0 and (got[1, 2::2] == 0).all()                       # no truth: no intersection
        assert got[2, 0] == H * W and (got[2, 2::2] == got[2, 1::2]).all()        # all truth: inter == pred
        assert 0 < got[0, 0] < H * W
        d, i = K.dice_iou(got)
        assert d.shape == (3, len(thr)) and (d[1][got[1, 1::2] > 0] == 0).all()


@gpu
def test_prob_score_refuses_beyond_4x(K):
    """40 -> 8 rows is 5x: ksize 11.  The wrapper returns None and nothing is launched; 4x is accepted."""
    truth = torch.from_numpy(blob_truth(8, 8)).cuda()[None]
    cut = torch.tensor([127], dtype=torch.int32).cuda()
    assert K.prob_score(torch.rand(1, 40, 8, device="cuda"), truth, cut, [0.5]) is None
    p = torch.rand(1, 32, 8, device="cuda")
    got = K.prob_score(p, truth, cut, [0.5])
    assert got.cpu().numpy()[0].tolist() == K.score_reference(p[0].cpu().numpy(), truth[0].cpu().numpy(), 127, [0.5]).tolist()
    with pytest.raises(AssertionError):
        K.prob_score(p, truth, cut, [0.5] * 9)
    with pytest.raises(AssertionError):
        K.prob_score(p.cpu(), truth, cut, [0.5])


# ---- host-side contracts: the launcher returns before it touches the device (no GPU needed) --------------------
needs_lib = pytest.mark.skipif(not _lib.LIB_PATH.exists(), reason="HIP library not built")
P = ctypes.c_void_p(0x1000)      # never dereferenced: the host checks return first
i32 = ctypes.c_int
HOST_THR = (ctypes.c_float * 8)(*([0.5] * 8))


def _ps(L, B=1, h=16, w=24, H=37, W=53, kh=3, kv=3, T=1, work_elems=17, probs=P, truth=P, cut=P, hb=P, hc=P, vb=P,
        vc=P, thresholds=HOST_THR, counts=P, work=P):
    return L.dpa_prob_score(probs, i32(B), i32(h), i32(w), truth, cut, i32(H), i32(W), hb, hc, i32(kh), vb, vc,
                            i32(kv), thresholds, i32(T), counts, work, ctypes.c_longlong(work_elems), None)


PS_BAD = [dict(probs=None), dict(truth=None), dict(cut=None), dict(hb=None), dict(hc=None), dict(vb=None),
          dict(vc=None), dict(thresholds=None), dict(counts=None), dict(work=None),
          dict(B=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=-3), dict(T=0), dict(T=9), dict(T=-1),
          dict(kh=1), dict(kv=5), dict(kh=9), dict(H=16, kv=3),
          dict(h=40, w=8, H=8, W=8, kh=1, kv=11),             # matching tables, 5x down: beyond the kernel's taps
          dict(H=65536, W=65536, work_elems=1 << 40), dict(h=65536, w=32768),             # 2^32 and 2^31 pixels
          dict(w=1, W=1, kh=1, H=64 * 65535 + 1, work_elems=1 << 40), dict(B=65536, work_elems=1 << 40),   # grid.y, grid.z
          dict(work_elems=2), dict(T=8, work_elems=16), dict(B=3, T=2, work_elems=14)]    # B * blocks * (1 + 2T) - 1


@needs_lib
@pytest.mark.parametrize("kw", PS_BAD)
def test_prob_score_launcher_rejects(kw):
    """24 -> 53 and 16 -> 37 are up-scales: ksize 3, one workgroup per image."""
    assert _ps(_lib.lib(), **kw) == INVALID


@needs_lib
def test_prob_score_blocks():
    L = _lib.lib()
    t = lambda H, W: L.dpa_prob_score_blocks(i32(H), i32(W))  # noqa: E731
    assert (t(1, 1), t(64, 64), t(65, 64), t(64, 65), t(130, 70), t(1030, 1100), t(1280, 1918)) == (1, 1, 2, 2, 6, 306, 600)
    assert t(64 * 65535, 1) == 65535
    assert t(0, 5) == 0 and t(5, -1) == 0 and t(65536, 32768) == 0 and t(64 * 65535 + 1, 1) == 0


@gpu
def test_prob_score_rejects_without_writing(K):
    """The same bad arguments with real buffers: the return value is 1 and the outputs keep their fill."""
    L = _lib.lib()
    probs = torch.rand(1, 16, 24, device="cuda")
    truth = torch.zeros(1, 37, 53, dtype=torch.uint8, device="cuda")
    cut = torch.zeros(1, dtype=torch.int32, device="cuda")
    hb, hc, _ = K._bilinear_device_table(24, 53, "cuda")
    vb, vc, _ = K._bilinear_device_table(16, 37, "cuda")
    counts = torch.full((17,), GARBAGE, dtype=torch.int64, device="cuda")
    work = torch.full((17,), -1, dtype=torch.int32, device="cuda")
    good = dict(probs=_lib.ptr(probs), truth=_lib.ptr(truth), cut=_lib.ptr(cut), hb=_lib.ptr(hb), hc=_lib.ptr(hc),
                vb=_lib.ptr(vb), vc=_lib.ptr(vc), counts=_lib.ptr(counts), work=_lib.ptr(work))
    for kw in PS_BAD:
        assert _ps(L, **{**good, **kw}) == INVALID, kw
    torch.cuda.synchronize()
    assert (counts == GARBAGE).all() and (work == -1).all()
    assert _ps(L, **good, T=8) == 0                              # and the good call does write: 17 counts
    assert (counts.cpu() != GARBAGE).all()


# ---- end to end ------------------------------------------------------------------------------------------------
@gpu
def test_score_files_equals_host_post(tmp_path, hip_lib):
    """6 files of two source sizes, batch size 4 (both sizes in a batch): the device counts equal the host path's
    on the same model; a source more than 4x smaller than the network size is finished on the host."""
    from distributedpytorch_amd.models.unet import build_model
    from distributedpytorch_amd.ops import kernels as K
    from distributedpytorch_amd.predict import Predictor, match_masks
    from PIL import Image
    imgs, masks = write_tree(tmp_path / "data", n=6)
    pairs = match_masks(sorted(str(p) for p in imgs.iterdir()), masks)
    torch.manual_seed(3)
    model = build_model("unet")
    with torch.no_grad():                           # a random net's output hugs 0.5: spread it over the threshold
        for p in model.parameters():
            p.mul_(3.0)
    pred = Predictor(model, "cuda:0", (64, 96))
    assert pred.strat.compute.name.startswith("hip") and not pred.host_post
    real_probs = pred.probs

    def both(jobs, batch_size):
        """The device path, then the host path on the SAME probabilities (replayed batch by batch)."""
        seen = []

        def spy(x):
            seen.append(real_probs(x))
            return seen[-1]

        pred.probs, pred.host_post, before = spy, False, pred.host_finished
        dev = list(pred.score_files(jobs, batch_size=batch_size, workers=2, thresholds=THRESHOLDS))
        on_host = pred.host_finished - before
        pred.probs, pred.host_post = (lambda x: seen.pop(0)), True
        host = list(pred.score_files(jobs, batch_size=batch_size, workers=2, thresholds=THRESHOLDS))
        assert pred.host_finished - before == on_host + len(jobs) and not seen
        pred.probs, pred.host_post = real_probs, False
        return dev, host, on_host

    dev, host, on_host = both(pairs, 4)
    assert on_host == 0 and [r[0] for r in dev] == [p for p, _ in pairs]
    assert {r[1] for r in dev[:4]} == {(32, 48), (37, 53)}
    for a, b in zip(dev, host):
        assert a[0] == b[0] and a[1] == b[1] and a[2].dtype == np.int64 and a[2].tolist() == b[2].tolist(), a[0]
    counts = np.stack([r[2] for r in dev])
    assert (counts[:, 0] > 0).all() and (counts[:, 2::2] > 0).any() and (counts[:, 2::2] < counts[:, 1::2]).any()

    # 64 / 12 rows > 4x: the launch is refused, the host scores; mixed with a normal file in one batch
    small = tmp_path / "small"
    small.mkdir()
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (12, 20, 3), dtype=np.uint8)).save(small / "s.png")
    Image.fromarray(blob_truth(12, 20)).save(small / "s_mask.png")
    got, want, on_host = both([(str(small / "s.png"), str(small / "s_mask.png")), pairs[0]], 2)
    assert on_host == 1 and got[0][1] == (12, 20)
    assert [g[2].tolist() for g in got] == [w[2].tolist() for w in want]
