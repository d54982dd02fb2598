"""csrc/tta.hip on the GPU: ``dpa_tta_views_f32`` against ``tta_views_reference`` and ``dpa_tta_accum`` against
``tta_merge_reference`` (both bit for bit, vector and scalar paths, bf16 and float32 sources), the launchers'
argument checks, and ``Predictor`` with ``tta`` and ``extra_models``: the device path against ``host_post`` and
against the reference merge of the members it computed."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from distributedpytorch_amd.ops import _lib
from distributedpytorch_amd.ops import kernels as KR

PIL = pytest.importorskip("PIL")

from test_device_folder_cpu import write_tree  # noqa: E402

INVALID = 1   # hipErrorInvalidValue
gpu = pytest.mark.gpu
FILL = 77.0
F32 = np.float32

# one pixel, ragged widths, exact vector widths, a vector width with more than one group per row and several blocks
HW = [(1, 1), (3, 5), (2, 16), (5, 17), (4, 32), (16, 52)]
SUBSETS = [list(c) for v in range(1, 5) for c in itertools.combinations(range(4), v)]      # 15 code subsets
MEMBERS = [0, 3, 1, 2, 1]                    # the codes of up to five members


@pytest.fixture(scope="module")
def K(hip_lib):
    return KR


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


# ---- tta_views ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bc", [(1, 1), (2, 3)])
@pytest.mark.parametrize("hw", HW)
def test_tta_views_equals_reference(K, bc, hw):
    (B, C), (h, w) = bc, hw
    rng = np.random.default_rng(B * 1000 + h * 10 + w)
    n = B * C * h * w
    flat = rng.integers(0, 256, size=n + 1, dtype=np.uint8)
    dev = torch.from_numpy(flat).cuda()
    for off in (0, 1):                       # off 1: a contiguous slice at an odd byte offset -> the scalar path
        u8 = dev[off:off + n].view(B, C, h, w)
        assert u8.is_contiguous() and u8.data_ptr() % 2 == off
        host = flat[off:off + n].reshape(B, C, h, w)
        for codes in SUBSETS:
            got = K.tta_views(u8, codes)
            assert got.dtype == torch.float32 and tuple(got.shape) == (len(codes), B, C, h, w)
            want = K.tta_views_reference(host, codes)
            assert np.array_equal(_bits(got), want.view(np.int32)), (off, codes)
        again = K.tta_views(u8, [0, 1, 2, 3])
        assert torch.equal(again, K.tta_views(u8, [0, 1, 2, 3]))               # two runs, the same bits
        assert np.array_equal(_bits(K.tta_views(u8, [3, 3, 0])), K.tta_views_reference(host, [3, 3, 0]).view(np.int32))


# ---- tta_accum ---------------------------------------------------------------------------------------------------
def _members(rng, N, B, h, w, dtype, exact=False):
    """N device tensors ``[B, h, w]`` of ``dtype`` cut from a flat buffer at element offsets 0 and 1, and the same
    values as float32 numpy arrays."""
    out = []
    for off in (0, 1):
        dev, host = [], []
        for _ in range(N):
            v = rng.choice(F32([0.0, 1.0]), size=B * h * w + 1) if exact else \
                rng.uniform(2.0 ** -20, 1.0, size=B * h * w + 1).astype(F32)
            t = torch.from_numpy(v).cuda().to(dtype)
            s = t[off:off + B * h * w].view(B, h, w)
            assert s.is_contiguous() and s.data_ptr() % 16 == off * t.element_size()
            dev.append(s)
            host.append(s.float().cpu().numpy())
        out.append((dev, host))
    return out


def _accumulate(K, dev, codes, prefill=None, as4d=False):
    B, h, w = dev[0].shape
    acc = torch.empty(B, h, w, dtype=torch.float32, device="cuda")
    if prefill is not None:
        acc.fill_(prefill)
    N = len(dev)
    for k, (m, c) in enumerate(zip(dev, codes)):
        K.tta_accum(acc, m.view(B, 1, h, w) if as4d else m, c, k == 0, k == N - 1, float(F32(1.0 / N)))
    return acc


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hw", HW)
def test_tta_accum_equals_reference(K, dtype, hw):
    h, w = hw
    for B in (1, 3):
        rng = np.random.default_rng(B * 100 + h * 7 + w)
        for N in range(1, 6):
            codes = MEMBERS[:N]
            for off, (dev, host) in enumerate(_members(rng, N, B, h, w, dtype)):      # aligned, then off by one element
                want = K.tta_merge_reference(host, codes)
                got = _accumulate(K, dev, codes, prefill=float("nan"))                 # `first`: the fill is not read
                assert np.array_equal(_bits(got), want.view(np.int32)), (B, N, off)
                if off == 0 and N in (2, 5):
                    assert torch.equal(_accumulate(K, dev, codes, as4d=True), got)      # [B, 1, h, w]; two runs
        dev, host = _members(rng, 4, B, h, w, dtype, exact=True)[0]                    # exact zeros and ones
        got = _accumulate(K, dev, [2, 0, 3, 1])
        assert np.array_equal(_bits(got), K.tta_merge_reference(host, [2, 0, 3, 1]).view(np.int32))
        assert set(np.unique(got.cpu().numpy()).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}


@gpu
def test_tta_accum_unaligned_acc_and_steps(K):
    """An accumulator that is not 16-byte aligned takes the scalar path; without `last` nothing is scaled, and
    `first` with `last` is a scaled copy."""
    rng = np.random.default_rng(4)
    B, h, w = 2, 4, 32
    src = torch.from_numpy(rng.random((B, h, w), dtype=F32)).cuda()
    flat = torch.full((B * h * w + 1,), FILL, device="cuda")
    acc = flat[1:].view(B, h, w)
    K.tta_accum(acc, src, 3, True, False, 0.5)
    assert torch.equal(acc, torch.flip(src, [1, 2])) and flat[0].item() == FILL
    K.tta_accum(acc, src.bfloat16(), 1, False, True, 0.5)
    want = (torch.flip(src, [1, 2]) + torch.flip(src.bfloat16().float(), [2])) * 0.5
    assert torch.equal(acc, want) and flat[0].item() == FILL
    K.tta_accum(acc, src, 0, True, True, 0.25)
    assert torch.equal(acc, src * 0.25)


# ---- host-side contracts: every launcher returns before it touches the device (no GPU needed) ----------------
needs_lib = pytest.mark.skipif(not _lib.LIB_PATH.exists(), reason="HIP library not built")
P = ctypes.c_void_p(0x1000)      # never dereferenced: the host checks return first
i32 = ctypes.c_int
CODES = object()                 # "the codes of this call, as a host array"


def _views(L, B=2, C=3, h=4, w=8, V=2, codes=(0, 1, 0, 0), src=P, table=P, dst=P, pcodes=CODES):
    arr = (i32 * 4)(*codes)
    return L.dpa_tta_views_f32(src, i32(B), i32(C), i32(h), i32(w), table, arr if pcodes is CODES else pcodes, i32(V),
                               dst, None)


def _accum(L, bf16=0, code=1, B=2, h=4, w=8, src=P, acc=P):
    return L.dpa_tta_accum(src, i32(bf16), i32(code), i32(B), i32(h), i32(w), acc, i32(1), i32(1),
                           ctypes.c_float(0.5), None)


def _off(p, by):
    return ctypes.c_void_p((p.value if isinstance(p, ctypes.c_void_p) else int(p)) + by)


VIEWS_BAD = [dict(B=0), dict(B=-1), dict(C=0), dict(C=-1), dict(h=0), dict(h=-1), dict(w=0), dict(w=-1),
             dict(V=0), dict(V=5), dict(codes=(0, -1, 0, 0)), dict(codes=(4, 0, 0, 0)), dict(V=4, codes=(0, 1, 2, 4)),
             dict(src=None), dict(table=None), dict(dst=None), dict(pcodes=None),
             dict(table="odd2"), dict(dst="odd1"), dict(dst="odd2"),
             dict(B=65536, C=1, h=256, w=128), dict(B=2 ** 31 - 1, C=2 ** 31 - 1, h=2 ** 31 - 1, w=2 ** 31 - 1),
             dict(B=2, C=1, h=2 ** 15, w=2 ** 15)]                          # 2^31 elements in a view
ACCUM_BAD = [dict(B=0), dict(B=-1), dict(h=0), dict(h=-1), dict(w=0), dict(w=-1), dict(code=-1), dict(code=4),
             dict(src=None), dict(acc=None), dict(acc="odd2"), dict(acc="odd1"), dict(src="odd2"), dict(src="odd1"),
             dict(bf16=1, src="odd1"), dict(B=32768, h=256, w=256), dict(B=2 ** 31 - 1, h=2 ** 31 - 1, w=2 ** 31 - 1)]


def _resolve(kw, good):
    """"odd1" / "odd2": the good pointer moved by that many bytes, so misaligned for a 4-byte (2-byte) element."""
    out = dict(kw)
    for k, v in kw.items():
        if isinstance(v, str):
            out[k] = _off(good.get(k, P), int(v[3:]))
    return out


@needs_lib
@pytest.mark.parametrize("kw", VIEWS_BAD)
def test_tta_views_launcher_rejects(kw):
    assert _views(_lib.lib(), **_resolve(kw, {})) == INVALID


@needs_lib
@pytest.mark.parametrize("kw", ACCUM_BAD)
def test_tta_accum_launcher_rejects(kw):
    assert _accum(_lib.lib(), **_resolve(kw, {})) == INVALID


@gpu
def test_tta_launchers_reject_without_writing(K):
    """The same bad arguments with real buffers: the return value is 1 and every buffer keeps its fill."""
    L = _lib.lib()
    u8 = torch.full((2, 3, 4, 8), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((2 * 2 * 3 * 4 * 8 + 4,), FILL, device="cuda")
    good = dict(src=_lib.ptr(u8), table=_lib.ptr(K.unit_table("cuda")), dst=_lib.ptr(dst))
    for kw in VIEWS_BAD:
        if max(kw.get(k, 0) for k in "BChw") > 8 or kw.get("V", 0) > 2:
            continue                                            # sizes beyond these buffers: host-only above
        assert _views(L, **{**good, **_resolve(kw, good)}) == INVALID, kw
    src = torch.full((2, 4, 8), 0.5, device="cuda")
    acc = torch.full((2 * 4 * 8 + 4,), FILL, device="cuda")
    good = dict(src=_lib.ptr(src), acc=_lib.ptr(acc))
    for kw in ACCUM_BAD:
        if max(kw.get(k, 0) for k in "Bhw") > 8:
            continue
        assert _accum(L, **{**good, **_resolve(kw, good)}) == INVALID, kw
    torch.cuda.synchronize()
    assert (dst == FILL).all() and (acc == FILL).all() and (u8 == 7).all() and (src == 0.5).all()
    with pytest.raises(AssertionError):                          # the Python wrappers assert before they launch
        K.tta_views(u8.cpu(), [0, 1])
    with pytest.raises(AssertionError):
        K.tta_views(u8, [0, 4])
    with pytest.raises(AssertionError):
        K.tta_views(u8, [0, 1, 2, 3, 0])
    with pytest.raises(AssertionError):
        K.tta_accum(acc[:64].view(2, 4, 8), src.double(), 0, True, True, 1.0)
    with pytest.raises(AssertionError):
        K.tta_accum(acc[:64].view(2, 4, 8), src, 4, True, True, 1.0)
    with pytest.raises(AssertionError):
        K.tta_accum(acc[:60].view(2, 3, 10), src, 0, True, True, 1.0)


# ---- end to end ------------------------------------------------------------------------------------------------
def _model(seed):
    from distributedpytorch_amd.models.unet import build_model
    torch.manual_seed(seed)
    model = build_model("unet")
    with torch.no_grad():                           # a random net's output hugs 0.5: spread it over the threshold
        for p in model.parameters():
            p.mul_(3.0)
    return model


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    imgs, masks = write_tree(tmp_path_factory.mktemp("tta") / "data", n=5)
    files = sorted(str(p) for p in imgs.iterdir())
    return files, [(f, str(masks / (os.path.splitext(os.path.basename(f))[0] + "_mask.gif"))) for f in files]


@gpu
@pytest.mark.parametrize("clean", ["none", "largest+fill"])
def test_predictor_tta_ensemble_equals_host_post(tree, hip_lib, monkeypatch, clean):
    """``hflip+vflip`` x two models, 5 files of two source sizes, batch size 2: masks, run lists and score counts of
    the device path equal those of ``host_post=True`` byte for byte; the merged tensor is ``tta_merge_reference`` of
    the members ``compute.probs`` returned; nothing is finished on the host."""
    from distributedpytorch_amd.predict import Predictor
    files, pairs = tree
    kw = dict(threshold=0.5, clean=clean, tta="hflip+vflip", rle_cap=1000)
    pred = Predictor(_model(3), "cuda:0", (64, 96), extra_models=[_model(5)], **kw)
    host = Predictor(_model(3), "cuda:0", (64, 96), extra_models=[_model(5)], host_post=True, **kw)
    assert pred.strat.compute.name.startswith("hip") and not pred.host_post and host.host_post
    assert pred.members == 6 and pred.tta_codes == [0, 1, 2]

    launches = {"views": 0, "accum": 0}
    real_views, real_accum = KR.tta_views, KR.tta_accum
    monkeypatch.setattr(KR, "tta_views", lambda *a, **k: launches.__setitem__("views", launches["views"] + 1) or real_views(*a, **k))
    monkeypatch.setattr(KR, "tta_accum", lambda *a, **k: launches.__setitem__("accum", launches["accum"] + 1) or real_accum(*a, **k))
    seen, merged = [], []
    for k, strat in enumerate(pred.strats):
        def spy(x, k=k, real=strat.compute.probs):
            p = real(x)
            seen.append((k, p.float().reshape(p.shape[0], p.shape[2], p.shape[3]).cpu().numpy()))
            return p
        strat.compute.probs = spy
    real_merged = pred.merged_probs
    pred.merged_probs = lambda items: merged.append(real_merged(items)) or merged[-1]

    dev = list(pred.predict_files(files, batch_size=2, workers=2))
    ref = list(host.predict_files(files, batch_size=2, workers=2))
    assert pred.host_finished == 0 and host.host_finished == 5
    assert launches == {"views": 3, "accum": 18} and len(seen) == 18 and len(merged) == 3        # 3 batches x 6 members
    for a, b in zip(dev, ref):
        assert a[0] == b[0] and a[1] == b[1] and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    assert {r[1] for r in dev} == {(32, 48), (37, 53)} and max(len(r[3]) for r in dev) >= 1
    for b in range(3):
        part = seen[6 * b:6 * b + 6]
        assert [k for k, _ in part] == [0, 0, 0, 1, 1, 1]
        want = KR.tta_merge_reference([m for _, m in part], [0, 1, 2] * 2)
        assert np.array_equal(_bits(merged[b]), want.view(np.int32)), b
    if clean == "none":
        plain = list(Predictor(_model(3), "cuda:0", (64, 96), threshold=0.5, rle_cap=1000).predict_files(files, 2, 2))
        assert any(a[2].tobytes() != p[2].tobytes() for a, p in zip(dev, plain))     # the average is another answer

    thr = (0.3, 0.5)
    dev = list(pred.run_files(pairs, batch_size=2, workers=2, want_masks=True, want_rle=True, thresholds=thr))
    ref = list(host.run_files(pairs, batch_size=2, workers=2, want_masks=True, want_rle=True, thresholds=thr))
    assert pred.host_finished == 0
    for a, b in zip(dev, ref):
        assert a[0] == b[0] and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
        assert a[4].dtype == np.int64 and a[4].shape == (5,) and a[4].tolist() == b[4].tolist()
    assert any(r[4][1] > 0 for r in dev) and all(r[4][0] > 0 for r in dev)


@gpu
def test_default_predictor_launches_nothing_new(tree, hip_lib, monkeypatch):
    from distributedpytorch_amd.predict import Predictor
    files, _ = tree
    calls = []
    real_views, real_accum = KR.tta_views, KR.tta_accum
    monkeypatch.setattr(KR, "tta_views", lambda *a, **k: calls.append("views") or real_views(*a, **k))
    monkeypatch.setattr(KR, "tta_accum", lambda *a, **k: calls.append("accum") or real_accum(*a, **k))
    pred = Predictor(_model(3), "cuda:0", (64, 96), tta="none", extra_models=())
    probs = []
    real = pred.probs
    pred.probs = lambda x: probs.append(1) or real(x)
    recs = list(pred.predict_files(files, batch_size=2, workers=2))
    assert len(recs) == 5 and calls == [] and len(probs) == 3 and pred.members == 1
    # the wrappers above do count: one view launch and two accumulations for a batch under hflip
    flip = Predictor(_model(3), "cuda:0", (64, 96), tta="hflip")
    list(flip.predict_files(files[:2], batch_size=2, workers=1))
    assert calls == ["views", "accum", "accum"]
