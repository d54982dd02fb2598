"""csrc/data_prep.hip and the resident folder dataset on the GPU: the bicubic / nearest resize kernels against
PIL (bit for bit), the batch kernel against ``index_select`` + the host conversion, the dataset and its loader
against the host ``CarvanaDataset`` path, the launchers' argument checks, and ``train.py --device-folder-data``
against ``train.py`` without it (same loss curve, bit for bit)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedpytorch_amd.ops import _lib

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

from test_device_folder_cpu import write_tree  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # hipErrorInvalidValue
gpu = pytest.mark.gpu

# (Hs, Ws) -> (Ho, Wo)
SHAPES = [((37, 53), (16, 24)),         # non-integer down-scale, ragged tiles
          ((50, 70), (64, 96)),         # up-scale
          ((20, 31), (48, 16)),         # up on one axis, down on the other
          ((32, 48), (32, 24)),         # vertical pass skipped
          ((64, 96), (64, 96)),         # identity
          ((600, 40), (8, 40)),         # 75x down: hundreds of source rows per output row
          ((1280, 1918), (640, 960))]   # the real ratio: many tiles, the tile-height choice


@pytest.fixture(scope="module")
def K(hip_lib):
    from distributedpytorch_amd.ops import kernels
    return kernels


def _pil_bicubic(a, ho, wo):
    r = np.array(Image.fromarray(a).resize((wo, ho), resample=Image.BICUBIC))
    return np.ascontiguousarray(r[None] if r.ndim == 2 else r.transpose(2, 0, 1))


def _gpu_bicubic(K, a, ho, wo):
    src = torch.from_numpy(a if a.ndim == 3 else a[:, :, None]).cuda()
    dst = torch.full((src.shape[2], ho, wo), 77, dtype=torch.uint8, device="cuda")
    ok = K.resize_bicubic_u8(src, dst)
    torch.cuda.synchronize()
    return ok, dst.cpu().numpy()


@gpu
@pytest.mark.parametrize("src,dst", SHAPES)
def test_resize_bicubic_equals_pil(K, src, dst):
    a = np.random.default_rng(src[0] + dst[1]).integers(0, 256, size=src + (3,), dtype=np.uint8)
    ok, got = _gpu_bicubic(K, a, *dst)
    ref = _pil_bicubic(a, *dst)
    if not ok:       # the launcher may refuse an extreme down-scale; then nothing ran and the CPU path serves
        assert src == (600, 40) and (got == 77).all()
        got = ref
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(ref))


@gpu
@pytest.mark.parametrize("src,dst", SHAPES[:3])
def test_resize_bicubic_grey_equals_pil(K, src, dst):
    a = np.random.default_rng(5).integers(0, 256, size=src, dtype=np.uint8)
    ok, got = _gpu_bicubic(K, a, *dst)
    assert ok and torch.equal(torch.from_numpy(got), torch.from_numpy(_pil_bicubic(a, *dst)))


@gpu
def test_resize_bicubic_refuses_when_no_tile_fits(K):
    """3000 -> 4 rows: one output row reads every source row; 3000 rows x 16 columns x 3 channels of LDS do not
    exist.  The launcher returns invalid-argument without launching (the destination keeps its fill)."""
    ok, got = _gpu_bicubic(K, np.zeros((3000, 8, 3), np.uint8), 4, 8)
    assert not ok and (got == 77).all()


@gpu
@pytest.mark.parametrize("src,dst", SHAPES)
def test_resize_nearest_equals_pil(K, src, dst):
    m = np.random.default_rng(src[1]).integers(0, 256, size=src, dtype=np.uint8)
    out = torch.empty(dst, dtype=torch.uint8, device="cuda")
    K.resize_nearest_u8(torch.from_numpy(m).cuda(), out, mask_rule=False)
    ref = np.array(Image.fromarray(m).resize((dst[1], dst[0]), resample=Image.NEAREST))
    assert torch.equal(out.cpu(), torch.from_numpy(ref))


@gpu
def test_mask_rule_on_device(K):
    from distributedpytorch_amd.data import BasicDataset
    rng = np.random.default_rng(3)
    box = (rng.integers(0, 2, size=(37, 53)) * 255).astype(np.uint8)
    grey = rng.integers(0, 256, size=(37, 53), dtype=np.uint8)            # any maximum > 1: value > 127
    for m in (box, box // 255, np.zeros((37, 53), np.uint8), grey):
        out = torch.empty(16, 24, dtype=torch.uint8, device="cuda")
        K.resize_nearest_u8(torch.from_numpy(m).cuda(), out)
        ref = BasicDataset.preprocess(Image.fromarray(m), (24, 16), is_mask=True)
        assert torch.equal(out.cpu().long(), torch.from_numpy(np.array(ref)).long())
        assert out.max().item() <= 1


@gpu
@pytest.mark.parametrize("W", [16, 24, 50, 64])
@pytest.mark.parametrize("flips", [False, True])
def test_batch_gather_equals_index_select(K, W, flips):
    g = torch.Generator().manual_seed(W)
    N, C, H = 5, 3, 7
    images = torch.randint(0, 256, (N, C, H, W), dtype=torch.uint8, generator=g)
    masks = torch.randint(0, 2, (N, H, W), dtype=torch.uint8, generator=g)
    idx = torch.tensor([4, 0, 0, 3, 1, 4, 2])                              # repeated, out of order
    flip = torch.tensor([1, 0, 1, 1, 0, 0, 1], dtype=torch.uint8) if flips else None
    img, tgt = K.batch_gather_u8(images.cuda(), masks.cuda(), idx.cuda(), None if flip is None else flip.cuda())
    ref_img = torch.as_tensor(images.index_select(0, idx).numpy() / 255.0).float()
    ref_tgt = masks.index_select(0, idx).long().to(torch.float32).unsqueeze(1)
    if flips:
        f = flip.bool().view(-1, 1, 1, 1)
        ref_img = torch.where(f, ref_img.flip(-1), ref_img)
        ref_tgt = torch.where(f, ref_tgt.flip(-1), ref_tgt)
    assert img.dtype == tgt.dtype == torch.float32 and tuple(tgt.shape) == (7, 1, H, W)
    assert torch.equal(img.cpu(), ref_img) and torch.equal(tgt.cpu(), ref_tgt)


@gpu
@pytest.mark.parametrize("W", [16, 10])          # the 16-byte path and the scalar path
def test_batch_gather_all_byte_values(K, W):
    k = np.arange(256, dtype=np.uint8)
    rows = -(-256 // W)
    images = torch.from_numpy(np.resize(k, (1, 1, rows, W)).copy())
    assert set(images.flatten().tolist()) == set(range(256))
    masks = torch.zeros(1, rows, W, dtype=torch.uint8)
    img, _ = K.batch_gather_u8(images.cuda(), masks.cuda(), torch.zeros(1, dtype=torch.int64).cuda())
    assert torch.equal(img.cpu(), torch.as_tensor(images.numpy() / 255.0).float())


@pytest.fixture(scope="module")
def tree(tmp_path_factory, hip_lib):
    from distributedpytorch_amd.data import CarvanaDataset, DeviceFolderDataset
    imgs, masks = write_tree(tmp_path_factory.mktemp("carvana"))
    host = CarvanaDataset(imgs, masks, newsize=(24, 16))
    dev = DeviceFolderDataset(imgs, masks, newsize=(24, 16), mask_suffix="_mask", device="cuda", workers=2)
    return host, dev


@gpu
def test_dataset_items_equal_host(tree):
    host, dev = tree
    assert dev.images.is_cuda and dev.cpu_resized == 0              # every file went through the kernels
    for i in range(len(host)):
        a, b = dev[i], host[i]
        assert torch.equal(a["image"].cpu(), b["image"]) and torch.equal(a["mask"].cpu(), b["mask"])


@gpu
def test_dataset_batches_equal_host(tree):
    from distributedpytorch_amd.data import DeviceBatcher, build_loaders, device_folder_loaders, split_dataset
    host, dev = tree
    ht, hv = split_dataset(host, 30, seed=0)
    dt, dv = split_dataset(dev, 30, seed=0)
    dl, dvl, ds = device_folder_loaders(dt, dv, 2, seed=3)
    hl, hvl, hs = build_loaders(ht, hv, 2, seed=3)
    ds.set_epoch(1)
    hs.set_epoch(1)
    for d, h in ((dl, hl), (dvl, hvl)):
        a, b = list(d), list(DeviceBatcher(h, torch.device("cpu")))
        assert len(a) == len(b) > 0
        for (xi, xt), (yi, yt) in zip(a, b):
            assert xi.is_cuda and torch.equal(xi.cpu(), yi) and torch.equal(xt.cpu(), yt)
    # hflip on the device = the plain batch mirrored where the flag is set
    aug, _, s = device_folder_loaders(dt, dv, 2, seed=3, augment="hflip")
    s.set_epoch(1)
    flipped = 0
    for (pi, pt), (ai, at) in zip(dl, aug):
        f = torch.from_numpy(aug.last_flags).bool().view(-1, 1, 1, 1).cuda()
        flipped += int(f.sum())
        assert torch.equal(ai, torch.where(f, pi.flip(-1), pi)) and torch.equal(at, torch.where(f, pt.flip(-1), pt))
    assert flipped > 0


@gpu
def test_dataset_cpu_fallback_for_a_refused_source(tmp_path, hip_lib):
    """A 3000-row strip resized to 4 rows is refused by the launcher: that file goes through PIL on the CPU and
    the item still equals the host path's."""
    from distributedpytorch_amd.data import CarvanaDataset, DeviceFolderDataset
    imgs, masks = tmp_path / "train_hq", tmp_path / "train_masks"
    imgs.mkdir()
    masks.mkdir()
    rng = np.random.default_rng(1)
    Image.fromarray(rng.integers(0, 256, size=(3000, 8, 3), dtype=np.uint8)).save(imgs / "strip.jpg", quality=95)
    Image.fromarray((rng.integers(0, 2, size=(3000, 8)) * 255).astype(np.uint8)).save(masks / "strip_mask.gif")
    host = CarvanaDataset(imgs, masks, newsize=(8, 4))
    dev = DeviceFolderDataset(imgs, masks, newsize=(8, 4), mask_suffix="_mask", device="cuda")
    assert dev.cpu_resized == 1                                     # the image; the mask kernel has no such limit
    assert torch.equal(dev[0]["image"].cpu(), host[0]["image"]) and torch.equal(dev[0]["mask"].cpu(), host[0]["mask"])


# ---- host-side contracts: every launcher returns before it touches the device (no GPU needed) ----------------
needs_lib = pytest.mark.skipif(not _lib.LIB_PATH.exists(), reason="HIP library not built")
P = ctypes.c_void_p(0x1000)      # never dereferenced: the host checks return first
i32 = ctypes.c_int


def _bicubic(L, Hs=37, Ws=53, C=3, Ho=16, Wo=24, kh=11, kv=11, src=P, hc=P):
    return L.dpa_resize_bicubic_u8(src, i32(Hs), i32(Ws), i32(C), P, i32(Ho), i32(Wo), P, hc, i32(kh), P, P, i32(kv), None)


@needs_lib
@pytest.mark.parametrize("kw", [dict(Hs=0), dict(Ws=-1), dict(Ho=0), dict(Wo=-5), dict(C=2), dict(C=4), dict(C=0),
                                dict(kh=9), dict(kv=5), dict(kh=1), dict(src=None), dict(hc=None),
                                dict(Hs=3000, Ho=4, kv=3001)])
def test_bicubic_launcher_rejects(kw):
    """53 -> 24 and 37 -> 16 both need ksize 2 * ceil(2 * in / out) + 1 = 11; any other width is a table built for
    other sizes.  The last case has matching tables and no tile that fits."""
    assert _bicubic(_lib.lib(), **kw) == INVALID


@needs_lib
def test_bicubic_launcher_ksize_of_a_skipped_pass():
    L = _lib.lib()
    assert _bicubic(L, Hs=32, Ws=48, Ho=32, Wo=24, kh=9, kv=9) == INVALID      # equal heights: identity table, 1
    assert _bicubic(L, Hs=32, Ws=48, Ho=32, Wo=24, kh=1, kv=1) == INVALID      # 48 -> 24 needs 9


@needs_lib
@pytest.mark.parametrize("kw", [dict(Hs=0), dict(Ws=0), dict(Ho=-1), dict(Wo=0), dict(src=None), dict(vmax=None)])
def test_nearest_launcher_rejects(kw):
    a = dict(src=P, Hs=37, Ws=53, Ho=16, Wo=24, vmax=P)
    a.update(kw)
    assert _lib.lib().dpa_resize_nearest_u8(a["src"], i32(a["Hs"]), i32(a["Ws"]), P, i32(a["Ho"]), i32(a["Wo"]), P, P,
                                            a["vmax"], i32(1), None) == INVALID


@needs_lib
@pytest.mark.parametrize("kw", [dict(N=0), dict(B=0), dict(C=0), dict(H=-1), dict(W=0), dict(idx=None), dict(lut=None)])
def test_gather_launcher_rejects(kw):
    a = dict(N=4, B=2, C=3, H=8, W=16, idx=P, lut=P)
    a.update(kw)
    assert _lib.lib().dpa_batch_gather_u8(P, P, a["idx"], None, a["lut"], P, P, ctypes.c_longlong(a["N"]), i32(a["B"]),
                                          i32(a["C"]), i32(a["H"]), i32(a["W"]), None) == INVALID


@needs_lib
def test_python_wrappers_assert_before_launch():
    from distributedpytorch_amd.ops import kernels
    with pytest.raises(AssertionError):                              # not on the device
        kernels.resize_bicubic_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(3, 2, 2, dtype=torch.uint8))
    with pytest.raises(AssertionError):
        kernels.batch_gather_u8(torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(1).long())


# ---- end to end ------------------------------------------------------------------------------------------------
@gpu
def test_train_py_same_loss_curve_with_the_flag(tmp_path, hip_lib):
    import pandas as pd
    write_tree(tmp_path / "data", n=13)

    def run(name, *extra):
        out = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--data-dir", str(tmp_path / "data"), "--img-size", "128",
               "-b", "4", "-e", "1", "--log-every", "1", "--out-dir", str(out), *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return pd.read_pickle(out / "loss" / "singleGPU" / "train_loss.pkl")["Loss"].to_numpy(), \
            (out / "logs" / "singleGPU.log").read_text()

    host, host_log = run("host")
    res, res_log = run("resident", "--device-folder-data")
    assert len(host) == len(res) == 3 and np.isfinite(host).all()      # 12 training images / batch 4
    assert host.tobytes() == res.tobytes(), (host, res)
    assert "backend=hip" in res_log and "folder dataset resident on cuda" in res_log
    assert "folder dataset resident" not in host_log
