"""csrc/augment.hip on the GPU: ``dpa_batch_augment_u8`` against ``augment_reference`` bit for bit (every matrix
family, with and without tone tables, both store forms, ragged row tails, views that are not 16-byte aligned),
against the plain batch kernel for the identity and the flip, the GPU-resident loader against the CPU-resident
one, the launcher's and the wrapper's argument checks, and ``train.py --augment`` twice (same losses)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributedpytorch_amd.data.augment import AugmentSpec, affine_matrices, augment_reference, inverse_affine, to_q16
from distributedpytorch_amd.ops import _lib

PIL = pytest.importorskip("PIL")

from test_augment_cpu import I32, Q, flip_mat, identity_mat, make_data, shift_mat  # noqa: E402
from test_device_folder_cpu import write_tree  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # hipErrorInvalidValue
gpu = pytest.mark.gpu

# (H, W, C): W = 7 (scalar stores, ragged 4-pixel groups), 24 and 40 (16-byte stores, a tile's ragged right edge),
# 48 and 96; H = 5 .. 64 (a ragged last tile row, more than one tile row)
SHAPES = [(16, 24, 3), (32, 48, 3), (8, 40, 1), (5, 7, 3), (64, 96, 3)]
B = 5
IDX = [2, 0, 2, 1, 3]                                                  # N = 4; one index twice


@pytest.fixture(scope="module")
def K(hip_lib):
    from distributedpytorch_amd.ops import kernels
    return kernels


def matrix_families(H, W):
    """name -> int32 [B, 6]"""
    fam = {"identity": [identity_mat()] * B, "flip": [flip_mat(W)] * B, "shift": [shift_mat(3, -2)] * B,
           "extreme": [[I32.max] * 6, [I32.min] * 6, [I32.max] * 6, [I32.min] * 6, [I32.max, I32.min] * 3]}
    one = np.ones(B)
    if H != W:                 # a quarter turn of a non-square image: much of the output maps outside
        fam["rot90"] = to_q16(inverse_affine(one, np.deg2rad(90.0) * one, 0 * one, 0 * one, one, H, W)).tolist()
    fam["zoom0.5"] = to_q16(inverse_affine(0.5 * one, 0 * one, 0 * one, 0 * one, one, H, W)).tolist()
    fam["zoom3"] = to_q16(inverse_affine(3 * one, 0 * one, 0 * one, 0 * one, one, H, W)).tolist()
    triple = AugmentSpec.parse("hflip+affine", scale=0.75, rotate=30.0, shift=0.3)
    drawn = affine_matrices(triple, 11, 2, np.arange(8), H, W)
    fam["drawn-a"], fam["drawn-b"] = drawn[:B].tolist(), drawn[3:].tolist()      # the eight, in two batches
    return {k: torch.tensor(v, dtype=torch.int32) for k, v in fam.items()}


_REF = {}


def reference(H, W, C):
    """Inputs and CPU results of one shape, computed once and shared: {(family, with luts): (img, tgt)}."""
    key = (H, W, C)
    if key not in _REF:
        images, masks = make_data(H, W, C, N=4)
        idx = torch.tensor(IDX)
        luts = torch.rand(B, 256, generator=torch.Generator().manual_seed(H * W))
        fams = matrix_families(H, W)
        out = {(name, use): augment_reference(images, masks, idx, m, luts if use else None)
               for name, m in fams.items() for use in (False, True)}
        _REF[key] = (images, masks, idx, luts, fams, out)
    return _REF[key]


def _unaligned(t):
    """A contiguous cuda copy of ``t`` whose base address is 4 (float32) or 1 (uint8) bytes past 16-byte alignment."""
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
    off = (16 - flat.data_ptr() % 16) % 16 // t.element_size() + 1
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@gpu
@pytest.mark.parametrize("H,W,C", SHAPES)
def test_kernel_equals_reference(K, H, W, C):
    images, masks, idx, luts, fams, ref = reference(H, W, C)
    gi, gm, gidx, gl = images.cuda(), masks.cuda(), idx.cuda(), luts.cuda()
    for name, m in fams.items():
        for use in (False, True):
            img, tgt = K.batch_augment_u8(gi, gm, gidx, m.cuda(), gl if use else None)
            ri, rt = ref[(name, use)]
            assert img.dtype == tgt.dtype == torch.float32 and tuple(tgt.shape) == (B, 1, H, W)
            assert torch.equal(img.cpu(), ri), (name, use, "image")
            assert torch.equal(tgt.cpu(), rt), (name, use, "target")
    # a short last batch: two items of the same set
    img, tgt = K.batch_augment_u8(gi, gm, gidx[:2].contiguous(), fams["drawn-a"][:2].contiguous().cuda(),
                                  gl[:2].contiguous())
    ri, rt = ref[("drawn-a", True)]
    assert torch.equal(img.cpu(), ri[:2]) and torch.equal(tgt.cpu(), rt[:2])


@gpu
@pytest.mark.parametrize("H,W,C", SHAPES)
def test_kernel_on_unaligned_views(K, H, W, C):
    """Sources and outputs off 16-byte alignment: the launcher takes the scalar store form, the result is the same."""
    images, masks, idx, luts, fams, ref = reference(H, W, C)
    gi, gm = _unaligned(images.cuda()), _unaligned(masks.cuda())
    oi = _unaligned(torch.zeros(B, C, H, W, device="cuda"))
    ot = _unaligned(torch.zeros(B, 1, H, W, device="cuda"))
    for name in fams:
        for use in (False, True):
            oi.fill_(-1), ot.fill_(-1)
            img, tgt = K.batch_augment_u8(gi, gm, idx.cuda(), fams[name].cuda(), luts.cuda() if use else None,
                                          out=(oi, ot))
            assert img is oi and tgt is ot
            ri, rt = ref[(name, use)]
            assert torch.equal(oi.cpu(), ri) and torch.equal(ot.cpu(), rt), (name, use)
    # aligned outputs, unaligned sources: the 16-byte store form reads bytes from anywhere
    img, tgt = K.batch_augment_u8(gi, gm, idx.cuda(), fams["drawn-b"].cuda())
    ri, rt = ref[("drawn-b", False)]
    assert torch.equal(img.cpu(), ri) and torch.equal(tgt.cpu(), rt)


@gpu
@pytest.mark.parametrize("H,W,C", SHAPES)
def test_identity_and_flip_equal_the_plain_kernel(K, H, W, C):
    images, masks, idx, _, fams, _ = reference(H, W, C)
    gi, gm, gidx = images.cuda(), masks.cuda(), idx.cuda()
    pi, pt = K.batch_gather_u8(gi, gm, gidx, None)
    img, tgt = K.batch_augment_u8(gi, gm, gidx, fams["identity"].cuda())
    assert torch.equal(img, pi) and torch.equal(tgt, pt)
    fi, ft = K.batch_gather_u8(gi, gm, gidx, torch.ones(B, dtype=torch.uint8, device="cuda"))
    img, tgt = K.batch_augment_u8(gi, gm, gidx, fams["flip"].cuda())
    assert torch.equal(img, fi) and torch.equal(tgt, ft)


@gpu
def test_gpu_loader_equals_cpu_loader(tmp_path, hip_lib):
    from distributedpytorch_amd.data import DeviceFolderDataset, device_folder_loaders
    imgs, masks = write_tree(tmp_path / "carvana")
    sets = [DeviceFolderDataset(imgs, masks, newsize=(24, 16), mask_suffix="_mask", device=d, workers=2)
            for d in ("cuda", "cpu")]
    assert torch.equal(sets[0].images.cpu(), sets[1].images)
    (gl, gv, gs), (cl, cv, cs) = [device_folder_loaders(d, d, 3, seed=4, augment="hflip+affine+color") for d in sets]
    assert gv.augment == cv.augment == "none"
    for epoch in (0, 1):
        gs.set_epoch(epoch)
        cs.set_epoch(epoch)
        n = 0
        for (gi, gt), (ci, ct) in zip(gl, cl):
            assert gi.is_cuda and torch.equal(gi.cpu(), ci) and torch.equal(gt.cpu(), ct)
            assert torch.equal(gl.last_params[0], cl.last_params[0]) and torch.equal(gl.last_params[1], cl.last_params[1])
            n += 1
        assert n == 3


# ---- host-side contracts: the launcher returns before it touches the device (no GPU needed) ------------------
needs_lib = pytest.mark.skipif(not _lib.LIB_PATH.exists(), reason="HIP library not built")
P = ctypes.c_void_p(0x1000)      # never dereferenced: the host checks return first
i32 = ctypes.c_int


@needs_lib
@pytest.mark.parametrize("kw", [dict(N=0), dict(B=0), dict(B=-2), dict(C=0), dict(H=-1), dict(H=0), dict(W=0),
                                dict(H=32768), dict(W=40000), dict(idx=None), dict(mats=None), dict(unit=None),
                                dict(images=None), dict(img=None)])
def test_augment_launcher_rejects(kw):
    a = dict(N=4, B=2, C=3, H=8, W=16, images=P, idx=P, mats=P, unit=P, img=P)
    a.update(kw)
    assert _lib.lib().dpa_batch_augment_u8(a["images"], P, a["idx"], a["mats"], None, a["unit"], a["img"], P,
                                           ctypes.c_longlong(a["N"]), i32(a["B"]), i32(a["C"]), i32(a["H"]),
                                           i32(a["W"]), None) == INVALID


@needs_lib
def test_python_wrapper_asserts_before_launch():
    from distributedpytorch_amd.ops import kernels
    images, masks = make_data(8, 16, 3)
    idx = torch.tensor([0, 1])
    mats = torch.tensor([identity_mat()] * 2, dtype=torch.int32)
    with pytest.raises(AssertionError):                              # not on the device
        kernels.batch_augment_u8(images, masks, idx, mats)


def _refused(K, why, *args, **kw):
    try:
        K.batch_augment_u8(*args, **kw)
    except AssertionError:
        return
    pytest.fail(f"batch_augment_u8 accepted {why}")


@gpu
def test_python_wrapper_asserts_on_device_arguments(K):
    """``mats``, ``luts`` and ``out`` of the wrong shape, dtype, device or layout, beside good device tensors: the
    wrapper's assertions are all that keeps the kernel from reading a short ``mats`` or ``luts`` past its end."""
    images, masks = make_data(8, 16, 3)
    gi, gm, gidx = images.cuda(), masks.cuda(), torch.tensor([0, 1]).cuda()
    mats = torch.tensor([identity_mat()] * 2, dtype=torch.int32)
    gmats = mats.cuda()
    good_luts = torch.rand(2, 256, device="cuda")
    bad_mats = {"[B,5]": gmats[:, :5].contiguous(), "[B-1,6]": gmats[:1], "[B+1,6]": torch.cat([gmats, gmats[:1]]),
                "flat": gmats.view(-1), "int64": gmats.long(), "float32": gmats.float(), "on the host": mats,
                "not contiguous": torch.cat([gmats, gmats], 1)[:, :6]}
    assert not bad_mats["not contiguous"].is_contiguous()
    for why, bad in bad_mats.items():
        _refused(K, f"mats {why}", gi, gm, gidx, bad)
    bad_luts = {"[B+1,256]": torch.zeros(3, 256, device="cuda"), "[B-1,256]": torch.zeros(1, 256, device="cuda"),
                "[B,255]": torch.zeros(2, 255, device="cuda"), "[256]": torch.zeros(256, device="cuda"),
                "float64": torch.zeros(2, 256, device="cuda", dtype=torch.float64), "on the host": torch.zeros(2, 256),
                "not contiguous": torch.zeros(2, 512, device="cuda")[:, ::2]}
    for why, bad in bad_luts.items():
        _refused(K, f"luts {why}", gi, gm, gidx, gmats, bad)
    oi, ot = torch.zeros(2, 3, 8, 16, device="cuda"), torch.zeros(2, 1, 8, 16, device="cuda")
    bad_out = {"target width": (oi, torch.zeros(2, 1, 8, 15, device="cuda")), "image batch": (oi[:1], ot),
               "float16": (oi.half(), ot), "on the host": (oi.cpu(), ot),
               "not contiguous": (torch.zeros(2, 3, 8, 32, device="cuda")[..., ::2], ot)}
    for why, bad in bad_out.items():
        _refused(K, f"out {why}", gi, gm, gidx, gmats, good_luts, out=bad)
    # and the good call beside them goes through, into the tensors given
    img, tgt = K.batch_augment_u8(gi, gm, gidx, gmats, good_luts, out=(oi, ot))
    assert img is oi and tgt is ot and torch.equal(tgt.cpu()[:, 0], masks[:2].float())


# ---- end to end ------------------------------------------------------------------------------------------------
@gpu
def test_train_py_augmented_twice_same_losses(tmp_path, hip_lib):
    """The engine is bitwise deterministic and the augmentation a pure function: two runs write the same losses,
    byte for byte (the Loss column of the loss pickle; its Time column is the wall clock)."""
    import pandas as pd
    write_tree(tmp_path / "data", n=13)

    def run(name):
        out = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--data-dir", str(tmp_path / "data"), "--img-size", "128",
               "-b", "4", "-e", "1", "--log-every", "1", "--out-dir", str(out), "--device-folder-data",
               "--augment", "hflip+affine+color"]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return pd.read_pickle(out / "loss" / "singleGPU" / "train_loss.pkl")["Loss"].to_numpy(), \
            (out / "logs" / "singleGPU.log").read_text()

    a, log_a = run("a")
    b, _ = run("b")
    assert len(a) == len(b) == 3 and np.isfinite(a).all()              # 12 training images / batch 4
    assert a.tobytes() == b.tobytes(), (a, b)
    assert "backend=hip" in log_a and "augment: hflip+affine+color scale=0.25" in log_a
