"""Training augmentation (data/augment.py) without a GPU: the integer warp arithmetic of ``augment_reference``
(exactness for identity, flip and integer shifts, any int32 matrix stays in bounds, the pixel-centre convention
against a float64 bilinear), the hashes behind the draws, the matrices and tone tables, the loader of a dataset
resident on the CPU, the command-line flags and one CPU epoch of training."""
import numpy as np
import pytest
import torch

from distributedpytorch_amd.data import DeviceFolderDataset, device_folder_loaders
from distributedpytorch_amd.data.augment import (AugmentSpec, aug_uniform, affine_matrices, augment_reference,
                                                 color_luts, inverse_affine, to_q16)
from distributedpytorch_amd.data.device_folder import flip_flags
from distributedpytorch_amd.ops import kernels as K

PIL = pytest.importorskip("PIL")

from test_device_folder_cpu import write_tree  # noqa: E402

Q = 1 << 16
I32 = np.iinfo(np.int32)
SHAPES = [(16, 24, 3), (32, 48, 3), (8, 40, 1), (5, 7, 3)]          # (H, W, C)
ZERO = dict(scale=0, rotate=0, shift=0, brightness=0, contrast=0, gamma=0)


def make_data(H, W, C, N=3, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    images = torch.randint(0, 256, (N, C, H, W), dtype=torch.uint8, generator=g)
    masks = torch.randint(0, 2, (N, H, W), dtype=torch.uint8, generator=g) * 255
    return images, masks


def identity_mat():
    return [Q, 0, 0, 0, Q, 0]


def flip_mat(W):
    return [-Q, 0, (W - 1) << 16, 0, Q, 0]


def shift_mat(dx, dy):
    return [Q, 0, dx * Q, 0, Q, dy * Q]


def mats_of(rows, B):
    return torch.tensor([rows[k % len(rows)] for k in range(B)], dtype=torch.int32)


def plain_batch(images, masks, idx):
    img = K.unit_table("cpu")[images.index_select(0, idx).long()]
    return img, masks.index_select(0, idx).to(torch.float32).unsqueeze(1)


# ---- the reference arithmetic -----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C", SHAPES)
def test_identity_flip_and_integer_shift_are_exact(H, W, C):
    images, masks = make_data(H, W, C)
    idx = torch.tensor([2, 0, 2, 1])                                   # B = 4, one index twice
    pi, pt = plain_batch(images, masks, idx)
    img, tgt = augment_reference(images, masks, idx, mats_of([identity_mat()], 4))
    assert img.dtype == tgt.dtype == torch.float32 and tuple(tgt.shape) == (4, 1, H, W)
    assert torch.equal(img, pi) and torch.equal(tgt, pt)
    img, tgt = augment_reference(images, masks, idx, mats_of([flip_mat(W)], 4))
    assert torch.equal(img, pi.flip(-1)) and torch.equal(tgt, pt.flip(-1))
    for dx, dy in ((3, -2), (-1, 4), (W + 5, 0)):                      # the last: every column is the right rim
        xs = (torch.arange(W) + dx).clamp(0, W - 1)
        ys = (torch.arange(H) + dy).clamp(0, H - 1)
        img, tgt = augment_reference(images, masks, idx, mats_of([shift_mat(dx, dy)], 4))
        assert torch.equal(img, pi[:, :, ys][:, :, :, xs]) and torch.equal(tgt, pt[:, :, ys][:, :, :, xs])


@pytest.mark.parametrize("H,W,C", SHAPES)
def test_extreme_matrices_stay_inside_the_planes(H, W, C):
    images, masks = make_data(H, W, C)
    masks = masks // 255 * 7 + 3                                       # values {3, 10}: not the fill of anything
    idx = torch.tensor([2, 0, 2, 1])
    luts = torch.rand(4, 256, generator=torch.Generator().manual_seed(1))
    mats = mats_of([[I32.max] * 6, [I32.min] * 6], 4)
    for lut in (None, luts):
        img, tgt = augment_reference(images, masks, idx, mats, lut)
        assert set(tgt.unique().tolist()) <= {3.0, 10.0}
        for b in range(4):
            table = K.unit_table("cpu") if lut is None else lut[b]
            assert torch.isin(img[b], table).all()


def test_pixel_centre_convention_against_float_bilinear():
    """Zoom 1.2, 17 degrees, shift (2.3, -1.7) of a smooth 64 x 96 image, against a float64 bilinear of the same
    inverse map (unquantised matrix, clamp-to-edge).  The bound is derived: 0.5 for the final rounding plus the
    image's largest neighbouring-pixel difference G times the coordinate error, 1/256 per axis for the truncated
    fraction and (W + H) 2^-17 per axis for the Q16 rounding of the matrix.  A half-pixel convention error moves
    the sample by 0.5 px, several times that."""
    H, W = 64, 96
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.rint((np.sin(xx / 9.0) + np.cos(yy / 7.0)) * 60 + 128).astype(np.uint8)
    m = inverse_affine(1.2, np.deg2rad(17.0), 2.3, -1.7, 1.0, H, W)
    ident = torch.arange(256, dtype=torch.float32).view(1, 256)                        # img = v itself
    img, _ = augment_reference(torch.from_numpy(a).view(1, 1, H, W), torch.zeros(1, H, W, dtype=torch.uint8),
                               torch.zeros(1, dtype=torch.int64), torch.from_numpy(to_q16(m)), ident)
    sx = m[0, 0] * xx + m[0, 1] * yy + m[0, 2]
    sy = m[0, 3] * xx + m[0, 4] * yy + m[0, 5]
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    f = a.astype(np.float64)

    def tap(yi, xi):
        return f[np.clip(yi, 0, H - 1).astype(int), np.clip(xi, 0, W - 1).astype(int)]

    ref = (1 - fx) * (1 - fy) * tap(y0, x0) + fx * (1 - fy) * tap(y0, x0 + 1) + (1 - fx) * fy * tap(y0 + 1, x0) \
        + fx * fy * tap(y0 + 1, x0 + 1)
    G = max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max())
    bound = 0.5 + G * (2 / 256 + 2 * (W + H) * 2.0 ** -17)
    err = np.abs(img[0, 0].numpy().astype(np.float64) - ref).max()
    print(f"max error {err:.4f} grey levels, bound {bound:.4f} (G = {G:.0f})")
    assert err <= bound
    half = ref - tap(np.floor(sy + 0.5), np.floor(sx + 0.5))           # what a half-pixel slip looks like
    assert np.abs(half).max() > 3 * bound


# ---- hashes, matrices, tables -----------------------------------------------------------------------------------
def test_aug_uniform_is_a_pure_per_item_hash():
    idx = np.arange(4096)
    streams = [aug_uniform(42, 3, idx, s) for s in range(1, 8)]
    for u in streams:
        assert u.dtype == np.float64 and u.shape == (4096,) and (u >= 0).all() and (u < 1).all()
        assert abs(u.mean() - 0.5) < 0.05
    for a in range(7):
        assert np.array_equal(streams[a], aug_uniform(42, 3, idx, a + 1))
        assert np.array_equal(streams[a][::-1], aug_uniform(42, 3, idx[::-1], a + 1))
        for b in range(a + 1, 7):
            assert not np.array_equal(streams[a], streams[b])
    assert not np.array_equal(streams[0], aug_uniform(42, 4, idx, 1))
    assert not np.array_equal(streams[0], aug_uniform(43, 3, idx, 1))


def test_flip_flags_are_unchanged():
    """Literal values from before the augmentation module existed."""
    assert flip_flags(0, 0, np.arange(16)).tolist() == [0, 0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1]
    assert flip_flags(42, 1, np.arange(16)).tolist() == [0, 0, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 1]
    assert flip_flags(7, 13, np.arange(16)).tolist() == [0, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 0, 1]
    assert flip_flags(42, 0, np.array([5087, 1000000, 2 ** 31 - 1])).tolist() == [1, 0, 0]


def test_zero_magnitudes_are_identity_and_unit_table():
    spec = AugmentSpec.parse("affine+color", **ZERO)
    idx = np.arange(9)
    for H, W in ((16, 24), (5, 7), (640, 960)):
        assert np.array_equal(affine_matrices(spec, 1, 2, idx, H, W), np.tile(identity_mat(), (9, 1)))
    luts = color_luts(spec, 1, 2, idx)
    assert luts.dtype == np.float32 and luts.shape == (9, 256)
    assert all(np.array_equal(row, K.unit_table("cpu").numpy()) for row in luts)
    assert color_luts(AugmentSpec.parse("hflip+affine"), 1, 2, idx) is None
    # hflip alone in the matrix: the identity or the exact flip matrix, by flip_flags
    m = affine_matrices(AugmentSpec.parse("hflip+color"), 1, 2, idx, 16, 24)
    want = [flip_mat(24) if f else identity_mat() for f in flip_flags(1, 2, idx)]
    assert m.dtype == np.int32 and np.array_equal(m, np.array(want))


def test_default_matrices_and_tables_are_in_range():
    spec = AugmentSpec.parse("hflip+affine+color")
    idx = np.arange(512)
    m = affine_matrices(spec, 5, 1, idx, 512, 512).astype(np.float64) / Q
    det = np.abs(m[:, 0] * m[:, 4] - m[:, 1] * m[:, 3])
    s = 1 + spec.scale
    tol = 1e-4                         # four entries of size <= 1.25, each off by <= 2^-17: 4 * 1.25 * 2^-17 = 3.8e-5
    assert (det >= 1 / s ** 2 - tol).all() and (det <= s ** 2 + tol).all()
    assert det.min() < 0.8 and det.max() > 1.25                         # and the range is used
    assert np.array_equal(m[:, 0] < 0, flip_flags(5, 1, idx) != 0)      # |angle| <= 10 degrees: the sign is the flip
    luts = color_luts(spec, 5, 1, idx)
    assert (np.diff(luts, axis=1) >= 0).all() and luts.min() >= 0 and luts.max() <= 1
    assert len({row.tobytes() for row in luts}) == 512


# ---- loader -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(tmp_path_factory):
    imgs, masks = write_tree(tmp_path_factory.mktemp("carvana"))
    return DeviceFolderDataset(imgs, masks, newsize=(24, 16), mask_suffix="_mask", device="cpu", workers=2)


def test_loader_batches_are_the_reference_of_last_params(dev):
    aug, val, s = device_folder_loaders(dev, dev, 3, seed=4, augment="color+affine+hflip")
    assert aug.augment == "hflip+affine+color" and val.augment == "none" and val.last_params is None
    runs = {}
    for epoch in (0, 1):
        s.set_epoch(epoch)
        got = []
        for b, (img, tgt) in zip(list(aug.batches), aug):
            i = torch.as_tensor(b)
            mats, luts = aug.last_params
            assert mats.dtype == torch.int32 and tuple(mats.shape) == (len(b), 6)
            assert luts.dtype == torch.float32 and tuple(luts.shape) == (len(b), 256)
            ri, rt = augment_reference(dev.images, dev.masks, i, mats, luts)
            assert torch.equal(img, ri) and torch.equal(tgt, rt)
            assert tuple(img.shape) == (len(b), 3, 16, 24) and tuple(tgt.shape) == (len(b), 1, 16, 24)
            assert np.array_equal(aug.last_flags, flip_flags(4, epoch, i.numpy()))
            assert np.array_equal(mats[:, 0].numpy() < 0, aug.last_flags != 0)
            assert np.array_equal(mats.numpy(), affine_matrices(aug.spec, 4, epoch, i.numpy(), 16, 24))
            got.append((img, tgt))
        assert got[-1][0].shape[0] == 1                                # 7 items: a short last batch
        again = list(aug)                                              # a second pass of the same epoch
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, again))
        runs[epoch] = got
    spec = aug.spec
    assert not np.array_equal(affine_matrices(spec, 4, 0, np.arange(7), 16, 24),
                              affine_matrices(spec, 4, 1, np.arange(7), 16, 24))
    assert not np.array_equal(color_luts(spec, 4, 0, np.arange(7)), color_luts(spec, 4, 1, np.arange(7)))
    assert not all(torch.equal(a[0], b[0]) for a, b in zip(runs[0], runs[1]))


def test_loader_keeps_the_plain_paths(dev):
    """``none`` and ``hflip`` do not build matrices; a spec object carries its magnitudes through."""
    for name in ("none", "hflip"):
        aug, _, _ = device_folder_loaders(dev, dev, 3, seed=4, augment=name)
        next(iter(aug))
        assert aug.augment == name and aug.last_params is None
    plain, _, _ = device_folder_loaders(dev, dev, 3, seed=4)
    zero, _, _ = device_folder_loaders(dev, dev, 3, seed=4, augment=AugmentSpec.parse("affine+color", **ZERO))
    for (pi, pt), (zi, zt) in zip(plain, zero):
        assert torch.equal(pi, zi) and torch.equal(pt, zt)
    with pytest.raises(ValueError, match="hflip, affine and color"):
        device_folder_loaders(dev, dev, 3, augment="rotate")


# ---- command line -----------------------------------------------------------------------------------------------
def test_cli_spec_and_magnitudes(capsys):
    from distributedpytorch_amd.config import parse_args
    from distributedpytorch_amd.data.augment import spec_from_config
    cfg = parse_args(["--augment", "color+hflip", "--device-folder-data"])
    assert cfg.augment == "hflip+color" and cfg.aug_gamma is None
    assert spec_from_config(cfg) == AugmentSpec(hflip=True, color=True)
    cfg = parse_args(["--augment", "affine", "--device-folder-data", "--aug-rotate", "25", "--aug-shift", "0"])
    spec = spec_from_config(cfg)
    assert spec.rotate == 25.0 and spec.shift == 0.0 and spec.scale == 0.25 and spec.name == "affine"
    with pytest.raises(SystemExit):
        parse_args(["--augment", "hflip+elastic", "--device-folder-data"])
    assert "hflip, affine and color" in capsys.readouterr().err
    with pytest.raises(SystemExit, match="--augment affine\\+color needs --device-folder-data"):
        parse_args(["--augment", "color+affine"])
    with pytest.raises(SystemExit, match="add color to --augment"):
        parse_args(["--augment", "hflip+affine", "--device-folder-data", "--aug-gamma", "0.5"])
    with pytest.raises(SystemExit, match="add affine to --augment"):
        parse_args(["--device-folder-data", "--aug-scale", "0.5"])
    with pytest.raises(SystemExit, match="negative"):
        parse_args(["--augment", "affine", "--device-folder-data", "--aug-rotate", "-3"])
    with pytest.raises(ValueError):
        AugmentSpec.parse("affine", rotate=-1)
    for v in ("inf", "nan"):                                           # refused at the command line, not later
        with pytest.raises(SystemExit, match="--aug-shift"):
            parse_args(["--augment", "affine", "--device-folder-data", "--aug-shift", v])
    with pytest.raises(ValueError, match="finite"):
        AugmentSpec.parse("affine", shift=float("inf"))
    with pytest.raises(ValueError, match="names affine more than once"):   # a known name, repeated: not "unknown"
        AugmentSpec.parse("affine+affine")
    with pytest.raises(SystemExit):
        parse_args(["--augment", "color+hflip+color", "--device-folder-data"])
    err = capsys.readouterr().err
    assert "names color more than once" in err and "unknown" not in err


def test_show_augment_writes_a_sheet(tmp_path):
    import importlib.util
    import os
    from PIL import Image
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "show_augment.py")
    spec = importlib.util.spec_from_file_location("show_augment", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    write_tree(tmp_path / "data", n=6)
    out = tool.main(["--data-dir", str(tmp_path / "data"), "--img-size", "32", "48", "--augment", "affine+hflip",
                     "-n", "6", "--device", "cpu", "--out", str(tmp_path / "sheet.png")])
    sheet = Image.open(out)
    assert sheet.size == (4 * 48, 2 * 32) and sheet.mode == "RGB"                 # 6 items: 4 columns, 2 rows
    px = np.asarray(sheet)
    # the same first batch of epoch 0, built here: each tile is the item's image, magenta exactly where ITS warped
    # mask has an edge
    ds = DeviceFolderDataset(str(tmp_path / "data" / "train_hq"), str(tmp_path / "data" / "train_masks"),
                             newsize=(48, 32), mask_suffix="_mask", device="cpu")
    loader, _, sampler = device_folder_loaders(ds, ds, 6, seed=42, augment="hflip+affine")
    sampler.set_epoch(0)
    img, tgt = next(iter(loader))
    assert img.shape[0] == 6
    edges = 0
    for k in range(6):
        tile = px[(k // 4) * 32:(k // 4 + 1) * 32, (k % 4) * 48:(k % 4 + 1) * 48]
        edge = tool.mask_edge(tgt[k, 0].numpy())
        want = (img[k].numpy() * 255.0).round().astype(np.uint8).transpose(1, 2, 0)
        assert (tile[edge] == (255, 0, 255)).all() and np.array_equal(tile[~edge], want[~edge]), k
        edges += int(edge.sum())
    assert edges > 0
    edge = tool.mask_edge(np.pad(np.ones((3, 3)), 2))
    assert edge.sum() == 8 and not edge[3, 3]                                     # the ring of a 3 x 3 block


# ---- end to end -------------------------------------------------------------------------------------------------
def test_train_cpu_augmented_epoch_is_reproducible(tmp_path):
    """Two augmented runs write the same losses, byte for byte (the Loss column of the loss pickle: its Time
    column is the wall clock), and other losses than the un-augmented run."""
    import pandas as pd
    from distributedpytorch_amd.config import parse_args
    from distributedpytorch_amd.trainer import train
    write_tree(tmp_path / "data", n=13)
    base = ["-e", "1", "-b", "4", "--data-dir", str(tmp_path / "data"), "--img-size", "128", "--model", "unet-tiny",
            "--backend", "torch", "--dtype", "fp32", "--log-every", "1", "--device-folder-data"]

    def run(name, *extra):
        out = tmp_path / name
        train(parse_args(base + ["--out-dir", str(out), *extra]))
        loss = pd.read_pickle(out / "loss" / "singleGPU" / "train_loss.pkl")["Loss"].to_numpy()
        assert len(loss) == 3 and np.isfinite(loss).all()              # 12 training images / batch 4
        return loss.tobytes(), (out / "logs" / "singleGPU.log").read_text()

    a, log_a = run("a", "--augment", "affine+color")
    b, _ = run("b", "--augment", "color+affine")
    plain, log_p = run("plain")
    assert a == b and a != plain
    assert "augment: affine+color scale=0.25 rotate=10 shift=0.1 brightness=0.2" in log_a
    assert "augment:" not in log_p
