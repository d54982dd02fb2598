"""Resident folder dataset (data/device_folder.py) on the CPU path: the same class holds PIL's results, so its
items, its loader's batches (samplers, split, short last batch, two DDP ranks), the hflip augmentation, the
resampling tables behind the GPU kernels and the command-line flags are all checked without a GPU."""
import numpy as np
import pytest
import torch

from distributedpytorch_amd.data import (CarvanaDataset, DeviceBatcher, DeviceFolderDataset, build_loaders,
                                         device_folder_loaders, split_dataset)
from distributedpytorch_amd.data.device_folder import flip_flags
from distributedpytorch_amd.ops import kernels as K

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

NEWSIZE = (24, 16)      # (W, H)


def write_tree(root, n=7, seed=0, mode="RGB"):
    """A tiny Carvana tree: JPEG + ``_mask.gif``, two different source sizes in one folder."""
    rng = np.random.default_rng(seed)
    imgs, masks = root / "train_hq", root / "train_masks"
    imgs.mkdir(parents=True)
    masks.mkdir(parents=True)
    for i in range(n):
        h, w = ((32, 48), (37, 53))[i % 2]
        shape = (h, w, 3) if mode == "RGB" else (h, w)
        # smooth + noise, so JPEG keeps structure and the bicubic overshoot is exercised
        px = (rng.integers(0, 256, size=shape) // 64 * 64 + rng.integers(0, 64, size=shape)).astype(np.uint8)
        m = np.zeros((h, w), np.uint8)
        m[h // 4:3 * h // 4, w // 4 + i:3 * w // 4] = 255
        Image.fromarray(px).save(imgs / f"car{i:02d}.jpg", quality=95)
        Image.fromarray(m).save(masks / f"car{i:02d}_mask.gif")
    return imgs, masks


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    imgs, masks = write_tree(tmp_path_factory.mktemp("carvana"))
    host = CarvanaDataset(imgs, masks, newsize=NEWSIZE)
    dev = DeviceFolderDataset(imgs, masks, newsize=NEWSIZE, mask_suffix="_mask", device="cpu", workers=2)
    return host, dev


def _same(dev_loader, host_loader):
    a, b = list(dev_loader), list(DeviceBatcher(host_loader, torch.device("cpu")))
    assert len(a) == len(b) and len(a) > 0
    for (xi, xt), (yi, yt) in zip(a, b):
        assert xi.dtype == yi.dtype == torch.float32 and xt.dtype == yt.dtype == torch.float32
        assert torch.equal(xi, yi) and torch.equal(xt, yt)
    return a


def test_items_equal_carvana(tree):
    host, dev = tree
    assert len(dev) == len(host) == 7 and dev.ids == host.ids
    assert dev.images.dtype == torch.uint8 and tuple(dev.images.shape) == (7, 3, 16, 24)
    assert dev.nbytes == 7 * 4 * 16 * 24
    for i in range(len(host)):
        a, b = dev[i], host[i]
        assert a["image"].dtype == torch.float32 and a["mask"].dtype == torch.int64
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["mask"], b["mask"])
    assert set(dev.masks.unique().tolist()) == {0, 1}


def test_grey_folder_items(tmp_path):
    imgs, masks = write_tree(tmp_path, n=3, mode="L")
    host = CarvanaDataset(imgs, masks, newsize=NEWSIZE)
    dev = DeviceFolderDataset(imgs, masks, newsize=NEWSIZE, mask_suffix="_mask", device="cpu")
    assert tuple(dev.images.shape) == (3, 1, 16, 24)
    for i in range(3):
        assert torch.equal(dev[i]["image"], host[i]["image"]) and torch.equal(dev[i]["mask"], host[i]["mask"])


def test_pairing_errors_are_basicdataset_s(tmp_path):
    imgs, masks = write_tree(tmp_path, n=3)
    with pytest.raises(RuntimeError, match="No input file found"):
        DeviceFolderDataset(tmp_path / "nowhere", masks, device="cpu")
    (masks / "car01_mask.gif").unlink()
    with pytest.raises(AssertionError, match="no mask or multiple masks"):
        DeviceFolderDataset(imgs, masks, mask_suffix="_mask", device="cpu")
    Image.fromarray(np.zeros((10, 10), np.uint8)).save(masks / "car01_mask.gif")
    with pytest.raises(AssertionError, match="should be the same size"):
        DeviceFolderDataset(imgs, masks, newsize=(8, 8), mask_suffix="_mask", device="cpu")


def test_not_8bit_names_the_file(tmp_path):
    imgs, masks = tmp_path / "i", tmp_path / "m"
    imgs.mkdir()
    masks.mkdir()
    np.save(imgs / "a.npy", np.full((8, 8), 1000, np.int32))          # PIL mode I: 32-bit
    np.save(masks / "a.npy", np.eye(8, dtype=np.uint8))
    with pytest.raises(ValueError, match="a.npy"):
        DeviceFolderDataset(imgs, masks, newsize=(8, 8), device="cpu")


@pytest.mark.parametrize("bs", [2, 3])       # 7 items: both leave a short last batch
def test_batches_equal_host_loader(tree, bs):
    host, dev = tree
    dl, dv, ds = device_folder_loaders(dev, dev, bs, seed=5)
    hl, hv, hs = build_loaders(host, host, bs, seed=5)
    for epoch in (0, 3):
        ds.set_epoch(epoch)
        hs.set_epoch(epoch)
        got = _same(dl, hl)
        assert got[-1][0].shape[0] == 7 % bs
    _same(dv, hv)


def test_batches_through_split(tree):
    host, dev = tree
    ht, hv = split_dataset(host, 30, seed=0)
    dt, dv = split_dataset(dev, 30, seed=0)
    assert len(dt) == 5 and len(dv) == 2
    dl, dvl, _ = device_folder_loaders(dt, dv, 2, seed=1)
    hl, hvl, _ = build_loaders(ht, hv, 2, seed=1)
    _same(dl, hl)
    _same(dvl, hvl)


@pytest.mark.parametrize("rank", [0, 1])
def test_batches_distributed_world2(tree, rank):
    host, dev = tree
    ht, hv = split_dataset(host, 30, seed=0)
    dt, dv = split_dataset(dev, 30, seed=0)
    dl, dvl, ds = device_folder_loaders(dt, dv, 2, rank=rank, world_size=2, seed=9)
    hl, hvl, hs = build_loaders(ht, hv, 2, rank=rank, world_size=2, seed=9)
    ds.set_epoch(2)
    hs.set_epoch(2)
    _same(dl, hl)
    _same(dvl, hvl)


def test_hflip_batches(tree):
    _, dev = tree
    plain, _, ps = device_folder_loaders(dev, dev, 3, seed=4)
    aug, val, s = device_folder_loaders(dev, dev, 3, seed=4, augment="hflip")
    assert val.augment == "none"                                  # training loader only
    flags_by_epoch = {}
    for epoch in (0, 1):
        ps.set_epoch(epoch)
        s.set_epoch(epoch)
        flags = []
        for (pi, pt), (ai, at) in zip(plain, aug):
            f = aug.last_flags
            assert f is not None and f.dtype == np.uint8 and f.shape == (pi.shape[0],)
            fb = torch.from_numpy(f).bool().view(-1, 1, 1, 1)
            assert torch.equal(ai, torch.where(fb, torch.flip(pi, dims=[-1]), pi))
            assert torch.equal(at, torch.where(fb, torch.flip(pt, dims=[-1]), pt))
            flags.append(f.copy())
        again = [aug.last_flags.copy() for _ in aug]               # a second pass of the same epoch
        assert all(np.array_equal(a, b) for a, b in zip(flags, again))
        flags_by_epoch[epoch] = np.concatenate(flags)
    assert 0 < flags_by_epoch[0].sum() < 7                         # some, not all, of the 7 items
    # per base index, epoch 1 differs from epoch 0 somewhere (compared item by item, not in shuffled order)
    assert not np.array_equal(flip_flags(4, 0, np.arange(7)), flip_flags(4, 1, np.arange(7)))


def test_flip_hash_is_balanced_and_pure():
    idx = np.arange(64)
    for seed, epoch in ((0, 0), (42, 0), (42, 1), (7, 13)):
        f = flip_flags(seed, epoch, idx)
        assert 16 <= int(f.sum()) <= 48, (seed, epoch, int(f.sum()))
        assert np.array_equal(f, flip_flags(seed, epoch, idx))
        assert np.array_equal(f[::-1], flip_flags(seed, epoch, idx[::-1]))     # per item, not per position
    assert not np.array_equal(flip_flags(42, 0, idx), flip_flags(42, 1, idx))
    assert not np.array_equal(flip_flags(42, 0, idx), flip_flags(43, 0, idx))


# the shapes of the GPU tests (H, W) -> (H, W), minus the full-size one
SHAPES = [((37, 53), (16, 24)), ((50, 70), (64, 96)), ((33, 47), (32, 48)), ((20, 31), (48, 16)),
          ((32, 48), (32, 24)), ((64, 96), (64, 96)), ((600, 40), (8, 40)), ((1280, 1918), (512, 512))]


@pytest.mark.parametrize("src,dst", SHAPES)
def test_bicubic_tables_equal_pil(src, dst):
    rng = np.random.default_rng(src[0] * 1000 + dst[1])
    for shape in (src + (3,), src):
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        ref = np.asarray(Image.fromarray(a).resize((dst[1], dst[0]), resample=Image.BICUBIC))
        assert np.array_equal(K.resize_bicubic_reference(a, dst[0], dst[1]), ref)


def test_bicubic_table_layout():
    b, c = K.bicubic_table(1918, 960)
    assert b.dtype == np.int32 and c.dtype == np.int32 and b.shape == (960, 2) and c.shape == (960, 9)
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 1918).all() and (b[:, 1] <= 9).all()
    assert (np.abs(c.sum(1) - (1 << 22)) <= 9).all()               # normalised; one rounding per tap
    b, c = K.bicubic_table(96, 96)                                 # skipped pass: the identity table
    assert c.shape == (96, 1) and (c == 1 << 22).all() and (b[:, 0] == np.arange(96)).all() and (b[:, 1] == 1).all()


@pytest.mark.parametrize("src,dst", SHAPES)
def test_nearest_table_equals_pil(src, dst):
    rng = np.random.default_rng(7)
    m = rng.integers(0, 256, size=src, dtype=np.uint8)
    ref = np.asarray(Image.fromarray(m).resize((dst[1], dst[0]), resample=Image.NEAREST))
    assert np.array_equal(m[K.nearest_table(src[0], dst[0])][:, K.nearest_table(src[1], dst[1])], ref)


def test_nearest_table_follows_pil_s_running_sum():
    """2 -> 7: (3 + 0.5) * 2 / 7 is exactly 1, but PIL's accumulated coordinate stays just below it."""
    ref = np.asarray(Image.fromarray(np.array([[10, 20]], np.uint8)).resize((7, 1), resample=Image.NEAREST))[0]
    assert np.array_equal(np.array([10, 20], np.uint8)[K.nearest_table(2, 7)], ref)


def test_unit_table_is_the_host_conversion():
    host = torch.as_tensor(np.arange(256, dtype=np.uint8) / 255.0).float()
    assert torch.equal(K.unit_table("cpu"), host)
    assert (torch.arange(256, dtype=torch.float32) * (1.0 / 255.0) != host).any()     # why it is a table


def test_augment_needs_device_folder_data():
    from distributedpytorch_amd.config import parse_args
    with pytest.raises(SystemExit, match="--augment hflip needs --device-folder-data"):
        parse_args(["--augment", "hflip"])
    cfg = parse_args(["--augment", "hflip", "--device-folder-data"])
    assert cfg.augment == "hflip" and cfg.device_folder_data
    cfg = parse_args([])
    assert cfg.augment == "none" and not cfg.device_folder_data


def test_train_cpu_same_loss_curve_with_the_flag(tmp_path):
    """One CPU epoch of the single-device method over real files: the resident dataset's CPU path feeds the
    same batches, so the loss curve is the host path's, value for value."""
    from distributedpytorch_amd.config import parse_args
    from distributedpytorch_amd.trainer import train
    write_tree(tmp_path / "data", n=8)
    base = ["-e", "1", "-b", "2", "-v", "25", "--data-dir", str(tmp_path / "data"), "--img-size", "32", "--model",
            "unet-tiny", "--backend", "torch", "--dtype", "fp32", "--log-every", "1"]
    a = train(parse_args(base + ["--out-dir", str(tmp_path / "host")]))
    b = train(parse_args(base + ["--out-dir", str(tmp_path / "resident"), "--device-folder-data"]))
    assert a["step"] == b["step"] == 3
    assert [r[2] for r in a["curves"].train] == [r[2] for r in b["curves"].train]
    assert [r[2] for r in a["curves"].val] == [r[2] for r in b["curves"].val]
    assert "folder dataset resident on cpu" in (tmp_path / "resident" / "logs" / "singleGPU.log").read_text()
