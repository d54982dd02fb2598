"""Scoring at the source resolution without a GPU: ``score_reference`` (PIL + numpy, the definition of the counts)
against a plain double loop, ``dice_iou`` on hand values and on the empty cases, the ground-truth rule against
``BasicDataset.preprocess``, and ``predict.py --score`` / ``evaluate.py --full-res`` end to end with the torch
backend (where a GPU is present the same tests compare the device counts with ``--host-post``)."""
import csv
import os
import re

import numpy as np
import pytest
import torch

from distributedpytorch_amd.ops import kernels as K

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

from test_device_folder_cpu import write_tree  # noqa: E402

# 0.5 and the float32 just below it: {0, 0.5, 1} inputs put many pixels exactly on 0.5, and `>` is strict
THRESHOLDS = [0.25, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.5, 0.75]


def blob_truth(H, W, seed=0):
    """Ground truth of 5-pixel runs, stored as 0 / 255 (also tests/test_score_gpu.py)."""
    rng = np.random.default_rng(seed)
    N = H * W
    return (np.repeat(rng.integers(0, 2, size=-(-N // 5)), 5)[:N] * 255).astype(np.uint8).reshape(H, W)


def _loop_counts(prob, truth, cut, thresholds):
    H, W = truth.shape
    r = np.asarray(Image.fromarray(prob).resize((W, H), resample=Image.BILINEAR))
    out = [0] * (1 + 2 * len(thresholds))
    for y in range(H):
        for x in range(W):
            car = int(truth[y, x]) > cut
            out[0] += car
            for t, thr in enumerate(thresholds):
                if r[y, x] > np.float32(thr):
                    out[1 + 2 * t] += 1
                    out[2 + 2 * t] += car
    return out


@pytest.mark.parametrize("src,dst", [((16, 24), (37, 53)), ((7, 5), (3, 11))])
def test_score_reference_equals_loop(src, dst):
    rng = np.random.default_rng(src[0] + dst[1])
    truth = blob_truth(*dst, seed=1)
    for p in (rng.random(src, dtype=np.float32), rng.choice(np.float32([0, 0.5, 1]), size=src)):
        for cut, tr in ((127, truth), (0, truth // 255)):
            got = K.score_reference(p, tr, cut, THRESHOLDS)
            assert got.dtype == np.int64 and got.shape == (9,)
            assert got.tolist() == _loop_counts(p, tr, cut, THRESHOLDS)
            assert got[0] == int((truth != 0).sum())
    assert K.score_reference(p, truth, 127, [0.5, 0.5, 0.25])[[1, 2]].tolist() == \
        K.score_reference(p, truth, 127, [0.5])[[1, 2]].tolist()                  # repeats, any order


def test_dice_iou():
    # (truth, pred, inter) per threshold: hand values, then the three degenerate cases
    d, i = K.dice_iou(np.array([10, 6, 4, 10, 10], np.int64))
    assert d.dtype == i.dtype == np.float64 and d.shape == i.shape == (2,)
    assert d.tolist() == [2 * 4 / 16, 1.0] and i.tolist() == [4 / 12, 1.0]
    d, i = K.dice_iou(np.array([[0, 0, 0], [7, 0, 0], [12, 12, 12]], np.int64))
    assert d[:, 0].tolist() == [1.0, 0.0, 1.0]          # empty / empty is a perfect score; empty prediction is 0
    assert i[:, 0].tolist() == [1.0, 0.0, 1.0]
    d, i = K.dice_iou(torch.tensor([[3, 1, 1, 0, 0]]))
    assert d.tolist() == [[0.5, 0.0]] and i.tolist() == [[1 / 3, 0.0]]
    with pytest.raises(AssertionError):
        K.dice_iou(np.zeros(4, np.int64))


@pytest.mark.parametrize("values", [(0, 1), (0, 255), (0, 100, 200, 255)])
def test_truth_rule_is_the_dataset_s(tmp_path, values):
    from distributedpytorch_amd.data.folder import BasicDataset
    from distributedpytorch_amd.predict import load_truth
    rng = np.random.default_rng(len(values))
    m = rng.choice(np.uint8(values), size=(13, 17))
    path = tmp_path / "m.png"
    Image.fromarray(m).save(path)
    arr, cut = load_truth(path, (13, 17))
    assert arr.dtype == np.uint8 and cut == (127 if max(values) > 1 else 0)
    pil = Image.open(path)
    ref = BasicDataset.preprocess(pil, pil.size, is_mask=True)
    assert np.array_equal(arr > cut, ref != 0) and 0 < int((arr > cut).sum()) < m.size
    if len(values) == 4:
        assert np.array_equal(arr > cut, m > 127)
    with pytest.raises(ValueError, match="m.png"):
        load_truth(path, (13, 18))
    # not uint8: normalised on the spot, cut 0; RGB: the first channel
    np.save(tmp_path / "f.npy", (m > 127).astype(np.int32) if max(values) > 1 else m.astype(np.int32))
    arr32, cut32 = load_truth(tmp_path / "f.npy", (13, 17))
    assert arr32.dtype == np.uint8 and cut32 == 0 and np.array_equal(arr32 > 0, arr > cut)
    Image.fromarray(np.stack([m, 255 - m, m], -1)).save(tmp_path / "rgb.png")
    a3, c3 = load_truth(tmp_path / "rgb.png", (13, 17))
    assert np.array_equal(a3 > c3, arr > cut)


# ---- the command-line tools (torch backend: run without a GPU) ------------------------------------------------
@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from distributedpytorch_amd.models.unet import build_model
    from distributedpytorch_amd.utils.checkpoint import save_model
    root = tmp_path_factory.mktemp("score")
    imgs, masks = write_tree(root / "data", n=10)
    torch.manual_seed(3)
    model = build_model("unet-tiny")
    with torch.no_grad():                           # a random net's output hugs 0.5: spread it over the threshold
        for p in model.parameters():
            p.mul_(4.0)
    save_model(model, str(root / "checkpoints" / "tiny.pth"))
    return root, imgs, masks


BASE = ["-c", "tiny", "--model", "unet-tiny", "--img-size", "16", "24", "-b", "3", "--backend", "torch",
        "--dtype", "fp32"]
CLI_THRESHOLDS = [0.3, 0.5, 0.7]


def _score(root, imgs, masks, name, *extra):
    from distributedpytorch_amd.predict import main
    out, table = root / name / "masks", root / name / "score.csv"
    res = main(BASE + ["--out-dir", str(root), "--input", str(imgs), "--output", str(out), "--score", str(masks),
                       "--score-thresholds", *map(str, CLI_THRESHOLDS), "--score-csv", str(table),
                       "--num-workers", "2", *extra])
    with open(table, newline="") as f:
        rows = list(csv.reader(f))
    return res, out, table, rows


def test_score_cli_end_to_end(setup, capsys):
    from distributedpytorch_amd.predict import load_truth
    root, imgs, masks = setup
    (n, host, (md, mi)), out, table, rows = _score(root, imgs, masks, "plain")
    printed = capsys.readouterr().out
    names = sorted(os.listdir(imgs))
    assert n == 10 and len(md) == len(mi) == 3
    assert rows[0] == ["img", "height", "width", "threshold", "truth", "pred", "inter", "dice", "iou"]
    assert [(r[0], float(r[3])) for r in rows[1:]] == [(f, t) for f in names for t in CLI_THRESHOLDS]    # N x T, sorted
    sizes, mixed = set(), 0
    for r in rows[1:]:
        name, Hs, Ws, thr, truth, pred, inter = r[0], int(r[1]), int(r[2]), float(r[3]), int(r[4]), int(r[5]), int(r[6])
        stem = os.path.splitext(name)[0]
        arr, cut = load_truth(masks / f"{stem}_mask.gif", (Hs, Ws))
        assert truth == int((arr > cut).sum()) > 0
        d, i = K.dice_iou(np.array([truth, pred, inter]))
        assert float(r[7]) == d[0] and float(r[8]) == i[0]
        if thr == 0.5:                              # --threshold: the mask that --output wrote
            png = np.array(Image.open(out / f"{stem}_mask.png"))
            assert png.shape == (Hs, Ws) and pred == int((png != 0).sum())
            assert inter == int(((png != 0) & (arr > cut)).sum())
            mixed += int(0 < inter < min(pred, truth))
        sizes.add((Hs, Ws))
    assert sizes == {(32, 48), (37, 53)} and mixed > 0          # two source sizes; not a degenerate net
    # one printed line per threshold: the mean of the CSV's per-image dice; exactly one marked best
    lines = re.findall(r"^score threshold (\S+): dice (\S+) iou (\S+) \(10 images\)(.*)$", printed, re.M)
    assert [float(l[0]) for l in lines] == CLI_THRESHOLDS
    for t, (thr, dice, iou, mark) in enumerate(lines):
        col = [float(r[7]) for r in rows[1:] if float(r[3]) == float(thr)]
        assert len(col) == 10 and abs(float(dice) - np.mean(col)) < 1e-6 and abs(md[t] - np.mean(col)) < 1e-12
        assert abs(float(iou) - mi[t]) < 1e-6
        assert ("best" in mark) == (t == int(np.argmax(md)))

    (n2, host2, _), out2, table2, _ = _score(root, imgs, masks, "hostpost", "--host-post")
    assert host2 == 10 and (host < 10 if torch.cuda.is_available() else host == 10)
    assert table2.read_bytes() == table.read_bytes()
    for f in sorted(os.listdir(out)):
        assert (out / f).read_bytes() == (out2 / f).read_bytes()


def test_score_alone_and_default_threshold(setup, capsys):
    """``--score`` is enough to run; without ``--score-thresholds`` the one threshold is ``--threshold``."""
    from distributedpytorch_amd.predict import main
    root, imgs, masks = setup
    files = [str(imgs / "car03.jpg"), str(imgs / "car00.jpg")]
    n, host, (md, mi) = main(BASE + ["--out-dir", str(root), "--input", *files, "--score", str(masks), "--threshold", "0.3"])
    out = capsys.readouterr().out
    assert n == 2 and md.shape == (1,) and "score threshold 0.3: dice" in out and "best" not in out
    assert 0.0 < md[0] < 1.0 and 0.0 < mi[0] < md[0]
    assert host == (0 if torch.cuda.is_available() else 2)


def test_score_argument_errors(setup, tmp_path, capsys):
    from distributedpytorch_amd.predict import main
    root, imgs, masks = setup
    base = BASE + ["--out-dir", str(root)]
    _, few = write_tree(tmp_path / "few", n=3)
    (few / "car01_mask.gif").unlink()
    _, twice = write_tree(tmp_path / "twice", n=3)
    Image.fromarray(np.zeros((32, 48), np.uint8)).save(twice / "car02_mask.png")
    cases = {"nothing to write": ["--input", str(imgs)],
             "--score": ["--input", str(imgs)],                                       # ... which now names --score
             "no mask for car01": ["--input", str(imgs), "--score", str(few)],
             "several masks for car02": ["--input", str(imgs / "car02.jpg"), "--score", str(twice)],
             "at most 8": ["--input", str(imgs), "--score", str(masks), "--score-thresholds", *["0.5"] * 9],
             "need --score": ["--input", str(imgs), "--rle", str(tmp_path / "a.csv"), "--score-csv", str(tmp_path / "b.csv")],
             "no such directory": ["--input", str(imgs), "--score", str(tmp_path / "nowhere")]}
    for msg, args in cases.items():
        with pytest.raises(SystemExit) as e:
            main(base + args)
        assert e.value.code == 2 and msg in capsys.readouterr().err, msg
    assert not (tmp_path / "a.csv").exists()
    # a mask of another size than its image: the decode raises, naming the image
    _, other = write_tree(tmp_path / "other", n=2)
    Image.fromarray(np.zeros((32, 47), np.uint8)).save(other / "car00_mask.gif")
    with pytest.raises(ValueError, match="car00.jpg"):
        main(base + ["--input", str(imgs / "car00.jpg"), "--score", str(other)])


def test_evaluate_full_res(setup, capsys, monkeypatch):
    import evaluate
    from distributedpytorch_amd.data import CarvanaDataset, split_dataset
    from distributedpytorch_amd.predict import Predictor
    root, imgs, masks = setup
    seen = []
    real = Predictor.score_files

    def spy(self, pairs, *args, **kw):
        seen.extend(pairs)
        return real(self, pairs, *args, **kw)

    monkeypatch.setattr(Predictor, "score_files", spy)
    args = ["-c", "tiny", "--out-dir", str(root), "--model", "unet-tiny", "--img-size", "16", "24", "-b", "3",
            "--backend", "torch", "--dtype", "fp32", "--data-dir", str(root / "data"), "-v", "40"]
    plain = evaluate.main(args)
    out = capsys.readouterr().out
    assert len(plain) == 2 and "full_res" not in out and not seen
    loss, dice, (fd, fi) = evaluate.main(args + ["--full-res"])
    out2 = capsys.readouterr().out
    assert (loss, dice) == plain and out2.startswith(out)              # the first two lines are unchanged
    m = re.search(r"^full_res dice (\S+) iou (\S+) \(4 images, threshold 0.5\)$", out2, re.M)
    assert m and abs(float(m.group(1)) - fd) < 1e-6 and abs(float(m.group(2)) - fi) < 1e-6
    assert 0.0 < fi < fd < 1.0
    ds = CarvanaDataset(imgs, masks, newsize=(24, 16))
    _, val = split_dataset(ds, 40, seed=0)
    assert [os.path.basename(p) for p, _ in seen] == [ds.ids[i] + ".jpg" for i in val.indices] and len(seen) == 4
    assert [os.path.basename(q) for _, q in seen] == [ds.ids[i] + "_mask.gif" for i in val.indices]
    with pytest.raises(SystemExit):
        evaluate.main(args + ["--full-res", "--synthetic"])
