"""Mask cleaning without a GPU: ``clean_reference`` / ``label_reference`` (numpy, the definition) on hand-drawn
masks, against scipy where it is installed, idempotence on every pattern, ``parse_clean``, and ``predict.py
--clean`` / ``evaluate.py --clean`` end to end with the torch backend (where a GPU is present the same test runs
the device path against the reference)."""
import csv
import os

import numpy as np
import pytest

from distributedpytorch_amd.ops import kernels as K

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

from clean_patterns import CASES, FLAGS, PATTERNS, SIZES, pattern  # noqa: E402
from test_score_cpu import BASE, CLI_THRESHOLDS, _score, setup  # noqa: E402,F401


def _m(*rows):
    return np.array([[int(c) for c in r] for r in rows], np.uint8)


# (mask, {(largest, fill): (expected, stats)})
DIAGONAL = _m("010000",        # diagonal steps only: ONE 8-connected component of six pixels ...
              "001000",
              "000100",
              "001010",        # ... and the background pixel (3, 3) in the diamond is cut off from the rest by
              "000100",        # diagonal steps only: background is 4-connected, so it is a hole
              "000000")
FILLED = DIAGONAL.copy()
FILLED[3, 3] = 1
TIE = _m("000011",             # two components of 2 pixels; the right one's first pixel comes first in row-major order
         "110000",
         "000000",
         "111000")             # the whole of it: a larger one below them wins
SPECK = _m("111111",
           "100001",
           "101001",           # a speck inside the hole: removed by `largest`, and the hole is then filled whole
           "100001",
           "111111",
           "000000")
HAND = [
    (DIAGONAL, {(True, False): (DIAGONAL, (1, 0, 0)),
                (False, True): (FILLED, (0, 0, 1)),
                (True, True): (FILLED, (1, 0, 1))}),
    (_m("00100",               # a diamond: its centre is enclosed by diagonal steps only
        "01010",
        "00100",
        "00000",
        "10000"),
     {(True, False): (_m("00100", "01010", "00100", "00000", "00000"), (2, 1, 0)),
      (False, True): (_m("00100", "01110", "00100", "00000", "10000"), (0, 0, 1)),
      (True, True): (_m("00100", "01110", "00100", "00000", "00000"), (2, 1, 1))}),
    (TIE[:2], {(True, False): (_m("000011", "000000"), (2, 2, 0)),
               (False, True): (TIE[:2], (0, 0, 0)),
               (True, True): (_m("000011", "000000"), (2, 2, 0))}),
    (TIE, {(True, False): (_m("000000", "000000", "000000", "111000"), (3, 4, 0)),
           (False, True): (TIE, (0, 0, 0)),
           (True, True): (_m("000000", "000000", "000000", "111000"), (3, 4, 0))}),
    (SPECK, {(True, False): (_m("111111", "100001", "100001", "100001", "111111", "000000"), (2, 1, 0)),
             (False, True): (_m("111111", "111111", "111111", "111111", "111111", "000000"), (0, 0, 11)),
             (True, True): (_m("111111", "111111", "111111", "111111", "111111", "000000"), (2, 1, 12))}),
    (_m("0000", "0000"), {(True, False): (_m("0000", "0000"), (0, 0, 0)),
                          (False, True): (_m("0000", "0000"), (0, 0, 0)),
                          (True, True): (_m("0000", "0000"), (0, 0, 0))}),
]


@pytest.mark.parametrize("k", range(len(HAND)))
def test_clean_reference_hand_drawn(k):
    mask, want = HAND[k]
    for (largest, fill), (exp, stats) in want.items():
        for value, scale in ((255, 7), (1, 1)):               # any non-zero byte is foreground
            got, st = K.clean_reference(mask * np.uint8(scale), largest, fill, value)
            assert got.dtype == np.uint8 and st.dtype == np.int64 and st.shape == (3,)
            assert np.array_equal(got, exp * np.uint8(value)), (k, largest, fill)
            assert tuple(st.tolist()) == stats, (k, largest, fill)


def test_label_reference_hand_drawn():
    lab8, lab4 = K.label_reference(DIAGONAL != 0, 8), K.label_reference(DIAGONAL != 0, 4)
    assert lab8.dtype == np.int32 and lab8.shape == DIAGONAL.shape
    assert (lab8[DIAGONAL != 0] == 1).all() and (lab8[DIAGONAL == 0] == -1).all()         # one component, rooted at 1
    assert np.array_equal(lab4[DIAGONAL != 0], np.flatnonzero(DIAGONAL.reshape(-1)))       # every pixel its own
    bg = K.label_reference(DIAGONAL == 0, 4)
    assert bg[3, 3] == 3 * 6 + 3 and (bg == 21).sum() == 1 and bg[0, 0] == 0 and bg[5, 5] == 0 and bg[0, 1] == -1
    assert K.label_reference(DIAGONAL == 0, 8)[3, 3] == 0
    with pytest.raises(AssertionError):
        K.label_reference(DIAGONAL, 6)


def _scipy_clean(ndi, m, largest, fill):
    fg, st = m != 0, [0, 0, 0]
    keep = fg
    if largest:
        lab, n = ndi.label(fg, structure=np.ones((3, 3)))     # numbered in the row-major order of the first pixels
        st[0] = n
        if n:
            keep = lab == int(np.argmax(np.bincount(lab.ravel())[1:])) + 1
            st[1] = int(fg.sum() - keep.sum())
    if fill:
        filled = ndi.binary_fill_holes(keep)
        st[2] = int(filled.sum() - keep.sum())
        keep = filled
    return keep, st


@pytest.mark.parametrize("name", list(PATTERNS))
def test_clean_reference_equals_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    for size in SIZES:
        m = pattern(name, size)
        for largest, fill in FLAGS:
            got, st = K.clean_reference(m, largest, fill)
            want, wst = _scipy_clean(ndi, m, largest, fill)
            assert np.array_equal(got != 0, want) and st.tolist() == wst, (name, size, largest, fill)
        for conn, structure in ((8, np.ones((3, 3))), (4, None)):
            lab = K.label_reference(m != 0, conn)
            ref, n = ndi.label(m != 0, structure=structure)
            assert np.array_equal(lab >= 0, ref > 0)
            if n:                                            # a bijection between the two numberings ...
                pairs = np.unique(np.stack([lab[ref > 0], ref[ref > 0]]), axis=1)
                assert pairs.shape[1] == n == len(set(pairs[0])) == len(set(pairs[1])), (name, size, conn)
                first = np.full(n + 1, m.size)               # ... and a label is its component's smallest index
                np.minimum.at(first, ref.reshape(-1), np.arange(m.size))
                assert np.array_equal(lab[ref > 0], first[ref[ref > 0]])


@pytest.mark.parametrize("name", list(PATTERNS))
def test_clean_reference_idempotent(name):
    for size in SIZES:
        m = pattern(name, size)
        for largest, fill in FLAGS:
            once, st = K.clean_reference(m, largest, fill)
            twice, st2 = K.clean_reference(once, largest, fill)
            assert np.array_equal(once, twice), (name, size, largest, fill)
            assert st2[1] == 0 and st2[2] == 0 and st2[0] == (int(once.any()) if largest else 0)
            assert set(np.unique(once).tolist()) <= {0, 255}
            if not largest:                                  # filling only adds
                assert ((m != 0) <= (once != 0)).all() and st[2] == int((once != 0).sum() - (m != 0).sum())
            if not fill:                                     # the largest component only removes
                assert ((once != 0) <= (m != 0)).all() and st[1] == int((m != 0).sum() - (once != 0).sum())


def test_pattern_properties():
    """The patterns are what their names say (at a size with 2 x 2 tiles and more)."""
    H, W = 130, 259
    one = lambda m: K.clean_reference(m, True, False)[1]  # noqa: E731
    assert one(pattern("checker", (H, W)))[0] == 1 and one(pattern("snake", (H, W))).tolist() == [1, 0, 0]
    ck, st = K.clean_reference(pattern("checker", (H, W)), False, True)
    assert st[2] == ((H - 2) * (W - 2)) // 2 and (ck[1:-1, 1:-1] != 0).all()
    fr, st = K.clean_reference(pattern("frame", (H, W)), True, True)
    assert (fr != 0).all() and st.tolist() == [1, 0, (H - 2) * (W - 2)]
    assert one(pattern("rings", (H, W)))[0] == (min(H, W) // 2 + 2) // 3 > 20
    for name, row in (("rects", 0), ("rects_shifted", -1)):
        m = pattern(name, (H, W))
        kept, st = K.clean_reference(m, True, False)
        assert st[0] == 2 and st[1] * 2 == int((m != 0).sum())                   # equal areas: a tie
        cols = np.flatnonzero((kept != 0).any(0))
        assert (cols.min() > W // 2) == (row < 0)             # level: the left one starts first; shifted: the right one
    for d in ("random30", "random50", "random59"):
        st = one(pattern(d, (H, W)))
        assert st[0] > 20 and st[1] > 0
    assert set(np.unique(pattern("bytes", (37, 53))).tolist()) == {0, 1, 7, 255}
    assert len(CASES) == len(PATTERNS) * len(SIZES) == 17 * 7


def test_parse_clean():
    for text, want in (("none", "none"), ("largest", "largest"), ("fill", "fill"), ("largest+fill", "largest+fill"),
                       ("fill+largest", "largest+fill"), (" fill + largest ", "largest+fill"),
                       ("fill+fill", "fill")):
        assert K.parse_clean(text) == want
    for text, part in (("holes", "'holes'"), ("largest+", "empty part"), ("+fill", "empty part"), ("", "empty part"),
                       ("largest+none", "'none'"), ("largest++fill", "empty part"), ("Largest", "'Largest'")):
        with pytest.raises(ValueError, match=part):
            K.parse_clean(text)


# ---- the command-line tools (torch backend: run without a GPU) ------------------------------------------------
def _rle_rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_clean_cli_end_to_end(setup, capsys):  # noqa: F811
    """``--clean largest+fill`` writes what ``clean_reference`` makes of the masks of a run without the flag: PNG,
    run-length CSV and score CSV; ``--clean none`` changes no byte and no printed line."""
    from distributedpytorch_amd.predict import load_truth, rle_string
    root, imgs, masks = setup
    (n, _, _), out0, table0, rows0 = _score(root, imgs, masks, "c_plain", "--rle", str(root / "c_plain" / "rle.csv"))
    printed0 = capsys.readouterr().out
    (n1, _, _), out1, table1, _ = _score(root, imgs, masks, "c_none", "--rle", str(root / "c_none" / "rle.csv"),
                                         "--clean", "none")
    printed1 = capsys.readouterr().out
    assert "cleaned" not in printed0 and table1.read_bytes() == table0.read_bytes()
    assert (root / "c_none" / "rle.csv").read_bytes() == (root / "c_plain" / "rle.csv").read_bytes()
    strip = lambda s: [l for l in s.splitlines() if not l.startswith("predicted ")]  # noqa: E731  (that line is timed)
    assert strip(printed1) == strip(printed0) and len(printed1.splitlines()) == len(printed0.splitlines())
    for f in sorted(os.listdir(out0)):
        assert (out1 / f).read_bytes() == (out0 / f).read_bytes()

    (n2, _, _), out2, table2, rows2 = _score(root, imgs, masks, "c_clean", "--rle", str(root / "c_clean" / "rle.csv"),
                                             "--clean", "fill+largest")
    printed2 = capsys.readouterr().out
    assert n == n1 == n2 == 10 and rows2[0] == rows0[0] and len(rows2) == len(rows0)
    rle = dict(_rle_rows(root / "c_clean" / "rle.csv")[1:])
    total, changed, lost = np.zeros(3, np.int64), 0, 0
    for f in sorted(os.listdir(out0)):
        plain = np.array(Image.open(out0 / f))
        want, st = K.clean_reference(plain, True, True)
        got = np.array(Image.open(out2 / f))
        assert got.dtype == np.uint8 and np.array_equal(got, want), f
        assert rle[f.replace("_mask.png", ".jpg")] == rle_string(K.rle_reference(want))
        total += st
        changed += int(not np.array_equal(want, plain))
        lost += int(st[1] > 0)
    assert changed > 0 and total[1] > 0                      # the cleaning did something to these masks
    removed = sum(max(int(K.clean_reference(np.array(Image.open(out0 / f)), True, False)[1][0]) - 1, 0)
                  for f in sorted(os.listdir(out0)))
    assert f"cleaned (largest+fill): {removed} components removed from {lost} files, {int(total[2])} pixels filled" \
        in printed2
    # the score CSV: the 0.5 rows count the cleaned --threshold masks; every row is clean_reference of SOME mask
    for r0, r2 in zip(rows0[1:], rows2[1:]):
        assert r0[:5] == r2[:5]                              # img, height, width, threshold, truth
        if float(r2[3]) == 0.5:
            stem = os.path.splitext(r2[0])[0]
            m = np.array(Image.open(out2 / f"{stem}_mask.png")) != 0
            arr, cut = load_truth(masks / f"{stem}_mask.gif", m.shape)
            assert int(r2[5]) == int(m.sum()) and int(r2[6]) == int((m & (arr > cut)).sum())
            d, i = K.dice_iou(np.array([int(r2[4]), int(r2[5]), int(r2[6])]))
            assert float(r2[7]) == d[0] and float(r2[8]) == i[0]

    # --host-post writes the same files, byte for byte
    _, out3, table3, _ = _score(root, imgs, masks, "c_host", "--rle", str(root / "c_host" / "rle.csv"),
                                "--clean", "largest+fill", "--host-post")
    assert table3.read_bytes() == table2.read_bytes()
    assert (root / "c_host" / "rle.csv").read_bytes() == (root / "c_clean" / "rle.csv").read_bytes()
    for f in sorted(os.listdir(out2)):
        assert (out3 / f).read_bytes() == (out2 / f).read_bytes()
    assert "cleaned (largest+fill)" in capsys.readouterr().out


def test_clean_cli_other_thresholds(setup):  # noqa: F811
    """Every row of the score CSV under ``--clean``: the counts of ``clean_reference`` of the mask at ITS threshold
    (taken from a run with that ``--threshold``)."""
    from distributedpytorch_amd.predict import load_truth, main
    root, imgs, masks = setup
    files = [str(imgs / "car01.jpg"), str(imgs / "car04.jpg")]
    table = root / "c_thr" / "score.csv"
    main(BASE + ["--out-dir", str(root), "--input", *files, "--score", str(masks), "--score-thresholds",
                 *map(str, CLI_THRESHOLDS), "--score-csv", str(table), "--clean", "largest"])
    rows = _rle_rows(table)[1:]
    assert len(rows) == 2 * len(CLI_THRESHOLDS)
    for thr in CLI_THRESHOLDS:
        out = root / "c_thr" / f"m{thr}"
        main(BASE + ["--out-dir", str(root), "--input", *files, "--output", str(out), "--threshold", str(thr)])
        for r in (r for r in rows if float(r[3]) == thr):
            stem = os.path.splitext(r[0])[0]
            want = K.clean_reference(np.array(Image.open(out / f"{stem}_mask.png")), True, False)[0] != 0
            arr, cut = load_truth(masks / f"{stem}_mask.gif", want.shape)
            assert (int(r[5]), int(r[6])) == (int(want.sum()), int((want & (arr > cut)).sum())), (thr, stem)


def test_clean_argument_errors(setup, capsys):  # noqa: F811
    import evaluate
    from distributedpytorch_amd.predict import main
    root, imgs, masks = setup
    for spec, msg in (("holes", "unknown part 'holes'"), ("largest+", "empty part")):
        with pytest.raises(SystemExit) as e:
            main(BASE + ["--out-dir", str(root), "--input", str(imgs), "--score", str(masks), "--clean", spec])
        assert e.value.code == 2 and msg in capsys.readouterr().err
    args = ["-c", "tiny", "--out-dir", str(root), "--model", "unet-tiny", "--img-size", "16", "24", "-b", "3",
            "--backend", "torch", "--dtype", "fp32", "--data-dir", str(root / "data"), "-v", "40"]
    with pytest.raises(SystemExit) as e:
        evaluate.main(args + ["--clean", "fill"])
    assert e.value.code == 2 and "--clean fill needs --full-res" in capsys.readouterr().err
    loss, dice, (fd, fi) = evaluate.main(args + ["--full-res", "--clean", "fill+largest"])
    out = capsys.readouterr().out
    assert "(4 images, threshold 0.5, clean largest+fill)" in out and 0.0 < fi < fd <= 1.0
    plain = evaluate.main(args + ["--full-res"])
    assert plain[:2] == (loss, dice) and plain[2] != (fd, fi)            # cleaning moved the score
