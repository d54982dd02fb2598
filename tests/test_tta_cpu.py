"""Test-time augmentation and ensembling without a GPU: ``parse_tta`` / ``tta_codes``, the numpy definitions
``tta_views_reference`` and ``tta_merge_reference`` (copies of one array come back bit for bit, the adds run in
member order), ``Predictor.merged_probs`` on a CPU (the un-mirror pairing with a pointwise stub, the member order
with two real models) and ``predict.py --tta / --ensemble`` and ``evaluate.py --tta`` end to end with the torch
backend."""
import csv
import math
import os

import numpy as np
import pytest
import torch

from distributedpytorch_amd.ops import kernels as K

PIL = pytest.importorskip("PIL")

from test_score_cpu import BASE, setup  # noqa: E402,F401

F32 = np.float32
FLIPS = {0: [], 1: [3], 2: [2], 3: [2, 3]}          # mirror code -> torch.flip dims of [B, C, h, w]


def test_parse_tta_and_codes():
    for text, want, codes in (("none", "none", [0]), ("hflip", "hflip", [0, 1]), ("vflip", "vflip", [0, 2]),
                              ("hvflip", "hvflip", [0, 3]), ("vflip+hflip", "hflip+vflip", [0, 1, 2]),
                              ("hvflip+hflip", "hflip+hvflip", [0, 1, 3]), (" hvflip + vflip ", "vflip+hvflip", [0, 2, 3]),
                              ("hvflip+vflip+hflip", "hflip+vflip+hvflip", [0, 1, 2, 3]),
                              ("hflip+hflip", "hflip", [0, 1])):
        assert K.parse_tta(text) == want and K.tta_codes(text) == codes
    for text, part in (("flip", "'flip'"), ("hflip+", "empty part"), ("+vflip", "empty part"), ("", "empty part"),
                       ("hflip+none", "'none'"), ("hflip++vflip", "empty part"), ("Hflip", "'Hflip'")):
        with pytest.raises(ValueError, match=part):
            K.parse_tta(text)
        with pytest.raises(ValueError, match=part):
            K.tta_codes(text)


def test_views_reference():
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, size=(2, 3, 3, 5), dtype=np.uint8)
    v = K.tta_views_reference(u8, [0, 1, 2, 3])
    assert v.dtype == F32 and v.shape == (4, 2, 3, 3, 5) and v.flags.c_contiguous
    unit = (np.arange(256, dtype=np.float64) / 255.0).astype(F32)
    for b in range(2):
        for y in range(3):
            for x in range(5):
                want = unit[u8[b, :, y, x]]
                assert np.array_equal(v[0, b, :, y, x], want) and np.array_equal(v[1, b, :, y, 4 - x], want)
                assert np.array_equal(v[2, b, :, 2 - y, x], want) and np.array_equal(v[3, b, :, 2 - y, 4 - x], want)
    assert np.array_equal(K.tta_views_reference(u8, [3, 0])[0], v[3])


@pytest.mark.parametrize("codes", [[0, 1], [0, 2], [3, 1], [0, 1, 2, 3], [2, 2, 1, 0]])
def test_merge_reference_of_copies_is_the_array(codes):
    """Sums of 2 or 4 equal float32 values and the factors 0.5 and 0.25 are exact."""
    rng = np.random.default_rng(len(codes))
    a = rng.random((2, 5, 7), dtype=F32)
    members = [np.ascontiguousarray(K._mirror(a, c)) for c in codes]
    got = K.tta_merge_reference(members, codes)
    assert got.dtype == F32 and got.tobytes() == a.tobytes()
    wrong = K.tta_merge_reference(members, codes[1:] + codes[:1])           # members paired with other codes
    assert wrong.tobytes() != a.tobytes()


def test_merge_reference_adds_in_member_order():
    big, one = F32(2.0 ** 24), F32(1.0)
    r = F32(1.0 / 3)
    m = lambda v: np.full((1, 1, 2), v, F32)  # noqa: E731
    first = K.tta_merge_reference([m(big), m(one), m(one)], [0, 0, 0])     # (2^24 + 1) + 1: both adds round back
    last = K.tta_merge_reference([m(one), m(one), m(big)], [0, 0, 0])      # (1 + 1) + 2^24 is exact
    assert first[0, 0, 0] == F32(big * r) and last[0, 0, 0] == F32(F32(big + F32(2.0)) * r)
    assert first[0, 0, 0] != last[0, 0, 0]
    # r is the rounded float64 quotient, applied once at the end
    seven = K.tta_merge_reference([m(F32(0.7))] * 3, [0, 0, 0])
    s = F32(F32(F32(0.7) + F32(0.7)) + F32(0.7))
    assert seven[0, 0, 0] == F32(s * r)
    one_member = np.random.default_rng(1).random((1, 3, 4), dtype=F32)
    assert K.tta_merge_reference([one_member[:, :, ::-1]], [1]).tobytes() == one_member.tobytes()
    with pytest.raises(AssertionError):
        K.tta_merge_reference([one_member], [0, 1])


def _items(rng, n, C, h, w):
    """Decoded items as ``Predictor._decode`` gives them for the CPU path: a non-symmetric random image each."""
    return [((h + 1, w + 2), rng.random((C, h, w), dtype=F32), False) for _ in range(n)]


def _tiny(seed, scale=4.0, **kw):
    from distributedpytorch_amd.models.unet import build_model
    torch.manual_seed(seed)
    model = build_model("unet-tiny", **kw)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(scale)
    return model


@pytest.mark.parametrize("spec", ["hflip", "vflip", "hflip+vflip+hvflip"])
def test_unmirror_pairing_with_pointwise_stub(spec):
    """A pointwise network commutes with a mirror, so every member mirrored back is the single-view result and the
    average is that result bit for bit; a member mirrored back by another code than its view's is not."""
    from distributedpytorch_amd.predict import Predictor

    def stub(x):
        """sigmoid(x[:, :1]) one element at a time: torch.sigmoid rounds a value differently in the vector body and
        in the scalar tail of a row, so IT does not commute with a mirror to the last bit."""
        z = x[:, :1].double().numpy()
        return torch.from_numpy(np.vectorize(lambda v: 1.0 / (1.0 + math.exp(-v)))(z).astype(F32))

    items = _items(np.random.default_rng(7), 3, 3, 6, 10)
    plain = Predictor(_tiny(0), "cpu", (6, 10), dtype="fp32", backend="torch")
    plain.strat.compute.probs = stub
    want = plain.merged_probs(list(items))
    assert want.dtype == torch.float32 and tuple(want.shape) == (3, 6, 10)
    pred = Predictor(_tiny(0), "cpu", (6, 10), dtype="fp32", backend="torch", tta=spec)
    pred.strat.compute.probs = stub
    assert pred.tta == spec and pred.members == len(K.tta_codes(spec)) and pred.host_post
    got = pred.merged_probs(list(items))
    assert got.dtype == torch.float32 and got.numpy().tobytes() == want.numpy().tobytes()
    assert not np.array_equal(want.numpy(), want.numpy()[:, :, ::-1]) and not np.array_equal(want.numpy(), want.numpy()[:, ::-1])


def test_default_path_is_one_probs_call():
    from distributedpytorch_amd.predict import Predictor
    pred = Predictor(_tiny(0), "cpu", (6, 10), dtype="fp32", backend="torch")
    assert pred.tta == "none" and pred.members == 1 and pred.tta_codes == [0]
    calls = []
    real = pred.probs
    pred.probs = lambda x: calls.append(x) or real(x)
    items = _items(np.random.default_rng(2), 2, 3, 6, 10)
    out = pred.merged_probs(list(items))
    assert len(calls) == 1 and np.array_equal(calls[0].numpy(), np.stack([it[1] for it in items]))
    assert np.array_equal(out.numpy(), real(calls[0]).numpy())


def test_member_order_with_real_models():
    """``hflip`` and one extra model: four forwards, checkpoint-major, each of the mirrored views in canonical order;
    the result is ``tta_merge_reference`` of exactly those outputs."""
    from distributedpytorch_amd.predict import Predictor
    m1, m2 = _tiny(3), _tiny(11)
    pred = Predictor(m1, "cpu", (8, 12), dtype="fp32", backend="torch", tta="hflip", extra_models=[m2])
    assert pred.members == 4 and len(pred.strats) == 2 and pred.strats[0] is pred.strat
    seen = []
    for k, strat in enumerate(pred.strats):
        def spy(x, k=k, real=strat.compute.probs):
            p = real(x)
            seen.append((k, x.clone(), p.clone()))
            return p
        strat.compute.probs = spy
    items = _items(np.random.default_rng(5), 2, 3, 8, 12)
    got = pred.merged_probs(list(items))
    x = torch.from_numpy(np.stack([it[1] for it in items]))
    assert [k for k, _, _ in seen] == [0, 0, 1, 1]
    for (_, xin, _), code in zip(seen, [0, 1, 0, 1]):
        assert torch.equal(xin, torch.flip(x, FLIPS[code]) if code else x)
    members = [p.float().reshape(2, 8, 12).numpy() for _, _, p in seen]
    assert not np.array_equal(members[0], members[2])                       # the second model is another one
    assert not np.array_equal(members[0], members[1][:, :, ::-1])           # a real net does not commute with a mirror
    want = K.tta_merge_reference(members, [0, 1, 0, 1])
    assert got.numpy().tobytes() == want.tobytes()
    assert want.tobytes() != K.tta_merge_reference(members, [0, 0, 1, 1]).tobytes()


def test_extra_model_of_other_channels_is_refused():
    from distributedpytorch_amd.predict import Predictor
    with pytest.raises(ValueError, match="input channels"):
        Predictor(_tiny(0), "cpu", (8, 12), dtype="fp32", backend="torch", extra_models=[_tiny(1, in_channels=1)])
    with pytest.raises(ValueError, match="'flop'"):
        Predictor(_tiny(0), "cpu", (8, 12), dtype="fp32", backend="torch", tta="flop")


# ---- the command-line tools (torch backend: run without a GPU) ------------------------------------------------
def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_tta_cli_end_to_end(setup, capsys):  # noqa: F811
    from distributedpytorch_amd.models.unet import build_model
    from distributedpytorch_amd.predict import Predictor, main, rle_string
    from distributedpytorch_amd.utils import load_model_state
    from distributedpytorch_amd.utils.checkpoint import save_model
    root, imgs, masks = setup
    save_model(_tiny(11), str(root / "checkpoints" / "tiny2.pth"))
    base = BASE + ["--out-dir", str(root), "--input", str(imgs), "--score", str(masks)]
    n0, _, (d0, _) = main(base + ["--rle", str(root / "t_none.csv"), "--tta", "none"])
    printed0 = capsys.readouterr().out
    n1, _, (d1, _) = main(base + ["--tta", "hflip", "--ensemble", "tiny2", "--rle", str(root / "t_tta.csv")])
    printed1 = capsys.readouterr().out
    assert n0 == n1 == 10 and "merged" not in printed0
    assert "merged (tta hflip): 2 views x 2 checkpoints" in printed1.splitlines()
    # an explicit path names the same checkpoint
    main(base + ["--tta", "hflip", "--ensemble", str(root / "checkpoints" / "tiny2.pth"), "--rle", str(root / "t_path.csv")])
    assert (root / "t_path.csv").read_bytes() == (root / "t_tta.csv").read_bytes()
    capsys.readouterr()

    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    models = []
    for name in ("tiny", "tiny2"):
        models.append(build_model("unet-tiny"))
        load_model_state(models[-1], str(root / "checkpoints" / f"{name}.pth"))
    files = sorted(str(p) for p in imgs.iterdir())
    plain = list(Predictor(models[0], dev, (16, 24), dtype="fp32", backend="torch").predict_files(files, 3))
    both = list(Predictor(models[0], dev, (16, 24), dtype="fp32", backend="torch", tta="hflip",
                          extra_models=[models[1]]).predict_files(files, 3))
    rows0, rows1 = _rows(root / "t_none.csv"), _rows(root / "t_tta.csv")
    assert rows0[0] == rows1[0] == ["img", "rle_mask"] and len(rows0) == len(rows1) == 11
    changed = 0
    for r0, r1, p, b in zip(rows0[1:], rows1[1:], plain, both):
        assert r0[0] == r1[0] == os.path.basename(p[0]) == os.path.basename(b[0])
        assert r0[1] == rle_string(K.rle_reference(p[2])) and r1[1] == rle_string(K.rle_reference(b[2]))
        assert r1[1] == rle_string(b[3])
        assert (r0[1] != r1[1]) == (not np.array_equal(p[2], b[2]))
        changed += int(r0[1] != r1[1])
    assert changed > 0 and d0[0] != d1[0]                        # averaging moved masks and the score

    # --host-post writes the same run lists, byte for byte
    main(base + ["--tta", "hflip", "--ensemble", "tiny2", "--rle", str(root / "t_host.csv"), "--host-post"])
    assert (root / "t_host.csv").read_bytes() == (root / "t_tta.csv").read_bytes()
    # tta alone: the line names one checkpoint
    main(base + ["--tta", "vflip+hflip"])
    assert "merged (tta hflip+vflip): 3 views x 1 checkpoints" in capsys.readouterr().out.splitlines()


def test_tta_argument_errors(setup, capsys):  # noqa: F811
    import evaluate
    from distributedpytorch_amd.predict import main
    root, imgs, masks = setup
    base = BASE + ["--out-dir", str(root), "--input", str(imgs), "--score", str(masks)]
    missing = os.path.join(str(root), "checkpoints", "missing.pth")
    for args, msg in ((["--ensemble", "missing"], f"--ensemble: checkpoint not found: {missing}"),
                      (["--ensemble", str(root / "nowhere" / "x.pth")], "checkpoint not found"),
                      (["--tta", "flip"], "unknown part 'flip'"), (["--tta", "hflip+"], "empty part")):
        with pytest.raises(SystemExit) as e:
            main(base + args)
        assert e.value.code == 2 and msg in capsys.readouterr().err, msg
    args = ["-c", "tiny", "--out-dir", str(root), "--model", "unet-tiny", "--img-size", "16", "24", "-b", "3",
            "--backend", "torch", "--dtype", "fp32", "--data-dir", str(root / "data"), "-v", "40"]
    with pytest.raises(SystemExit) as e:
        evaluate.main(args + ["--tta", "hflip"])
    assert e.value.code == 2 and "--tta hflip needs --full-res" in capsys.readouterr().err
    loss, dice, (fd, fi) = evaluate.main(args + ["--full-res", "--tta", "vflip+hflip"])
    out = capsys.readouterr().out
    assert "(4 images, threshold 0.5, tta hflip+vflip)" in out and 0.0 < fi < fd <= 1.0
    plain = evaluate.main(args + ["--full-res"])
    assert "tta" not in capsys.readouterr().out
    assert plain[:2] == (loss, dice) and plain[2] != (fd, fi)            # averaging moved the score
