"""The exact-data helper (tests/exact_data.py) without a GPU.

Every case table of the GPU files (tests/test_exact_conv.py, test_exact_wgrad.py, test_exact_pool.py,
test_exact_fp32.py) goes through the generators and float64 references here, which asserts each case's
preconditions -- integer data, sums of |terms| below 2^24, ``small`` references exact in bf16, ``round``
references with at least 8 exact ties and 64 inexact outputs, tie-rich pool windows with every winner -- on the
CPU.  The float64 references themselves are anchored to fp32 torch autograd on ``randn`` data, the pool routing to
autograd of ``max_pool2d``, and ``assert_exact``'s failure report is checked on planted mismatches.  The block
references (tests/test_exact_blocks.py's tables) get the same two checks: preconditions in every regime used, and,
with rounding switched off, agreement with fp32 autograd of the same modules to 1e-5.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_data as E
import test_exact_blocks as TB
import test_exact_conv as TC
import test_exact_fp32 as TF
import test_exact_pool as TP
import test_exact_wgrad as TW


def _shape(case):
    return case[1:6]


@pytest.mark.parametrize("regime", E.REGIMES)
def test_conv_case_tables_meet_their_preconditions(regime):
    for case in TC.FWD_CASES + TC.DUAL_CASES + TC.POOL_CASES:
        c = E.conv_fwd_case(regime, *_shape(case))
        assert c.y.min() >= 0 and c.y.max() > 0
    for case in TC.DGRAD_CASES + TC.SPLIT_CASES:
        c = E.conv_dgrad_case(regime, *_shape(case))
        assert bool((c.x > 0).any()) and bool((c.x == 0).any()) and not torch.equal(c.dx, c.dxm)
    for case in TC.DECONV_IGEMM_CASES + TC.DECONV_FUSED_CASES:
        E.deconv_fwd_case(regime, *_shape(case))
        E.deconv_bwd_case(regime, *_shape(case))
    for case in TW.BWD_CASES + TW.BWD_DUAL_CASES:
        E.conv_bwd_case(regime, *_shape(case))


def test_round_regime_rounds_and_small_regime_does_not():
    """The two regimes differ where they should: the round references change under bf16 rounding (ties and
    inexact values both present), the small ones do not; a truncating or double-rounding epilogue would therefore
    differ from the round reference."""
    for case in (TC.FWD_CASES[0], TC.FWD_CASES[-1]):
        y = E.conv_fwd_case("round", *_shape(case)).y
        ties, inexact = E.rounding_census(y)
        assert ties >= 8 and inexact >= 64
        trunc = (y.float().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
        assert not torch.equal(trunc, E.bf16(y)), "truncation must be distinguishable from round-to-nearest-even"
        ys = E.conv_fwd_case("small", *_shape(case)).y
        assert E.rounding_census(ys) == (0, 0) and float(ys.abs().max()) <= 64


def test_rounding_census_counts_ties_and_inexact_values():
    # bf16 keeps 8 significant bits: 257 is a tie between 256 and 258, 259 a tie, 258 exact, 513 inexact (not a tie)
    t = torch.tensor([256.0, 257.0, 258.0, 259.0, 513.0, 514.0, 1.0, -257.0], dtype=torch.float64)
    assert E.rounding_census(t) == (4, 5)
    assert E.bf16(torch.tensor([257.0, 259.0, -257.0])).tolist() == [256.0, 260.0, -256.0]   # ties to even


def test_wgrad_case_tables_meet_their_preconditions():
    for case in TW.WGRAD_CASES:
        name, N, H, W, Cin, Cout, cin_pad, path = case
        c = E.conv_wgrad_case(N, H, W, Cin, Cout, **TW.wgrad_amps(N, H, W))
        assert float(c.x.abs().max()) == (3 if N * H * W > 4096 else 1)
        assert torch.equal(c.gw, c.gw.round()) and float(c.gw.abs().max()) < E.ACC_LIMIT
        assert not torch.equal(c.gw, c.gw0)
    big = {}
    for case in TW.WGRAD_CASES:
        name, N, H, W, Cin, Cout, cin_pad, path = case
        if N * H * W > 4096 and H % 2 == 1:
            big.setdefault(path, []).append(W)
    assert set(big) == {"auto", "halo", "stream", "generic", "gemm", "band", "band128"}, sorted(big)
    # a ragged last strip wherever the path takes a width that is not a multiple of its 32 / 64-pixel strips
    assert all(any(w % 32 for w in big[p]) for p in ("auto", "stream", "generic"))
    for case in TW.DECONV_WGRAD_CASES:
        E.deconv_bwd_case("small", *_shape(case))
    for name, sizes, H, W, Cin, Cout in TW.MULTI_CASES:
        E.conv_wgrad_case(sum(sizes), H, W, Cin, Cout, seed=1)
    assert any(N * H * W > 4096 and H % 2 == 1 and W % 64 for _, N, H, W, *_ in TW.BWD_CASES)


def test_pool_case_tables_meet_their_preconditions():
    for N, H, W, C in TP.POOL_CASES + TP.POOL_ODD_CASES + TP.F32_POOL_CASES:
        c = E.pool_case(N, H, W, C)
        assert float(c.dpool.abs().min()) > 0 and float((c.dskip + c.routed).abs().max()) <= 256   # exact in bf16
        E.require_small(c.g, "pool gradient")
    for shape in TP.CONV_POOL_CASES:
        E.conv_pool_case(*shape)
    for name, N, H, W, tb in TW.BWD_POOL_CASES:
        c = E.conv_bwd_pool_case(N, H, W)
        ties, inexact = E.rounding_census(c.skip.dxm)
        assert ties >= 8 and inexact >= 64          # the pool-folded dx exercises the rounding too
        assert not torch.equal(c.skip.gw1, c.gw10)


def test_fp32_case_tables_meet_their_preconditions():
    for name, N, H, W, Cin, Cout, Cs in TF.CONV_CASES:
        c = E.f32_conv_case(N, H, W, Cin, Cout)
        assert torch.equal(c.y.float().double(), c.y) and float(c.x.abs().max()) == 32 and float(c.b.abs().max()) > 512
    for name, N, H, W, Cs, Cin, Cout, sw in TF.WGRAD_CASES:
        c = E.f32_conv_case(N, H, W, Cin, Cout, seed=1)
        assert torch.equal(c.gw.float().double(), c.gw)
    for case in TF.DECONV_CASES:
        E.f32_deconv_case(*_shape(case))


def test_block_case_tables_meet_their_preconditions():
    """Every case of tests/test_exact_blocks.py, in the regime it is used in: the builders assert integers, every
    forward / dgrad / weight-gradient sum of |terms| below 2^24, ``small`` stored tensors exact in bf16, ``round``
    outputs with ties and inexact values, live ReLUs and non-trivial gradients."""
    for case in TB.ENC_CASES:
        c = TB.enc_case(case)
        assert (c.dx is None) == (case[1] == 0) and (c.code is None) == bool(c.x.shape[2] % 2 or c.x.shape[3] % 2)
        assert float((c.dskip.abs() + E.pool_route(c.dpooled.abs(), c.q, *c.y.shape[2:])).max()) <= 128   # exact in bf16
    for case in TB.MID_CASES:
        c = TB.mid_case(case)
        assert torch.equal(c.g, c.g * (c.y > 0)) and bool((c.g != 0).any())
    for case in TB.DEC_CASES:
        c = TB.dec_case(case)
        if case[7]:
            (Hs, Ws), (top, left) = case[7], c.crop
            assert tuple(c.dskip.shape[2:]) == (Hs, Ws) and (top, left) == E.crop_offsets(Hs, Ws, *c.y.shape[2:])
            win = torch.zeros_like(c.dskip)
            win[:, :, top:top + c.y.shape[2], left:left + c.y.shape[3]] = 1
            assert not bool((c.dskip * (1 - win)).any()) and bool((c.dskip * win).any())
    for case in TB.HALF_CASES:
        TB.half_case(case)
    for case in TB.DEFER_CASES:
        c = TB.defer_case(case)
        assert c.x.shape[0] == sum(TB.DEFER_SIZES) and c.dx is not None
    small, rnd = E.trunk_case("small", *TB.TRUNK), E.trunk_case("round", *TB.TRUNK)
    assert len(small.G) == 46 and torch.equal(small.G["segmap.bias"], small.G0["segmap.bias"])
    assert max(float(t.abs().max()) for t in small.stored.values()) <= 256
    assert max(float(t.abs().max()) for t in rnd.stored.values()) > 256
    # every regime a block kind is used in rounds where it says it does
    for c in (TB.enc_case(TB.ENC_CASES[6]), TB.mid_case(TB.MID_CASES[1]), TB.dec_case(TB.DEC_CASES[6])):
        assert E.rounding_census(c.raw.a)[1] >= 64 and E.rounding_census(c.raw.y)[0] >= 8
        assert E.rounding_census(c.raw.g1)[1] >= 64, "the stored gradient between the two convs must round"
        assert not torch.equal(E.bf16(c.raw.dx).double(), c.raw.dx)


def _close(a, b, tol):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item() < tol


def test_float64_references_match_fp32_autograd_on_randn():
    """The reference functions the case builders use, against independent fp32 torch formulations."""
    g = E.rng(3)
    x, w, b = torch.randn(2, 5, 7, 9, generator=g), torch.randn(6, 5, 3, 3, generator=g), torch.randn(6, generator=g)
    gy = torch.randn(2, 6, 7, 9, generator=g)
    assert _close(E.conv_fwd_ref(x.double(), w.double(), b.double()), F.relu(F.conv2d(x, w, b, padding=1)), 1e-5)
    dx, dw, db = E.conv_grads_ref(x.double(), w.double(), gy.double())
    assert _close(dx, torch.nn.grad.conv2d_input(x.shape, w, gy, padding=1), 1e-5)
    assert _close(dw, torch.nn.grad.conv2d_weight(x, w.shape, gy, padding=1), 1e-5)
    assert _close(db, gy.sum((0, 2, 3)), 1e-5)
    # transposed conv k2 s2: y[2h+i][2w+j][co] = b[co] + sum_ci x[h][w][ci] w[ci][co][i][j], written out
    xt, wt, bt = torch.randn(2, 5, 3, 4, generator=g), torch.randn(5, 6, 2, 2, generator=g), torch.randn(6, generator=g)
    gt = torch.randn(2, 6, 6, 8, generator=g)
    y = torch.einsum("nchw,cdij->ndhiwj", xt, wt).reshape(2, 6, 6, 8) + bt.view(1, -1, 1, 1)
    assert _close(E.deconv_fwd_ref(xt.double(), wt.double(), bt.double()), y, 1e-5)
    dx, dw, db = E.deconv_grads_ref(xt.double(), wt.double(), gt.double())
    g6 = gt.reshape(2, 6, 3, 2, 4, 2)
    assert _close(dx, torch.einsum("ndhiwj,cdij->nchw", g6, wt), 1e-5)
    assert _close(dw, torch.einsum("nchw,ndhiwj->cdij", xt, g6), 1e-5)
    assert _close(db, gt.sum((0, 2, 3)), 1e-5)


@pytest.mark.parametrize("H,W", [(6, 8), (7, 9)])
def test_pool_reference_matches_autograd_and_the_first_maximum_rule(H, W):
    g = E.rng(H)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    p = F.max_pool2d(x, 2, 2)
    dp = torch.randn(p.shape, generator=g, dtype=torch.float64)
    (dx,) = torch.autograd.grad(p, x, dp)
    pooled, q = E.pool_ref(x.detach())
    assert torch.equal(pooled, p.detach()) and torch.equal(E.pool_route(dp, q, H, W), dx)
    # ties: the first maximum in scan order tl, tr, bl, br
    t = torch.tensor([[[[2.0, 2.0, 1.0, 3.0, 0.0, 0.0, 1.0, 2.0], [2.0, 2.0, 3.0, 3.0, 0.0, 0.0, 2.0, 2.0]]]],
                     dtype=torch.float64)
    _, q = E.pool_ref(t)
    assert q.flatten().tolist() == [0, 1, 0, 1]
    code = E.pool_codes_ref(t).flatten().tolist()
    assert code == [0 | 0b1111 << 2, 1 | 0b1111 << 2, 0, 1 | 0b1111 << 2]


def test_assert_exact_locates_mismatches():
    ref = torch.arange(2 * 3 * 130 * 16, dtype=torch.float32).reshape(2, 3, 130, 16).to(torch.bfloat16)
    E.assert_exact(ref.clone(), ref, "same")
    E.assert_exact(torch.tensor([0.0, -0.0]), torch.tensor([-0.0, 0.0]), "signed zeros compare equal")
    got = ref.clone()
    got[1, 2, 129, 15] += 64.0             # last image, last row, last column, last channel
    got[0, 0, 64, 3] = float("nan")
    with pytest.raises(AssertionError) as e:
        E.assert_exact(got, ref, "planted")
    msg = str(e.value)
    assert "planted: 2 of" in msg and "(0, 0, 64, 3)" in msg and "(1, 2, 129, 15)" in msg
    assert "w mod 64: {0: 1, 1: 1}" in msg and "w mod 128: {1: 1, 64: 1}" in msg
    assert "first row: 1, last row: 1" in msg and "last column: 1" in msg and "last 8 channels: 1" in msg
    assert "per image: [1, 1]" in msg
    with pytest.raises(AssertionError):
        E.assert_exact(ref.float(), ref, "dtype")
    flat = torch.zeros(10)
    with pytest.raises(AssertionError) as e:
        E.assert_exact(flat + torch.eye(10)[3], flat, "flat")
    assert "index (3,)" in str(e.value)


def test_guarded_buffers_detect_overruns_on_the_cpu():
    G = E.Guarded(2, 3, 4, 8, torch.bfloat16, E.SENTINEL, lead=8, trail=8, device="cpu")
    assert tuple(G.view.shape) == (2, 3, 4, 8) and G.view.stride(2) == 24 and bool((G.view == E.SENTINEL).all())
    G.view.zero_()
    G.check("inside the view")
    G.buf[0, 2, 3, 9] = 1.0                # the image before the view
    with pytest.raises(AssertionError):
        G.check("guard image")
    G = E.Guarded(1, 2, 2, 8, torch.float32, E.POISON, trail=4, data=torch.ones(1, 2, 2, 8, dtype=torch.float64), device="cpu")
    G.check("untouched input")
    G.buf[1, 0, 0, 8] = 0.0                # a guard channel
    with pytest.raises(AssertionError):
        G.check("guard channel")
    Fl = E.GuardedFlat(5, torch.float32, E.SENTINEL, torch.arange(5.0), device="cpu")
    Fl.check("flat")
    Fl.buf[64 + 5] = 0.0
    with pytest.raises(AssertionError):
        Fl.check("flat overrun")


def _randn_double_conv(g, cin, cmid, cout):
    return (torch.randn(cmid, cin, 3, 3, generator=g), torch.randn(cmid, generator=g),
            torch.randn(cout, cmid, 3, 3, generator=g), torch.randn(cout, generator=g))


def _leaves(*ts):
    return [t.clone().requires_grad_(True) for t in ts]


def test_block_references_match_fp32_autograd_on_randn():
    """The float64 block references with every rounding switched off against plain fp32 autograd of the same
    modules (conv -> ReLU -> conv -> ReLU, max-pool, ConvTranspose2d + centre crop + cat), to 1e-5 relative: the
    masking conventions of the engines are then the only thing the references add."""
    g = E.rng(5)
    D = lambda *ts: [t.double() for t in ts]   # noqa: E731
    # encoder block 5 -> 6 at 6 x 7 (odd width: the last column is outside the pooled area)
    x = torch.randn(2, 5, 6, 7, generator=g)
    P = _randn_double_conv(g, 5, 6, 6)
    dskip, dpooled = torch.randn(2, 6, 6, 7, generator=g), torch.randn(2, 6, 3, 3, generator=g)
    xl, *pl = _leaves(x, *P)
    y = F.relu(F.conv2d(F.relu(F.conv2d(xl, pl[0], pl[1], padding=1)), pl[2], pl[3], padding=1))
    pooled = F.max_pool2d(y, 2, 2)
    grads = torch.autograd.grad([y, pooled], [xl] + pl, [dskip, dpooled], retain_graph=True)
    r = E.enc_block_ref(*D(x, *P, dskip, dpooled), rnd=False)
    assert _close(r.y, y, 1e-5) and _close(r.pooled, pooled, 1e-5)
    for got, ref in zip((r.dx, r.dw1, r.db1, r.dw2, r.db2), grads):
        assert _close(got, ref, 1e-5)
    # DoubleConv from an already-masked output gradient
    gy = torch.randn(2, 6, 6, 7, generator=g)
    a64, y64 = E.double_conv_fwd_ref(*D(x, *P), rnd=False)
    r = E.double_conv_bwd_ref(x.double(), a64, P[0].double(), P[2].double(), gy.double() * (y64 > 0), rnd=False)
    grads = torch.autograd.grad(y, [xl] + pl, gy)
    for got, ref in zip((r.dx, r.dw1, r.db1, r.dw2, r.db2), grads):
        assert _close(got, ref, 1e-5)
    # decoder block 8 -> 4 with an 8 x 13 skip cropped to 6 x 10 at (1, 2); x is a ReLU output (dx masked by x > 0)
    x0, skip = torch.randn(2, 8, 3, 5, generator=g), torch.randn(2, 4, 8, 13, generator=g)
    wt, bt = torch.randn(8, 4, 2, 2, generator=g), torch.randn(4, generator=g)
    P = _randn_double_conv(g, 8, 4, 4)
    gy = torch.randn(2, 4, 6, 10, generator=g)
    x0l, sl, wtl, btl, *pl = _leaves(x0, skip, wt, bt, *P)
    up = F.conv_transpose2d(F.relu(x0l), wtl, btl, stride=2)
    top, left = E.crop_offsets(8, 13, 6, 10)
    assert (top, left) == (1, 2) and E.crop_offsets(7, 11, 6, 10) == (0, 0)           # Python rounds 1.5 and 0.5 to even
    cat = torch.cat([sl[:, :, top:top + 6, left:left + 10], up], 1)
    y = F.relu(F.conv2d(F.relu(F.conv2d(cat, pl[0], pl[1], padding=1)), pl[2], pl[3], padding=1))
    grads = torch.autograd.grad(y, [x0l, sl, wtl, btl] + pl, gy)
    r = E.dec_block_ref(*D(F.relu(x0), skip, wt, bt, *P, gy), rnd=False)
    assert _close(r.y, y, 1e-5)
    for got, ref in zip((r.dx, r.dskip, r.dwt, r.dbt, r.dw1, r.db1, r.dw2, r.db2), grads):
        assert _close(got, ref, 1e-5)
    assert not bool(r.dskip[:, :, 0].any()) and not bool(r.dskip[:, :, 7:].any()) and not bool(r.dskip[:, :, :, :2].any()) \
        and not bool(r.dskip[:, :, :, 12:].any()) and bool(r.dskip[:, :, 1:7, 2:12].any())


def test_trunk_reference_matches_fp32_autograd_of_the_model():
    """``trunk_ref`` without rounding against fp32 autograd of the ``unet`` modules themselves (encoder, mid,
    decoder; no head) on randn parameters: every parameter gradient and the output, to 1e-5 relative."""
    from distributedpytorch_amd.models.unet import build_model
    torch.manual_seed(7)
    net = build_model("unet")
    g = E.rng(7)
    img = torch.randn(1, 3, 16, 32, generator=g)
    x, *skips = net.encoder(img)
    y = net.decoder(net.mid(x), *skips)
    gy = torch.randn(y.shape, generator=g)
    names = [n for n, _ in net.named_parameters() if not n.startswith("segmap")]
    params = dict(net.named_parameters())
    assert [p for p, _ in E.trunk_names()] == sorted({n.rsplit(".", 1)[0] for n in names}, key=[p for p, _ in E.trunk_names()].index)
    grads = torch.autograd.grad(y, [params[n] for n in names], gy)
    P = {n: params[n].detach().double() for n in names}
    stored, ref = E.trunk_ref(P, img.double(), gy.double(), rnd=False)
    assert _close(stored["dec3.y"], y, 1e-5)
    for n, got in zip(names, grads):
        assert _close(ref[n], got, 1e-5), n
