"""The exact-data helper (tests/exact_data.py) without a GPU.

Every case table of the GPU files (tests/test_exact_conv.py, test_exact_wgrad.py, test_exact_pool.py,
test_exact_fp32.py) goes through the generators and float64 references here, which asserts each case's
preconditions -- integer data, sums of |terms| below 2^24, ``small`` references exact in bf16, ``round``
references with at least 8 exact ties and 64 inexact outputs, tie-rich pool windows with every winner -- on the
CPU.  The float64 references themselves are anchored to fp32 torch autograd on ``randn`` data, the pool routing to
autograd of ``max_pool2d``, and ``assert_exact``'s failure report is checked on planted mismatches.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_data as E
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
