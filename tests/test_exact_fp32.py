"""The fp32 kernel family (ops/fp32.py, csrc/fp32.hip) on integer data: every output EQUAL to the float64 reference.

fp32 stores are exact and every partial sum is an integer below 2^24 -- in ``v_mfma_f32_16x16x4_f32`` accumulators
too -- so there is nothing to round and no tolerance: ``igemm`` (generic and halo form), every ``wgrad`` form (halo,
its two-halves variant, first-layer, big-tile, pixel-major), the transposed conv forward and backward, ``relu_bwd``
and ``channel_sum``.  Data: tests/exact_data.py ``f32_*_case`` (the ``small`` construction at amplitudes up to 2^10).
"""
import pytest
import torch

import exact_data as E

pytestmark = pytest.mark.gpu

F32T = torch.float32

# (id, N, H, W, Cin, Cout, padded Cin)
CONV_CASES = [
    ("first-layer", 2, 9, 13, 3, 32, 4), ("wide-128", 2, 9, 13, 64, 128, 64), ("odd-96", 2, 7, 11, 96, 64, 96),
    # the halo-staged narrow kernel's shapes (GEMM-N 32, or 64 with the halo switch at 2)
    ("halo-32-32", 2, 8, 32, 32, 32, 32), ("halo-64-64", 2, 8, 32, 64, 64, 64), ("halo-96-64", 2, 8, 64, 96, 64, 96),
    ("halo-odd-rows", 2, 7, 32, 32, 64, 32),
]
CONV_HALO_MODES = (0, 2)

# (id, N, H, W, Cin (B channels, padded), real Cin, Cout, switches)
WGRAD_CASES = [
    ("halo", 2, 8, 64, 32, 32, 32, dict(USE_WGRAD_HALO=True, WGRAD3_HALVES=False)),
    ("halo-64-whole", 2, 6, 32, 64, 64, 96, dict(USE_WGRAD_HALO=True, WGRAD3_HALVES=False)),
    ("halo-64-halves", 2, 6, 32, 64, 64, 96, dict(USE_WGRAD_HALO=True, WGRAD3_HALVES=True)),
    ("halo-big", 2, 34, 64, 32, 32, 64, dict(USE_WGRAD_HALO=True)),                    # 4352 pixels
    ("generic-big-odd", 2, 35, 61, 32, 32, 64, dict(USE_WGRAD_HALO=False)),            # 4270 pixels, odd rows and width
    ("first-layer-c4", 2, 5, 64, 4, 3, 32, dict(WGRAD_C4=True)),
    ("first-layer-generic", 2, 5, 64, 4, 3, 32, dict(WGRAD_C4=False)),
    ("first-layer-c4-192", 3, 5, 192, 4, 3, 32, dict(WGRAD_C4=True)),
    ("big-tile", 2, 8, 16, 256, 256, 256, dict(USE_WGRAD_BIG=True, target_blocks=7)),
    ("big-tile-ragged-columns", 2, 6, 10, 320, 320, 256, dict(USE_WGRAD_BIG=True, target_blocks=7)),
    ("pixel-major", 2, 5, 7, 96, 96, 32, dict(USE_WGRAD_HALO=False, WGRAD_PX=True, target_blocks=13)),
    ("transposing", 2, 5, 7, 96, 96, 32, dict(USE_WGRAD_HALO=False, WGRAD_PX=False, target_blocks=13)),
    ("pixel-major-128", 2, 8, 16, 64, 64, 128, dict(USE_WGRAD_HALO=False, WGRAD_PX=True, target_blocks=13)),
    ("transposing-128", 2, 8, 16, 64, 64, 128, dict(USE_WGRAD_HALO=False, WGRAD_PX=False, target_blocks=13)),
]

# (id, N, h, w, Cin, Cout)
DECONV_CASES = [("64-32", 2, 5, 7, 64, 32), ("256-128", 2, 3, 5, 256, 128)]


def _ids(cases):
    return [c[0] for c in cases]


def _in(t_nchw, lead=0, trail=0):
    d = E.nhwc(t_nchw)
    N, H, W, C = d.shape
    return E.Guarded(N, H, W, C, F32T, E.POISON, lead, trail, data=d)


def _out(N, H, W, C, lead=0, trail=0):
    return E.Guarded(N, H, W, C, F32T, E.SENTINEL, lead, trail)


def _flat(t):
    return E.GuardedFlat(t.numel(), F32T, E.SENTINEL, t)


def _done(what, *bufs):
    torch.cuda.synchronize()
    for b in bufs:
        b.check(what)


class _switches:
    """Set module-level dispatch switches of ops.fp32 for one block, restore them after."""

    def __init__(self, mod, **kw):
        self.mod, self.kw = mod, kw

    def __enter__(self):
        self.old = {k: getattr(self.mod, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.mod, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(self.mod, k, v)


@pytest.mark.parametrize("halo", CONV_HALO_MODES)
@pytest.mark.parametrize("case", CONV_CASES, ids=_ids(CONV_CASES))
def test_f32_conv_exact(hip_lib, case, halo):
    """Forward (bias + ReLU) and masked dgrad through the per-tap implicit GEMM (halo switch 0) and with the
    halo-staged narrow kernel enabled for GEMM-N 32 and 64 (switch 2)."""
    from distributedpytorch_amd.ops import fp32 as F32
    name, N, H, W, Cin, Cout, Cs = case
    c = E.f32_conv_case(N, H, W, Cin, Cout)
    wp, kp = F32.pack_conv_fwd(c.w.float().cuda(), Cs)
    X, Y = _in(E.pad_channels(c.x, Cs)), _out(N, H, W, Cout, lead=4, trail=8)
    with _switches(F32, CONV_HALO=halo):
        F32.igemm(X.view, wp, Y.view, Ngemm=Cout, Kpad=kp, KH=3, KW=3, stride=1, pad=1, Cs=Cs, out_grid=(N, H, W),
                  bias=c.b.float().cuda(), relu=True)
        _done(name, X, Y)
        E.assert_exact(Y.view, E.nhwc(c.y).float(), f"fp32 conv fwd {name} halo={halo}")
        if Cin % 32:
            return
        wd, kd = F32.pack_conv_dgrad(c.w.float().cuda())
        G, M, DX = _in(c.g, lead=4, trail=8), _in(c.xm), _out(N, H, W, Cin)
        F32.igemm(G.view, wd, DX.view, Ngemm=Cin, Kpad=kd, KH=3, KW=3, stride=1, pad=1, Cs=Cout, out_grid=(N, H, W),
                  mask=M.view)
        _done(name, G, M, DX)
        E.assert_exact(DX.view, E.nhwc(c.dxm).float(), f"fp32 conv dgrad {name} halo={halo}")


@pytest.mark.parametrize("case", WGRAD_CASES, ids=_ids(WGRAD_CASES))
def test_f32_wgrad_exact(hip_lib, case):
    from distributedpytorch_amd.ops import fp32 as F32
    name, N, H, W, Cs, Cin, Cout, sw = case
    sw = dict(sw)
    tb = sw.pop("target_blocks", 1024)
    c = E.f32_conv_case(N, H, W, Cin, Cout, seed=1)
    A, B = _in(c.g), _in(E.pad_channels(c.x, Cs))
    GW, GB = _flat(c.gw0), _flat(c.gb0)
    with _switches(F32, **sw):
        if sw.get("USE_WGRAD_BIG"):
            assert F32.wgrad_f32_tile(Cout, 9 * Cs, True) == (256, 256)
        F32.wgrad(A.view, B.view, GW.view, GB.view, KH=3, KW=3, s=1, pad=1, target_blocks=tb, nreal=Cin)
        _done(name, A, B, GW, GB)
    E.assert_exact(GW.view.view(Cout, Cin, 3, 3), c.gw.float(), f"fp32 wgrad {name} gw [co, ci, kh, kw]")
    E.assert_exact(GB.view, c.gb.float(), f"fp32 wgrad {name} gb")


@pytest.mark.parametrize("case", DECONV_CASES, ids=_ids(DECONV_CASES))
def test_f32_deconv_exact(hip_lib, case):
    """Transposed conv: the scatter forward into the upper half of a concat buffer; dgrad, weight gradient and
    bias gradient (``channel_sum``) reading the gradient from a concat half."""
    from distributedpytorch_amd.ops import fp32 as F32
    name, N, h, w, Cin, Cout = case
    c = E.f32_deconv_case(N, h, w, Cin, Cout)
    X, Y = _in(c.x), _out(N, 2 * h, 2 * w, Cout, lead=Cout, trail=4)
    F32.igemm(X.view, F32.pack_deconv_fwd(c.w.float().cuda()), Y.view, Ngemm=4 * Cout, Kpad=Cin, KH=1, KW=1, stride=1,
              pad=0, Cs=Cin, out_grid=(N, h, w), bias=c.b.float().cuda(), mode=1, Cout=Cout)
    _done(name, X, Y)
    E.assert_exact(Y.view, E.nhwc(c.y).float(), f"fp32 deconv fwd {name}")
    G, DX = _in(c.g, lead=Cout, trail=4), _out(N, h, w, Cin)
    F32.igemm(G.view, F32.pack_deconv_dgrad(c.w.float().cuda()), DX.view, Ngemm=Cin, Kpad=4 * Cout, KH=2, KW=2, stride=2,
              pad=0, Cs=Cout, out_grid=(N, h, w))
    GW, GB = _flat(c.gw0), _flat(c.gb0)
    F32.wgrad(X.view, G.view, GW.view, None, KH=2, KW=2, s=2, pad=0)
    F32.channel_sum(G.view, GB.view)
    _done(name, X, G, DX, GW, GB)
    E.assert_exact(DX.view, E.nhwc(c.dx).float(), f"fp32 deconv dgrad {name}")
    E.assert_exact(GW.view.view(Cin, Cout, 2, 2), c.gw.float(), f"fp32 deconv wgrad {name} gw [ci, co, i, j]")
    E.assert_exact(GB.view, c.gb.float(), f"fp32 deconv bias gradient (channel_sum) {name}")


@pytest.mark.parametrize("N,H,W,C", [(2, 7, 9, 32), (1, 33, 65, 16), (3, 1, 1, 4)])
def test_f32_relu_bwd_and_channel_sum_exact(hip_lib, N, H, W, C):
    from distributedpytorch_amd.ops import fp32 as F32
    gen = E.rng(N * H + C)
    g = E.integers(gen, (N, H, W, C), -1024, 1024)
    r = E.integers(gen, (N, H, W, C), -2, 2)
    out = F32.relu_bwd(g.float().cuda(), r.float().cuda())
    E.assert_exact(out, (g * (r > 0)).float(), "fp32 relu_bwd")
    assert float(g.abs().sum((0, 1, 2)).max()) + 8 < E.ACC_LIMIT
    G = E.Guarded(N, H, W, C, F32T, E.POISON, lead=4, trail=8, data=g)
    s0 = E.integers(gen, (C,), -8, 8)
    S = _flat(s0)
    F32.channel_sum(G.view, S.view)
    _done("channel_sum", G, S)
    E.assert_exact(S.view, (s0 + g.sum((0, 1, 2))).float(), "fp32 channel_sum of a channel slice")
