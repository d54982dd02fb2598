"""Weight / bias gradients and the fused conv backward, bit for bit, on integer data (tests/exact_data.py).

``kernels.wgrad`` (conv3x3 through every path, transposed conv, the dense ``up`` form), ``wgrad_multi`` and
``conv_bwd_fused`` (masked / split / plain epilogues, dual input, the pool-folded and first-level modes) write
fp32 gradients that are sums of integer products below 2^24: exact in any summation order, under any split-K and
any slab reduction.  ``gw`` / ``gb`` start from integers (accumulate semantics) and must come out EQUAL to the
float64 reference; the fused backward's bf16 ``dx`` must equal its round-to-nearest-even rounding.  One case per
path has more than 4096 pixels and an odd row count, with a ragged last strip wherever the path admits a row
width that is not a strip multiple (the row-halo, dense-GEMM and band kernels only take whole 32 / 64-pixel
strips; their big cases end in a partial split instead).

Excluded: the head-folded and BatchNorm modes of ``conv_bwd_fused`` (a sigmoid / an rsqrt inside).
"""
import pytest
import torch

import exact_data as E
from test_hip_kernels import _pack_one

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# conv3x3 weight gradient: (id, N, H, W, Cin, Cout, padded Cin or None, path)
WGRAD_CASES = [
    # > 4096 pixels, odd row count (ragged last strip where the path takes one)
    ("auto-big-ragged", 2, 35, 120, 64, 128, None, "auto"),        # -> row-streaming, strips 64 + 56
    ("auto-big-band128", 2, 33, 64, 64, 128, None, "auto"),
    ("halo-big", 2, 33, 96, 32, 64, None, "halo"),
    ("stream-big-ragged", 2, 35, 120, 32, 64, None, "stream"),
    ("generic-big-ragged", 2, 35, 61, 32, 32, None, "generic"),
    ("gemm-big", 2, 33, 64, 64, 256, None, "gemm"),
    ("band-big", 2, 33, 64, 32, 256, None, "band"),
    ("band128-big", 2, 11, 192, 64, 128, None, "band128"),
    # small shapes: every tile family of each path
    ("auto-first-layer", 2, 9, 13, 3, 32, 8, "auto"), ("auto-deep-ragged", 2, 5, 100, 192, 128, None, "auto"),
    ("halo-32x32", 2, 5, 32, 32, 32, None, "halo"), ("halo-32x64", 2, 3, 64, 64, 32, None, "halo"),
    ("halo-64x32", 2, 3, 32, 32, 64, None, "halo"),
    ("stream-64", 2, 5, 64, 32, 32, None, "stream"), ("stream-32-strips", 2, 3, 96, 128, 64, None, "stream"),
    ("stream-ragged60", 2, 3, 60, 64, 128, None, "stream"), ("stream-first-layer", 2, 5, 128, 3, 32, 8, "stream"),
    ("stream-first-layer-ragged200", 2, 5, 200, 3, 32, 8, "stream"),
    ("generic-first-layer", 2, 9, 13, 3, 32, 8, "generic"), ("generic-64x32", 2, 9, 13, 64, 128, None, "generic"),
    ("generic-32x32", 2, 9, 13, 32, 96, None, "generic"),
    ("gemm-32wide", 2, 6, 32, 128, 256, None, "gemm"), ("gemm-deep", 2, 5, 64, 512, 256, None, "gemm"),
    ("band-32wide", 2, 6, 32, 64, 256, None, "band"), ("band-one-row", 2, 1, 64, 32, 512, None, "band"),
    ("band128-128wide", 2, 3, 128, 128, 128, None, "band128"), ("band128-256out", 2, 1, 64, 64, 256, None, "band128"),
]

# transposed-conv weight gradient (kind 1): (id, N, h, w, Cin, Cout, path)
DECONV_WGRAD_CASES = [
    ("cfg11", 2, 5, 7, 64, 32, "auto"), ("cfg12", 2, 5, 7, 64, 64, "auto"), ("cfg14", 2, 7, 9, 256, 128, "auto"),
    ("up-eligible", 16, 8, 16, 512, 256, "auto"),     # 16 x 8 tiles = 128 workgroups: the dense LDS-DMA form
    ("up-forced", 2, 8, 16, 256, 64, "up"),
]

# wgrad_multi: (id, images per tensor, H, W, Cin, Cout)
MULTI_CASES = [("stream", (2, 1), 5, 64, 32, 32), ("stream-first-layer", (1, 2), 5, 128, 3, 32),
               ("band", (1, 1), 4, 64, 32, 256), ("band128", (2, 2), 3, 64, 64, 128)]

# conv_bwd_fused: (id, N, H, W, Cin, Cout, epilogue, keywords)
BWD_CASES = [
    # target_blocks: 1 = whole image columns per block (the large-batch form), 12 = row segments 12 + 12 + 11;
    # the default at these batch sizes is one row per block
    ("plain-big-ragged", 2, 35, 120, 32, 64, "plain", dict(target_blocks=1)),
    ("plain-big-ragged-segments", 2, 35, 120, 32, 64, "plain", dict(target_blocks=12)),
    ("mask-big-ragged-rows", 2, 35, 120, 32, 64, "mask", {}),
    ("mask-32-32", 2, 5, 64, 32, 32, "mask", {}), ("mask-64-64-ragged120", 2, 5, 120, 64, 64, "mask", {}),
    ("mask-32-64", 2, 7, 192, 32, 64, "mask", {}), ("mask-64-32-rows", 2, 9, 128, 64, 32, "mask", dict(target_blocks=6)),
    ("split-64-32", 2, 5, 64, 64, 32, "split", {}), ("split-64-64-ragged240", 2, 3, 240, 64, 64, "split", {}),
    ("plain-64-64", 2, 3, 64, 64, 64, "plain", {}), ("mask-ragged60", 2, 3, 60, 32, 32, "mask", {}),
]
BWD_DUAL_CASES = [("dual-plain", 2, 5, 64, 64, 32, "plain", {}), ("dual-split-ragged120", 2, 3, 120, 64, 64, "split", {})]
# (id, N, H, W, target_blocks)
BWD_POOL_CASES = [("pool", 2, 6, 64, 0), ("pool-two-strips-whole-columns", 2, 4, 128, 1)]


def wgrad_amps(N, H, W):
    """Operand amplitudes of a conv3x3 weight-gradient case: the > 4096-pixel cases use x in [-3, 3] and g in
    [-2, 2] (an error that ternary data could cancel by sign symmetry shows), the small ones {-1, 0, 1}."""
    return dict(amp_x=3, amp_g=2) if N * H * W > 4096 else {}


def _ids(cases):
    return [c[0] for c in cases]


def _in(t_nchw, lead=0, trail=0):
    d = E.nhwc(t_nchw)
    N, H, W, C = d.shape
    return E.Guarded(N, H, W, C, BF, E.POISON, lead, trail, data=d)


def _flat(t):
    return E.GuardedFlat(t.numel(), torch.float32, E.SENTINEL, t)


def _done(what, *bufs):
    torch.cuda.synchronize()
    for b in bufs:
        b.check(what)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=_ids(WGRAD_CASES))
def test_conv_wgrad_exact(hip_lib, case):
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, Cin, Cout, cin_pad, path = case
    c = E.conv_wgrad_case(N, H, W, Cin, Cout, **wgrad_amps(N, H, W))
    Cs = cin_pad or Cin
    A, B = _in(c.g), _in(E.pad_channels(c.x, Cs))
    GW, GB = _flat(c.gw0), _flat(c.gb0)
    K.wgrad(A.view, B.view, kind=0, grid=(N, H, W), M=Cout, Nc=Cs, s=1, pad=1, KW=3, gw=GW.view, gb=GB.view, Nreal=Cin,
            path=path)
    _done(name, A, B, GW, GB)
    E.assert_exact(GW.view.view(Cout, Cin, 3, 3), c.gw.float(), f"wgrad {name} gw [co, ci, kh, kw]")
    E.assert_exact(GB.view, c.gb.float(), f"wgrad {name} gb")


@pytest.mark.parametrize("case", DECONV_WGRAD_CASES, ids=_ids(DECONV_WGRAD_CASES))
def test_deconv_wgrad_exact(hip_lib, case):
    """kind 1, the output gradient read from the second half of a concat gradient buffer."""
    from distributedpytorch_amd.ops import kernels as K
    name, N, h, w, Cin, Cout, path = case
    d = E.deconv_bwd_case("small", N, h, w, Cin, Cout)
    A, B = _in(d.g, lead=Cout, trail=8), _in(d.x)
    GW, GB = _flat(d.gw0), _flat(d.gb0)
    if path == "auto":
        assert K.wgrad_up_eligible(Cout, Cin, (N, h, w)) == (name == "up-eligible")
    K.wgrad(A.view, B.view, kind=1, grid=(N, h, w), M=Cout, Nc=Cin, s=2, pad=0, KW=2, gw=GW.view, gb=GB.view, Nreal=Cin,
            path=path)
    _done(name, A, B, GW, GB)
    E.assert_exact(GW.view.view(Cin, Cout, 2, 2), d.gw.float(), f"deconv wgrad {name} gw [ci, co, i, j]")
    E.assert_exact(GB.view, d.gb.float(), f"deconv wgrad {name} gb")


@pytest.mark.parametrize("case", MULTI_CASES, ids=_ids(MULTI_CASES))
def test_wgrad_multi_exact(hip_lib, case):
    """Several (gradient, input) tensor pairs in one launch == the gradient over all their images."""
    from distributedpytorch_amd.ops import kernels as K
    name, sizes, H, W, Cin, Cout = case
    N = sum(sizes)
    c = E.conv_wgrad_case(N, H, W, Cin, Cout, seed=1)
    Cs = K.round_up(Cin, 8)
    xs = E.pad_channels(c.x, Cs)
    As, Bs, n0 = [], [], 0
    for n in sizes:
        As.append(_in(c.g[n0:n0 + n]))
        Bs.append(_in(xs[n0:n0 + n]))
        n0 += n
    GW, GB = _flat(c.gw0), _flat(c.gb0)
    K.wgrad_multi([a.view for a in As], [b.view for b in Bs], M=Cout, Nc=Cs, gw=GW.view, gb=GB.view, Nreal=Cin)
    _done(name, GW, GB, *As, *Bs)
    E.assert_exact(GW.view.view(Cout, Cin, 3, 3), c.gw.float(), f"wgrad_multi {name} gw [co, ci, kh, kw]")
    E.assert_exact(GB.view, c.gb.float(), f"wgrad_multi {name} gb")


def _bwd_fused(K, name, regime, c, N, H, W, Cin, Cout, epi, kw, dual):
    wd, _, kd = _pack_one(1, c.w.float())
    G = _in(c.g)
    if dual:
        X, X2 = _in(c.x[:, :32]), _in(c.x[:, 32:])
        kw = dict(kw, x2=X2.view)
    else:
        X, X2 = _in(c.x), None
    GW, GB = _flat(c.gw0), _flat(c.gb0)
    bufs = [G, X, GW, GB] + ([X2] if dual else [])
    if epi == "split":
        s = Cin // 2
        LO = E.Guarded(N, H, W, s, BF, E.SENTINEL)
        HI = E.Guarded(N, H, W, Cin - s, BF, E.SENTINEL)
        K.conv_bwd_fused(G.view, X.view, wd, kd, GW.view, GB.view, mask=False, dx=LO.view, dx2=HI.view, split=s, **kw)
        _done(name, LO, HI, *bufs)
        got = torch.cat([LO.view, HI.view], dim=3)
        ref = c.dx
    else:
        DX = E.Guarded(N, H, W, Cin, BF, E.SENTINEL)
        K.conv_bwd_fused(G.view, X.view, wd, kd, GW.view, GB.view, mask=epi == "mask", dx=DX.view, **kw)
        _done(name, DX, *bufs)
        got = DX.view
        ref = c.dxm if epi == "mask" else c.dx
    E.assert_exact(got, E.bf16(E.nhwc(ref)), f"conv_bwd_fused {name} {regime} dx")
    E.assert_exact(GW.view.view(Cout, Cin, 3, 3), c.gw.float(), f"conv_bwd_fused {name} {regime} gw [co, ci, kh, kw]")
    E.assert_exact(GB.view, c.gb.float(), f"conv_bwd_fused {name} {regime} gb")


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("case", BWD_CASES, ids=_ids(BWD_CASES))
def test_conv_bwd_fused_exact(hip_lib, case, regime):
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, Cin, Cout, epi, kw = case
    _bwd_fused(K, name, regime, E.conv_bwd_case(regime, N, H, W, Cin, Cout), N, H, W, Cin, Cout, epi, kw, dual=False)


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("case", BWD_DUAL_CASES, ids=_ids(BWD_DUAL_CASES))
def test_conv_bwd_fused_dual_input_exact(hip_lib, case, regime):
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, Cin, Cout, epi, kw = case
    _bwd_fused(K, name, regime, E.conv_bwd_case(regime, N, H, W, Cin, Cout), N, H, W, Cin, Cout, epi, kw, dual=True)


@pytest.mark.parametrize("with_skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("case", BWD_POOL_CASES, ids=_ids(BWD_POOL_CASES))
def test_conv_bwd_fused_pool_mode_exact(hip_lib, case, with_skip):
    """The max-pool backward folded into the loader, from tie-rich window codes: dx (which rounds: gradients up
    to 96 through 288 taps), gw, gb against the float64 reference of pool routing + conv backward."""
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, tb = case
    C = 32
    c = E.conv_bwd_pool_case(N, H, W)
    r = c.skip if with_skip else c.noskip
    wd, _, kd = _pack_one(1, c.w.float())
    X, DP = _in(c.x), _in(c.pool.dpool)
    DS = _in(c.pool.dskip, lead=8, trail=24) if with_skip else None
    CD = E.Guarded(N, H // 2, W // 2, C, torch.uint8, E.CODE_SENTINEL, data=E.nhwc(c.pool.code))
    GW, GB = _flat(c.gw0), _flat(c.gb0)
    DX = E.Guarded(N, H, W, C, BF, E.SENTINEL)
    K.conv_bwd_fused(DS.view if with_skip else None, X.view, wd, kd, GW.view, GB.view, mask=True, dx=DX.view,
                     pool=(CD.view, DP.view), target_blocks=tb)
    _done(name, X, DP, CD, GW, GB, DX, *([DS] if with_skip else []))
    E.assert_exact(DX.view, E.bf16(E.nhwc(r.dxm)), f"pool-folded backward {name} dx")
    E.assert_exact(GW.view.view(C, C, 3, 3), r.gw.float(), f"pool-folded backward {name} gw")
    E.assert_exact(GB.view, r.gb.float(), f"pool-folded backward {name} gb")


@pytest.mark.parametrize("case", BWD_POOL_CASES, ids=_ids(BWD_POOL_CASES))
def test_conv_bwd_fused_first_level_exact(hip_lib, case):
    """First-level mode: conv2's gradients as in pool mode; conv1's weight / bias gradients from the unstored dx,
    which the kernel hands on as bf16 (as the unfused engine stores it): the reference rounds dx once to bf16
    and is exact from there.  Returns no dx."""
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, tb = case
    C = 32
    c = E.conv_bwd_pool_case(N, H, W)
    r = c.skip
    wd, _, kd = _pack_one(1, c.w.float())
    X, DP, DS, X1 = _in(c.x), _in(c.pool.dpool), _in(c.pool.dskip), _in(c.x1)
    CD = E.Guarded(N, H // 2, W // 2, C, torch.uint8, E.CODE_SENTINEL, data=E.nhwc(c.pool.code))
    GW, GB, GW1, GB1 = _flat(c.gw0), _flat(c.gb0), _flat(c.gw10), _flat(c.gb10)
    out = K.conv_bwd_fused(DS.view, X.view, wd, kd, GW.view, GB.view, mask=True, pool=(CD.view, DP.view),
                           w1=(X1.view, GW1.view, GB1.view), target_blocks=tb)
    _done(name, X, DP, DS, X1, CD, GW, GB, GW1, GB1)
    assert out is None
    E.assert_exact(GW.view.view(C, C, 3, 3), r.gw.float(), f"first-level backward {name} gw")
    E.assert_exact(GB.view, r.gb.float(), f"first-level backward {name} gb")
    E.assert_exact(GW1.view.view(C, 3, 3, 3), r.gw1.float(), f"first-level backward {name} conv1 gw")
    E.assert_exact(GB1.view, r.gb1.float(), f"first-level backward {name} conv1 gb")
