"""bf16 conv / transposed-conv kernels, bit for bit, on integer data (tests/exact_data.py).

Every path ``kernels.igemm`` can take (generic gather cfg 0-7, row-streaming, row-halo, LDS-DMA variants and
each automatic row-block form), ``deconv_fwd_fused`` and ``deconv_bwd_fused`` are run on data whose exact
result is known: the stored bf16 output must equal ``round_to_nearest_even_bf16`` of the float64 reference,
``torch.equal``, in the ``small`` regime (nothing rounds: pure indexing) and the ``round`` regime (outputs
with more than 8 significant bits, exact ties included).  Inputs and outputs are slices of larger owned
buffers: finite poison around the inputs, a sentinel around and under the outputs; the guards must survive.

``accumulate=True`` has no caller in the package and is not covered.

The case tables are module-level so that tests/test_exact_data_cpu.py can prove every case's preconditions
without a GPU.
"""
import pytest
import torch

import exact_data as E
from test_hip_kernels import _pack_one

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# (id, N, H, W, Cin, Cout, igemm keywords)  -- forward conv3x3 + bias + ReLU
FWD_CASES = [
    # generic gather kernel (csrc/igemm.hip): 270 pixels = full and partial 64 / 128 / 256-pixel tiles
    ("generic-first-layer", 2, 9, 15, 3, 32, dict(path="generic")),        # Cs = 8, K = 72 in Kpad = 96 -> cfg 5
    ("generic-k32", 2, 9, 15, 32, 64, dict(path="generic")),               # Kpad = 288 -> cfg 3
    ("generic-cfg1", 2, 9, 15, 64, 128, dict(cfg=1)), ("generic-cfg2", 2, 9, 15, 64, 128, dict(cfg=2)),
    ("generic-cfg3", 2, 9, 15, 64, 64, dict(cfg=3)), ("generic-cfg4", 2, 9, 15, 64, 64, dict(cfg=4)),
    ("generic-cfg5", 2, 9, 15, 64, 32, dict(cfg=5)), ("generic-cfg6", 2, 9, 15, 64, 32, dict(cfg=6)),
    ("generic-cfg7", 2, 9, 15, 64, 128, dict(cfg=7)),
    # row-streaming kernel (csrc/halo.hip): 128-pixel strips (variants 1, 3), 64-pixel strips (2, 4), ragged rows
    ("stream-128", 2, 5, 128, 32, 32, dict(path="stream", variant=1)),
    ("stream-128-ragged200", 2, 3, 200, 64, 64, dict(path="stream", variant=1)),
    ("stream-128-v3", 2, 5, 128, 64, 32, dict(path="stream", variant=3)),
    ("stream-64", 2, 5, 64, 64, 32, dict(path="stream", variant=2)),
    ("stream-64-ragged96", 2, 3, 96, 32, 64, dict(path="stream", variant=2)),
    ("stream-64-v4", 2, 5, 64, 32, 64, dict(path="stream", variant=4)),
    ("stream-auto-ragged96", 2, 5, 96, 32, 32, dict(path="stream")),
    ("stream-auto-ragged120", 2, 5, 120, 64, 64, dict(path="stream")),
    # ... its first-layer form (Cs = 8) for 32 and 64 outputs
    ("stream8-32", 2, 5, 128, 3, 32, dict(path="stream")), ("stream8-64", 2, 5, 128, 3, 64, dict(path="stream")),
    ("stream8-32-ragged200", 2, 5, 200, 3, 32, dict(path="stream")),
    ("stream8-64-ragged200", 2, 3, 200, 3, 64, dict(path="stream")),
    # row-halo kernel: whole and ragged tiles, one- and two-row forms
    ("halo-256", 2, 3, 256, 32, 32, dict(path="halo")), ("halo-ragged240-c32", 2, 3, 240, 32, 32, dict(path="halo")),
    ("halo-128", 2, 5, 128, 64, 64, dict(path="halo")), ("halo-ragged120", 2, 3, 120, 128, 128, dict(path="halo")),
    ("halo-ragged240", 2, 3, 240, 64, 128, dict(path="halo")),
    ("halo-ragged120-cfg3", 2, 3, 120, 32, 32, dict(path="halo", variant=3)),
    # LDS-DMA GEMMs (csrc/igemm_glds.hip): 234 pixels = zero-filled DMA rows in the last tile
    ("glds-v0", 2, 9, 13, 64, 256, dict(path="glds", variant=0)), ("glds-v1", 2, 9, 13, 128, 256, dict(path="glds", variant=1)),
    ("glds-v2", 2, 9, 13, 64, 128, dict(path="glds", variant=2)), ("glds-v4", 2, 7, 11, 128, 128, dict(path="glds", variant=4)),
    ("glds-v8", 2, 9, 13, 128, 256, dict(path="glds", variant=8)), ("glds-v14", 2, 9, 13, 128, 256, dict(path="glds", variant=14)),
    # the 256-channel row-block kernel (igemm_pp2h_kernel<EP, 256>) and, with the slp256 switch, the slice-staged
    # ping-pong kernel that replaces it (igemm_slp_kernel<EP, 256>); the library refuses a forced variant it cannot run
    ("glds-v14-rowblock", 2, 8, 32, 64, 256, dict(path="glds", variant=14)),
    ("glds-v14-slp256", 2, 8, 32, 64, 256, dict(path="glds", variant=14, slp256=True)),
    # the 128- and 64-channel row-block forms, forced: cfg 15, slice-staged cfg 18, slice-staged ping-pong cfg 19
    ("glds-v15-rb128", 2, 8, 32, 64, 128, dict(path="glds", variant=15)),
    ("glds-sl128", 2, 16, 32, 64, 128, dict(path="glds", variant=262144)),
    ("glds-slp64", 2, 16, 32, 128, 64, dict(path="glds", variant=524288)),
    # the automatic row-block forms, at the smallest shapes their predicates admit (ops/kernels.py igemm)
    ("auto-rb128", 2, 8, 32, 64, 128, dict()),            # H W = 256: row-block cfg 15
    ("auto-rb128-sliced", 2, 16, 32, 64, 128, dict()),    # H W = 512: slice-staged cfg 18
    ("auto-slp64", 2, 16, 32, 128, 64, dict()),           # 64 outputs from 128 (64 -> 64 is the stream kernel's)
    # 256 outputs on a grid this small: the library's automatic choice is the plain 128 x 128 tile (cfg 4), not a
    # row-block form (those need >= 512 tiles); the 256-channel row-block kernels are the forced glds-v14 rows
    ("auto-256-small-grid", 2, 8, 32, 64, 256, dict()),
    ("auto-256-small-grid-deep", 2, 16, 32, 128, 256, dict()),
]

# (id, N, H, W, Cin, Cout, igemm keywords)  -- dgrad (GEMM-N = Cin, Cs = Cout), masked by the layer input's ReLU support
DGRAD_CASES = [
    ("generic", 2, 9, 15, 64, 32, dict(path="generic")), ("generic-128", 2, 9, 15, 128, 64, dict(path="generic")),
    ("stream", 2, 5, 128, 32, 32, dict(path="stream")), ("stream-ragged96", 2, 3, 96, 64, 32, dict(path="stream")),
    ("stream-ragged120", 2, 3, 120, 64, 64, dict(path="stream")), ("stream-64", 2, 5, 64, 32, 64, dict(path="stream")),
    ("halo-ragged240", 2, 3, 240, 128, 64, dict(path="halo")), ("halo-ragged120", 2, 3, 120, 128, 128, dict(path="halo")),
    ("halo-256", 2, 3, 256, 64, 32, dict(path="halo")),
    ("glds-v2", 2, 9, 13, 128, 256, dict(path="glds", variant=2)), ("glds-v4", 2, 7, 11, 128, 128, dict(path="glds", variant=4)),
    ("glds-v1", 2, 9, 13, 256, 128, dict(path="glds", variant=1)), ("glds-v8", 2, 9, 13, 256, 128, dict(path="glds", variant=8)),
    ("glds-v14", 2, 9, 13, 256, 128, dict(path="glds", variant=14)), ("glds-v0", 2, 9, 13, 256, 64, dict(path="glds", variant=0)),
    ("auto-rb128", 2, 8, 32, 128, 64, dict()), ("auto-rb128-sliced", 2, 16, 32, 128, 64, dict()),
    ("auto-slp64", 2, 16, 32, 64, 128, dict()), ("auto-256-small-grid", 2, 8, 32, 256, 64, dict()),      # -> cfg 4
    # forced row-block forms: the masked-dgrad epilogue of the 256-channel row-block / slice-staged ping-pong kernels,
    # cfg 15, cfg 18, cfg 19
    ("glds-v14-rowblock", 2, 8, 32, 256, 64, dict(path="glds", variant=14)),
    ("glds-v14-slp256", 2, 8, 32, 256, 64, dict(path="glds", variant=14, slp256=True)),
    ("glds-v15-rb128", 2, 8, 32, 128, 64, dict(path="glds", variant=15)),
    ("glds-sl128", 2, 16, 32, 128, 64, dict(path="glds", variant=262144)),
    ("glds-slp64", 2, 16, 32, 64, 128, dict(path="glds", variant=524288)),
]

# dgrad with the output split into the two dense halves of a concat gradient (y2 / split), unmasked
SPLIT_CASES = [
    ("generic", 2, 9, 15, 128, 64, dict(path="generic")), ("stream-ragged96", 2, 3, 96, 64, 32, dict(path="stream")),
    ("halo-ragged240", 2, 3, 240, 128, 64, dict(path="halo")), ("glds", 2, 9, 13, 256, 128, dict(path="glds")),
    ("auto-rb128", 2, 8, 32, 128, 64, dict()), ("auto-256-small-grid", 2, 8, 32, 256, 64, dict()),       # -> cfg 4
    # forced row-block forms: the split epilogue of the 256-channel kernels, cfg 15 and cfg 18
    ("glds-v14-rowblock", 2, 8, 32, 256, 64, dict(path="glds", variant=14)),
    ("glds-v14-slp256", 2, 8, 32, 256, 64, dict(path="glds", variant=14, slp256=True)),
    ("glds-v15-rb128", 2, 8, 32, 128, 64, dict(path="glds", variant=15)),
    ("glds-sl128", 2, 16, 32, 128, 64, dict(path="glds", variant=262144)),
]

# dual input: the conv input is [x | x2], two 32-channel tensors (row-streaming kernel only)
DUAL_CASES = [("dual-32", 2, 5, 96, 64, 32, dict(path="stream")), ("dual-64", 2, 3, 128, 64, 64, dict())]

# forward + 2x2 max-pool + window codes, the conv output a concat half: fused into the row-streaming epilogue
# (Cin == Cout), or the separate pool pass the wrapper runs after any other kernel (auto)
POOL_CASES = [("stream-32", 2, 5, 128, 32, 32, dict(path="stream")), ("stream-ragged96", 2, 6, 96, 64, 64, dict(path="stream")),
              ("stream-64-strips", 2, 9, 64, 32, 32, dict(path="stream", variant=2)), ("separate-stream-conv", 2, 9, 64, 32, 64, dict()),
              ("separate", 2, 6, 14, 64, 128, dict())]

# transposed conv k2 s2: (id, N, h, w, Cin, Cout)
DECONV_IGEMM_CASES = [("generic", 2, 5, 7, 32, 32), ("glds", 2, 5, 7, 64, 32), ("glds-deep", 2, 3, 5, 256, 128)]
DECONV_FUSED_CASES = [("64-32", 2, 5, 7, 64, 32), ("128-64", 2, 9, 11, 128, 64)]


def _ids(cases):
    return [c[0] for c in cases]


def _in(t_nchw, lead=0, trail=0):
    """A guarded bf16 NHWC input (poison around it) from an NCHW float64 tensor."""
    d = E.nhwc(t_nchw)
    N, H, W, C = d.shape
    return E.Guarded(N, H, W, C, BF, E.POISON, lead, trail, data=d)


def _out(N, H, W, C, lead=0, trail=0, dtype=BF, fill=E.SENTINEL):
    return E.Guarded(N, H, W, C, dtype, fill, lead, trail)


def _expect(t_nchw):
    return E.bf16(E.nhwc(t_nchw))


class _slp256:
    """Run a block with the library's slp256 switch (256-channel convs on 32 / 64-wide grids as slice-staged
    ping-pong instead of the row-block kernel) set as the case asks; restores the configured value."""

    def __init__(self, kw):
        self.on = kw.pop("slp256", None)

    def __enter__(self):
        if self.on is not None:
            import ctypes
            from distributedpytorch_amd.ops import _lib
            _lib.lib().dpa_igemm_set_slp256(ctypes.c_int(int(self.on)))

    def __exit__(self, *exc):
        if self.on is not None:
            import ctypes
            from distributedpytorch_amd.ops import _lib, kernels as K
            _lib.lib().dpa_igemm_set_slp256(ctypes.c_int(int(K.CFG.slp256)))


def _done(what, *bufs):
    torch.cuda.synchronize()
    for b in bufs:
        b.check(what)


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("case", FWD_CASES, ids=_ids(FWD_CASES))
def test_conv_fwd_exact(hip_lib, case, regime):
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, Cin, Cout, kw = case
    c = E.conv_fwd_case(regime, N, H, W, Cin, Cout)
    Cs = K.round_up(Cin, 8)
    packed, ng, kp = _pack_one(0, c.w.float(), Cs)
    X, Y = _in(E.pad_channels(c.x, Cs)), _out(N, H, W, Cout)
    kw = dict(kw)
    with _slp256(kw):
        K.igemm(X.view, packed, Y.view, Ngemm=ng, Kpad=kp, KH=3, KW=3, stride=1, pad=1, Cs=Cs, out_grid=(N, H, W),
                bias=c.b.float().cuda(), relu=True, **kw)
        _done(name, X, Y)
    E.assert_exact(Y.view, _expect(c.y), f"conv fwd {name} {regime}")


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_ids(DGRAD_CASES))
def test_conv_dgrad_masked_exact(hip_lib, case, regime):
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, Cin, Cout, kw = case
    c = E.conv_dgrad_case(regime, N, H, W, Cin, Cout)
    packed, ng, kp = _pack_one(1, c.w.float())
    G, M, Y = _in(c.g), _in(c.x), _out(N, H, W, Cin)
    kw = dict(kw)
    with _slp256(kw):
        K.igemm(G.view, packed, Y.view, Ngemm=ng, Kpad=kp, KH=3, KW=3, stride=1, pad=1, Cs=Cout, out_grid=(N, H, W),
                mask=M.view, **kw)
        _done(name, G, M, Y)
    E.assert_exact(Y.view, _expect(c.dxm), f"conv dgrad {name} {regime}")


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("case", SPLIT_CASES, ids=_ids(SPLIT_CASES))
def test_conv_dgrad_split_exact(hip_lib, case, regime):
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, Cin, Cout, kw = case
    c = E.conv_dgrad_case(regime, N, H, W, Cin, Cout)
    packed, ng, kp = _pack_one(1, c.w.float())
    s = Cin // 2
    G, LO, HI = _in(c.g), _out(N, H, W, s), _out(N, H, W, Cin - s)
    kw = dict(kw)
    with _slp256(kw):
        K.igemm(G.view, packed, LO.view, Ngemm=ng, Kpad=kp, KH=3, KW=3, stride=1, pad=1, Cs=Cout, out_grid=(N, H, W),
                y2=HI.view, split=s, **kw)
        _done(name, G, LO, HI)
    ref = _expect(c.dx)
    E.assert_exact(LO.view, ref[..., :s].contiguous(), f"split dgrad {name} {regime} low half")
    E.assert_exact(HI.view, ref[..., s:].contiguous(), f"split dgrad {name} {regime} high half")


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("case", DUAL_CASES, ids=_ids(DUAL_CASES))
def test_conv_dual_input_exact(hip_lib, case, regime):
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, Cin, Cout, kw = case
    c = E.conv_fwd_case(regime, N, H, W, Cin, Cout)
    packed, ng, kp = _pack_one(0, c.w.float(), Cin)
    X1, X2, Y = _in(c.x[:, :32]), _in(c.x[:, 32:]), _out(N, H, W, Cout)
    K.igemm(X1.view, packed, Y.view, Ngemm=ng, Kpad=kp, KH=3, KW=3, stride=1, pad=1, Cs=64, out_grid=(N, H, W),
            bias=c.b.float().cuda(), relu=True, x2=X2.view, **kw)
    _done(name, X1, X2, Y)
    E.assert_exact(Y.view, _expect(c.y), f"dual-input conv {name} {regime}")


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids(POOL_CASES))
def test_conv_fused_pool_exact(hip_lib, case, regime):
    """The conv output goes into a concat half (guard channels either side); the pooled tensor and the window
    codes are those of the STORED bf16 values: max-pool of the rounded reference, first maximum wins."""
    from distributedpytorch_amd.ops import kernels as K
    name, N, H, W, Cin, Cout, kw = case
    c = E.conv_fwd_case(regime, N, H, W, Cin, Cout)
    packed, ng, kp = _pack_one(0, c.w.float(), Cin)
    X, Y = _in(c.x), _out(N, H, W, Cout, lead=16, trail=8)
    P = _out(N, H // 2, W // 2, Cout)
    CD = _out(N, H // 2, W // 2, Cout, dtype=torch.uint8, fill=E.CODE_SENTINEL)
    K.igemm(X.view, packed, Y.view, Ngemm=ng, Kpad=kp, KH=3, KW=3, stride=1, pad=1, Cs=Cin, out_grid=(N, H, W),
            bias=c.b.float().cuda(), relu=True, pool=P.view, pcode=CD.view, **kw)
    _done(name, X, Y, P, CD)
    stored = E.bf16(c.y).double()
    E.assert_exact(Y.view, _expect(c.y), f"conv+pool {name} {regime} output")
    E.assert_exact(P.view, _expect(E.pool_ref(stored)[0]), f"conv+pool {name} {regime} pooled")
    E.assert_exact(CD.view, E.nhwc(E.pool_codes_ref(stored)), f"conv+pool {name} {regime} codes")


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("case", DECONV_IGEMM_CASES, ids=_ids(DECONV_IGEMM_CASES))
def test_deconv_igemm_exact(hip_lib, case, regime):
    """Transposed conv through ``igemm``: mode 1 forward scattered into the second half of a concat buffer, and
    the masked dgrad reading its gradient from a concat half."""
    from distributedpytorch_amd.ops import kernels as K
    name, N, h, w, Cin, Cout = case
    c = E.deconv_fwd_case(regime, N, h, w, Cin, Cout)
    packed, ng, kp = _pack_one(2, c.w.float())
    X, Y = _in(c.x), _out(N, 2 * h, 2 * w, Cout, lead=Cout, trail=8)
    K.igemm(X.view, packed, Y.view, Ngemm=ng, Kpad=kp, KH=1, KW=1, stride=1, pad=0, Cs=Cin, out_grid=(N, h, w),
            bias=c.b.float().cuda(), mode=1, Cout=Cout)
    _done(name, X, Y)
    E.assert_exact(Y.view, _expect(c.y), f"deconv fwd {name} {regime}")
    d = E.deconv_bwd_case(regime, N, h, w, Cin, Cout)
    packed, ng, kp = _pack_one(3, d.w.float())
    G, M, DX = _in(d.g, lead=Cout, trail=8), _in(d.x), _out(N, h, w, Cin)
    K.igemm(G.view, packed, DX.view, Ngemm=ng, Kpad=kp, KH=2, KW=2, stride=2, pad=0, Cs=Cout, out_grid=(N, h, w),
            mask=M.view)
    _done(name, G, M, DX)
    E.assert_exact(DX.view, _expect(d.dxm), f"deconv dgrad {name} {regime}")


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("case", DECONV_FUSED_CASES, ids=_ids(DECONV_FUSED_CASES))
def test_deconv_fused_exact(hip_lib, case, regime):
    """csrc/deconv.hip: the full-resolution forward into a concat half; the one-pass backward (masked dx, weight
    and bias gradients accumulated on integer start values) reading its gradient from a concat half."""
    from distributedpytorch_amd.ops import kernels as K
    name, N, h, w, Cin, Cout = case
    c = E.deconv_fwd_case(regime, N, h, w, Cin, Cout)
    wf, _, _ = _pack_one(2, c.w.float())
    X, Y = _in(c.x), _out(N, 2 * h, 2 * w, Cout, lead=Cout, trail=8)
    K.deconv_fwd_fused(X.view, wf, c.b.float().cuda(), Y.view)
    _done(name, X, Y)
    E.assert_exact(Y.view, _expect(c.y), f"deconv_fwd_fused {name} {regime}")
    d = E.deconv_bwd_case(regime, N, h, w, Cin, Cout)
    wd, _, _ = _pack_one(3, d.w.float())
    G, XI = _in(d.g, lead=Cout, trail=8), _in(d.x)
    GW = E.GuardedFlat(d.gw0.numel(), torch.float32, E.SENTINEL, d.gw0)
    GB = E.GuardedFlat(Cout, torch.float32, E.SENTINEL, d.gb0)
    dx = K.deconv_bwd_fused(G.view, XI.view, wd, GW.view, GB.view)
    _done(name, G, XI, GW, GB)
    E.assert_exact(dx, _expect(d.dxm), f"deconv_bwd_fused {name} {regime} dx")
    E.assert_exact(GW.view, d.gw.float().reshape(-1), f"deconv_bwd_fused {name} {regime} gw")
    E.assert_exact(GB.view, d.gb.float(), f"deconv_bwd_fused {name} {regime} gb")


def test_input_nhwc8_rounds_to_nearest_even(hip_lib):
    """fp32 image values placed exactly on bf16 ties and one fp32 ulp either side of them (and on exact bf16
    values, and just below the next one) must round to nearest even; the padding channels 3..7 are zero."""
    from distributedpytorch_amd.ops import kernels as K
    gen = E.rng(21)
    N, C, H, W = 2, 3, 7, 10
    base = (torch.randn(N, C, H, W, generator=gen) * 3).to(BF).view(torch.int16).to(torch.int32) & 0xFFFF
    low = torch.tensor([0x8000, 0x7FFF, 0x8001, 0x0000, 0xFFFF])[torch.arange(N * C * H * W) % 5].view(N, C, H, W)
    x = ((base << 16) | low).to(torch.int32).view(torch.float32)
    assert bool(torch.isfinite(x).all()) and int((low == 0x8000).sum()) >= 8
    y = K.input_nhwc8(x.cuda())
    torch.cuda.synchronize()
    assert tuple(y.shape) == (N, H, W, 8)
    E.assert_exact(y[..., :C].contiguous(), E.nhwc(x).to(BF), "input_nhwc8 rounding")
    E.assert_exact(y[..., C:].contiguous(), torch.zeros(N, H, W, 8 - C, dtype=BF), "input_nhwc8 padding channels")
    # an odd / even mantissa neighbour pair: ties go to the even one in both directions
    t = torch.tensor([257.0, 259.0, -257.0, -259.0, 1.00390625, 1.01171875]).view(1, 1, 1, 6)
    got = K.input_nhwc8(t.cuda())[0, 0, :, 0].float().cpu().tolist()
    assert got == [256.0, 260.0, -256.0, -260.0, 1.0, 1.015625], got


@pytest.mark.parametrize("N,H,W,C,nblk", [(2, 7, 9, 32, 0), (1, 33, 65, 64, 0), (2, 5, 3, 8, 0), (2, 33, 65, 32, 7)])
def test_chan_sum_bf16_exact(hip_lib, N, H, W, C, nblk):
    """Per-channel sums of a concat half of integers, accumulated on integer start values: exact."""
    from distributedpytorch_amd.ops import kernels as K
    gen = E.rng(N * H + C + nblk)
    g = E.integers(gen, (N, H, W, C), -64, 64)
    s0 = E.integers(gen, (C,), -8, 8)
    assert float(g.abs().sum((0, 1, 2)).max()) + 8 < E.ACC_LIMIT
    G = E.Guarded(N, H, W, C, BF, E.POISON, lead=C, trail=8, data=g)
    S = E.GuardedFlat(C, torch.float32, E.SENTINEL, s0)
    K._chan_sum_bf16(G.view, S.view, nblk)
    _done("chan_sum_bf16", G, S)
    E.assert_exact(S.view, (s0 + g.sum((0, 1, 2))).float(), "chan_sum_bf16")
