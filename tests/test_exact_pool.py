"""Max-pool forward / backward on tie-rich data: the first maximum in scan order (tl, tr, bl, br) wins.

``randn`` never puts two equal positive values into one 2x2 window, so the tie rule that csrc/unet_aux.hip
promises -- implemented separately in ``pool_code`` (``maxpool2``), the packed-u16 pool epilogue of the
row-streaming conv, the pool-folded fused backward (tests/test_exact_wgrad.py) and the fp32 kernels -- is only
exercised here: integer inputs in [0, 3], where most windows tie at a positive maximum and every window position
is the expected winner somewhere (asserted on the data by tests/exact_data.py).  The reference is torch's
``max_pool2d`` with ``return_indices``; the routed gradient is compared WITHOUT multiplying ties away.
"""
import pytest
import torch

import exact_data as E
from test_hip_kernels import _pack_one

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

POOL_CASES = [(2, 6, 8, 32), (2, 4, 20, 64), (3, 2, 2, 8)]          # (N, H, W, C), even sizes (window codes)
POOL_ODD_CASES = [(2, 7, 9, 32), (1, 5, 6, 64), (2, 6, 5, 8)]       # odd H and / or W: floor semantics
# conv + fused pool through the row-streaming kernel (Cin == Cout): (N, H, W, Cin, Cout)
CONV_POOL_CASES = [(2, 6, 128, 32, 32), (2, 5, 96, 64, 64), (2, 4, 64, 32, 32), (2, 6, 200, 64, 64)]
F32_POOL_CASES = [(2, 6, 8, 32), (2, 7, 9, 64), (3, 5, 4, 4)]


def _in(t_nchw, lead=0, trail=0, dtype=BF):
    d = E.nhwc(t_nchw)
    N, H, W, C = d.shape
    return E.Guarded(N, H, W, C, dtype, E.POISON, lead, trail, data=d)


def _out(N, H, W, C, lead=0, trail=0, dtype=BF, fill=E.SENTINEL):
    return E.Guarded(N, H, W, C, dtype, fill, lead, trail)


def _codes(t_nchw_u8):
    d = E.nhwc(t_nchw_u8)
    N, H, W, C = d.shape
    return E.Guarded(N, H, W, C, torch.uint8, E.CODE_SENTINEL, data=d)


def _done(what, *bufs):
    torch.cuda.synchronize()
    for b in bufs:
        b.check(what)


@pytest.mark.parametrize("N,H,W,C", POOL_CASES + POOL_ODD_CASES)
def test_maxpool2_values_and_codes_exact(hip_lib, N, H, W, C):
    """``maxpool2`` reading the skip half of a concat buffer: pooled values and window codes (argmax + ReLU bits)."""
    from distributedpytorch_amd.ops import kernels as K
    c = E.pool_case(N, H, W, C)
    X = _in(c.x, lead=8, trail=C)
    P = _out(N, H // 2, W // 2, C, lead=8, trail=8)
    CD = _out(N, H // 2, W // 2, C, dtype=torch.uint8, fill=E.CODE_SENTINEL)
    K.maxpool2(X.view, P.view, CD.view)
    _done("maxpool2", X, P, CD)
    E.assert_exact(P.view, E.bf16(E.nhwc(c.pooled)), "maxpool2 pooled")
    E.assert_exact(CD.view, E.nhwc(c.code), "maxpool2 codes")


@pytest.mark.parametrize("with_skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("N,H,W,C", POOL_CASES + POOL_ODD_CASES)
def test_pool_bwd_routes_ties_to_first_maximum(hip_lib, N, H, W, C, with_skip):
    """Value-based ``pool_bwd``: g = (dskip + route(dpool)) * (skip > 0); pixels outside the pooled area of an
    odd-sized grid get the skip gradient alone."""
    from distributedpytorch_amd.ops import kernels as K
    c = E.pool_case(N, H, W, C)
    S, DP, G = _in(c.x, lead=8, trail=C), _in(c.dpool), _out(N, H, W, C)
    DS = _in(c.dskip, lead=C, trail=8) if with_skip else None
    K.pool_bwd(S.view, DS.view if with_skip else None, DP.view, G.view)
    _done("pool_bwd", S, DP, G, *([DS] if with_skip else []))
    E.assert_exact(G.view, E.bf16(E.nhwc(c.g if with_skip else c.g_noskip)), "pool_bwd gradient")


@pytest.mark.parametrize("with_skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("N,H,W,C", POOL_CASES)
def test_pool_bwd_code_routes_ties_to_first_maximum(hip_lib, N, H, W, C, with_skip):
    """``pool_bwd_code`` from the reference's codes, and from the codes ``maxpool2`` writes: the same gradient."""
    from distributedpytorch_amd.ops import kernels as K
    c = E.pool_case(N, H, W, C)
    ref = E.bf16(E.nhwc(c.g if with_skip else c.g_noskip))
    X = _in(c.x)
    P = _out(N, H // 2, W // 2, C)
    CK = _out(N, H // 2, W // 2, C, dtype=torch.uint8, fill=E.CODE_SENTINEL)
    K.maxpool2(X.view, P.view, CK.view)
    for what, CD in (("reference codes", _codes(c.code)), ("maxpool2 codes", CK)):
        DP, G = _in(c.dpool), _out(N, H, W, C, lead=8, trail=8)
        DS = _in(c.dskip, lead=C, trail=8) if with_skip else None
        K.pool_bwd_code(CD.view, DS.view if with_skip else None, DP.view, G.view)
        _done(what, CD, DP, G, *([DS] if with_skip else []))
        E.assert_exact(G.view, ref, f"pool_bwd_code gradient from {what}")


@pytest.mark.parametrize("N,H,W,Cin,Cout", CONV_POOL_CASES)
def test_stream_conv_fused_pool_ties_exact(hip_lib, N, H, W, Cin, Cout):
    """The row-streaming conv's pool epilogue (packed-u16 maximum / compare) on a tie-rich conv output: pooled
    values and codes against torch's indices, and identical to what ``maxpool2`` writes from the stored output."""
    from distributedpytorch_amd.ops import kernels as K
    c = E.conv_pool_case(N, H, W, Cin, Cout)
    packed, ng, kp = _pack_one(0, c.w.float(), Cin)
    X, Y = _in(c.x), _out(N, H, W, Cout, lead=0, trail=Cout)
    P = _out(N, H // 2, W // 2, Cout)
    CD = _out(N, H // 2, W // 2, Cout, dtype=torch.uint8, fill=E.CODE_SENTINEL)
    K.igemm(X.view, packed, Y.view, Ngemm=ng, Kpad=kp, KH=3, KW=3, stride=1, pad=1, Cs=Cin, out_grid=(N, H, W),
            bias=c.b.float().cuda(), relu=True, pool=P.view, pcode=CD.view, path="stream")
    P2 = _out(N, H // 2, W // 2, Cout)
    CD2 = _out(N, H // 2, W // 2, Cout, dtype=torch.uint8, fill=E.CODE_SENTINEL)
    K.maxpool2(Y.view, P2.view, CD2.view)
    _done("conv + pool", X, Y, P, CD, P2, CD2)
    E.assert_exact(Y.view, E.bf16(E.nhwc(c.y)), "conv + pool: conv output")
    pooled, code = E.pool_ref(c.y)[0], E.pool_codes_ref(c.y)
    E.assert_exact(P.view, E.bf16(E.nhwc(pooled)), "conv + pool: fused pooled values")
    E.assert_exact(CD.view, E.nhwc(code), "conv + pool: fused codes")
    E.assert_exact(CD2.view, E.nhwc(code), "conv + pool: maxpool2 codes of the stored output")
    assert torch.equal(P.view, P2.view) and torch.equal(CD.view, CD2.view)


@pytest.mark.parametrize("N,H,W,C", F32_POOL_CASES)
def test_f32_pool_exact(hip_lib, N, H, W, C):
    """The fp32 engine: ``maxpool2`` (values + argmax code) of a concat half, ``maxpool2_bwd`` and ``enc_out_bwd``
    (skip gradient + routed pool gradient, ReLU-masked) with odd sizes (floor: the last row / column gets no
    pooled gradient)."""
    from distributedpytorch_amd.ops import fp32 as F32
    c = E.pool_case(N, H, W, C)
    X = _in(c.x, lead=4, trail=C, dtype=torch.float32)
    pooled, code = F32.maxpool2(X.view)
    _done("fp32 maxpool2", X)
    E.assert_exact(pooled, E.nhwc(c.pooled).float(), "fp32 maxpool2 pooled")
    E.assert_exact(code, E.nhwc(c.q).to(torch.uint8), "fp32 maxpool2 argmax code")
    gp = E.nhwc(c.dpool).float().cuda()
    E.assert_exact(F32.maxpool2_bwd(gp, code, H, W), E.nhwc(c.routed).float(), "fp32 maxpool2_bwd")
    GS = _in(c.dskip, lead=C, trail=4, dtype=torch.float32)
    ge = F32.enc_out_bwd(GS.view, gp, code, X.view)
    _done("fp32 enc_out_bwd", GS, X)
    E.assert_exact(ge, E.nhwc(c.g).float(), "fp32 enc_out_bwd")
    E.assert_exact(F32.enc_out_bwd(None, gp, code, X.view), E.nhwc(c.g_noskip).float(), "fp32 enc_out_bwd without skip")
