"""The engines' block Functions, bit for bit, on integer data (tests/exact_data.py).

``models/hip_unet.py`` strings the kernels together: ``_EncFn`` / ``_MidFn`` / ``_DecFn`` and the half-block Functions
choose between the pool-folded and the unfused backward, run the first level in image chunks through two
``SlabSink``s, write skips into concat halves or dense tensors, split a 2C-channel backward into two passes over
column slices of dW, crop skips, push weight gradients to a side stream and, under a pipeline, merge them over
microbatches.  Each of these is an index, an offset, a stream wait or an accumulate-versus-overwrite decision, so
each block runs here on data with ONE correct answer (``E.enc_block_case`` / ``double_conv_case`` / ``dec_block_case``
/ ``trunk_case``: float64 references rounded to bf16 exactly where the engine stores a tensor) and every output,
input gradient and parameter gradient -- on top of integer start values -- must be EQUAL to it; the parameters of
every other block must still hold their start values.

A pass only counts if the intended branch ran: ``Rec`` wraps the kernel entry points the Functions call and each
case asserts the launches (and their keyword arguments) of the branch it names, plus the public predicate that
routes its shape there, so a moved threshold fails loudly instead of silently moving the case to another path.

Parameter gradients are snapshot on the compute stream BEFORE the device is synchronised: a weight gradient still
in flight on a side stream that the block did not join shows as a mismatch.

The fp32 engine (``models/hip_unet_f32.py``) runs every ``small`` case (nothing rounds, so the references are its
too) through the same checks.  Out of scope: BatchNorm / bilinear variants and the head (an rsqrt, non-dyadic
weights, a sigmoid inside).
"""
import pytest
import torch

import exact_data as E

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ENC_CH = ((3, 32), (32, 64), (64, 128), (128, 256))       # (Cin, C) of encoder level l
DEC_C = (256, 128, 64, 32)                                 # output width of decoder block i
MID_CH = (256, 512, 512)

# encoder blocks: (id, level, regime, N, H, W)
ENC_CASES = [
    ("enc0-pool-fold", 0, "small", 2, 6, 64),
    ("enc0-chunks-sinks", 0, "small", 9, 4, 64),
    ("enc0-chunks-no-sink", 0, "small", 8, 4, 64),
    ("enc0-ragged60", 0, "small", 2, 6, 60),
    ("enc0-odd-height", 0, "small", 2, 7, 64),
    ("enc1-cat-half", 1, "small", 2, 8, 64),
    ("enc1-cat-half-round", 1, "round", 2, 8, 64),
    ("enc1-dense-skip", 1, "small", 2, 8, 64),
    ("enc2-gemm-side-stream", 2, "small", 2, 16, 32),
    ("enc3-deep", 3, "small", 2, 8, 32),
]
# the bottleneck: (id, regime, N, H, W)
MID_CASES = [("mid-deep", "small", 2, 4, 32), ("mid-deep-round", "round", 2, 4, 32), ("mid-generic-3x5", "small", 2, 3, 5)]
# decoder blocks: (id, block, regime, N, h, w, skip kind, (Hs, Ws) of a larger skip or None); output 2h x 2w
DEC_CASES = [
    ("dec0-own-half", 0, "small", 2, 4, 16, "own", None), ("dec0-foreign", 0, "small", 2, 4, 16, "foreign", None),
    ("dec1-own-half", 1, "small", 2, 8, 16, "own", None), ("dec1-foreign", 1, "small", 2, 8, 16, "foreign", None),
    ("dec2-halves", 2, "small", 2, 8, 32, "own", None),
    ("dec3-dual-own", 3, "small", 2, 4, 32, "own", None), ("dec3-dual-round", 3, "round", 2, 4, 32, "foreign", None),
    ("dec3-strided-skip", 3, "small", 2, 4, 32, "strided", None),
    ("dec3-crop", 3, "small", 2, 4, 32, "foreign", (9, 66)),
]
# half blocks (a pipeline cut between the two convs): (id, kind, index, N, H or h, W or w)
HALF_CASES = [("enc1-halves", "enc", 1, 2, 8, 64), ("mid-halves", "mid", 0, 2, 4, 32), ("dec3-halves", "dec", 3, 2, 4, 32),
              ("dec0-halves", "dec", 0, 2, 4, 16)]
# deferred weight gradients: (id, level, H, W, wgrad_multi eligible); microbatches of 2, 1, 2 images.  Every level of
# ``unet`` is eligible at any width >= 8, so the case that is not is the same level at a 4 x 6 grid (a different level
# in shape only); the predicate is asserted either way
DEFER_SIZES = (2, 1, 2)
DEFER_CASES = [("enc2-merged", 2, 16, 32, True), ("enc2-narrow-not-eligible", 2, 4, 6, False)]
TRUNK = (2, 32, 64)
RECORDED = ("conv_bwd_fused", "pool_bwd", "pool_bwd_code", "wgrad", "wgrad_multi", "igemm", "deconv_bwd_fused")


def _ids(cases):
    return [c[0] for c in cases]


def enc_case(case):
    _, l, regime, N, H, W = case
    return E.enc_block_case(regime, N, H, W, *ENC_CH[l])


def mid_case(case):
    _, regime, N, H, W = case
    return E.double_conv_case(regime, N, H, W, *MID_CH)


def dec_case(case):
    _, i, regime, N, h, w, _, big = case
    return E.dec_block_case(regime, N, h, w, DEC_C[i], Hs=big[0] if big else 0, Ws=big[1] if big else 0)


def half_case(case):
    _, kind, i, N, H, W = case
    if kind == "enc":
        return E.enc_block_case("small", N, H, W, *ENC_CH[i])
    return E.double_conv_case("small", N, H, W, *MID_CH) if kind == "mid" else E.dec_block_case("small", N, H, W, DEC_C[i])


def defer_case(case):
    _, l, H, W, _ = case
    return E.enc_block_case("small", sum(DEFER_SIZES), H, W, *ENC_CH[l], seed=1)


# ------------------------------------------------------------------------------------------- harness
class Rec:
    """Call-through recorders on the kernel entry points: (name, args, kwargs, stream the call was issued on)."""

    def __init__(self, monkeypatch, K):
        self.calls = []
        for name in RECORDED:
            monkeypatch.setattr(K, name, self._wrap(name, getattr(K, name)))

    def _wrap(self, name, fn):
        def call(*a, **k):
            self.calls.append((name, a, k, torch.cuda.current_stream().cuda_stream))
            return fn(*a, **k)
        return call

    def of(self, name, **where):
        return [c for c in self.calls if c[0] == name and all(c[2].get(k) == v for k, v in where.items())]

    def n(self, name, **where):
        return len(self.of(name, **where))


class Eng:
    """One ``unet`` and one engine over it; ``load`` writes a block's integer parameters, re-packs
    (``FlatParameterSpace.touch``) and pre-fills EVERY gradient with integer start values."""

    def __init__(self, f32: bool):
        from distributedpytorch_amd.models.hip_unet import HipBlocks
        from distributedpytorch_amd.models.hip_unet_f32 import HipF32Blocks
        from distributedpytorch_amd.models.unet import build_model
        torch.manual_seed(0)
        self.f32 = f32
        self.net = build_model("unet").cuda()
        self.B = (HipF32Blocks if f32 else HipBlocks)(self.net)
        self.space = self.net._flat_space
        self.dtype, self.cpad = (torch.float32, 4) if f32 else (BF, 8)
        self.params = dict(self.net.named_parameters())
        assert len(self.params) == 46
        gen = E.rng(99)
        self.start = {n: E.integers(gen, p.shape, -8, 8) for n, p in self.params.items()}

    def load(self, weights, starts):
        with torch.no_grad():
            for n, t in weights.items():
                self.params[n].copy_(t.float())
            for n, p in self.params.items():
                p.grad.copy_(starts.get(n, self.start[n]).float())
        self.space.touch()

    def snapshot(self):
        """Every parameter gradient as the compute stream sees it now (no device synchronisation before)."""
        return {n: p.grad.clone() for n, p in self.params.items()}

    def check_grads(self, expect, snap=None):
        snap = self.snapshot() if snap is None else snap
        torch.cuda.synchronize()
        for n, got in snap.items():
            own = n in expect
            E.assert_exact(got, (expect[n] if own else self.start[n]).float(),
                           f"{n} gradient" if own else f"{n} gradient (another block's: must keep its start value)")

    def x(self, t, grad=False, trail=0):
        """A Guarded activation from the NCHW float64 ``t`` (3 channels: zero-padded to the engine's input
        width): (guard, logical-NCHW view the block API takes)."""
        if t.shape[1] == 3:
            t = E.pad_channels(t, self.cpad)
        d = E.nhwc(t)
        G = E.Guarded(*d.shape, self.dtype, E.POISON, 0, trail, data=d)
        v = G.view.permute(0, 3, 1, 2)
        return G, (v.requires_grad_() if grad else v)

    def g(self, t):
        return E.nhwc(t).to(self.dtype).cuda().permute(0, 3, 1, 2)

    def eq(self, got, ref, what):
        E.assert_exact(got.permute(0, 2, 3, 1), E.nhwc(ref).to(self.dtype), what)


@pytest.fixture(scope="module")
def eng16(hip_lib):
    return Eng(False)


@pytest.fixture(scope="module")
def eng32(hip_lib):
    return Eng(True)


def _dc(pre, c, kind):
    """A DoubleConv's parameters (``w``), gradient starts (``0``) or reference gradients (``g``) by state-dict name."""
    f = {"w": ("w1", "b1", "w2", "b2"), "0": ("gw10", "gb10", "gw20", "gb20"), "g": ("gw1", "gb1", "gw2", "gb2")}[kind]
    return dict(zip((pre + ".0.weight", pre + ".0.bias", pre + ".2.weight", pre + ".2.bias"), (getattr(c, n) for n in f)))


def _up(pre, c, kind):
    f = {"w": ("wt", "bt"), "0": ("gwt0", "gbt0"), "g": ("gwt", "gbt")}[kind]
    return dict(zip((pre + ".weight", pre + ".bias"), (getattr(c, n) for n in f)))


def _on_side(B, calls):
    return bool(calls) and all(c[3] == B.side.cuda_stream for c in calls)


# ------------------------------------------------------------------------------------------- encoder
def _run_enc(eng, l, c, halves=False):
    pre = f"encoder.conv{l + 1}.conv_block"
    eng.load(_dc(pre, c, "w"), _dc(pre, c, "0"))
    B = eng.B
    Gx, x = eng.x(c.x, grad=l > 0)
    if halves:
        a = B.enc_a(l, x)
        skip, pooled = B.enc_b(l, a)
        eng.eq(a, c.a, "conv1 output")
    else:
        skip, pooled = B.enc(l, x)
    torch.autograd.backward([skip, pooled], [eng.g(c.dskip), eng.g(c.dpooled)])
    snap = eng.snapshot()
    torch.cuda.synchronize()
    Gx.check("encoder input")
    eng.eq(skip, c.y, "skip")
    eng.eq(pooled, c.pooled, "pooled")
    if l > 0:
        eng.eq(x.grad, c.dx, "input gradient")
    else:
        assert x.grad is None
    eng.check_grads(_dc(pre, c, "g"), snap)
    return skip


def _enc_evidence(name, rec, B, K, c, skip, reduces):
    N, _, H, W = c.x.shape
    C = c.y.shape[1]
    fused, bc, bp, wg = rec.of("conv_bwd_fused"), rec.n("pool_bwd_code"), rec.n("pool_bwd"), rec.of("wgrad")
    folded = [f for f in fused if f[2].get("pool") is not None]
    assert rec.n("wgrad_multi") == 0
    if name == "enc0-pool-fold":
        assert K.bwd_fused_eligible(32, 32, W, whole=True) and K.bwd_pool_foldable(32, 32) and N < K.ENC0_CHUNKS
        assert len(fused) == len(folded) == 1 and fused[0][2].get("sink") is None and fused[0][2].get("w1") is None
        assert bc == bp == 0 and len(wg) == 1 and wg[0][2]["Nc"] == 8 and wg[0][2].get("sink") is None and _on_side(B, wg)
    elif name in ("enc0-chunks-sinks", "enc0-chunks-no-sink"):
        sizes = [1, 1, 1, 1, 1, 1, 1, N - 7]
        assert K.ENC0_CHUNKS == 8 and N >= 8 and K.wgrad_multi_eligible(32, 8, W)
        assert len(fused) == len(folded) == len(wg) == 8 and bc == bp == 0
        assert [f[1][1].shape[0] for f in fused] == sizes and [w[1][0].shape[0] for w in wg] == sizes
        s2, s1 = {id(f[2].get("sink")) for f in fused}, {id(w[2].get("sink")) for w in wg}
        if name == "enc0-chunks-sinks":
            assert K.CHUNK_SINK and len(s2) == len(s1) == 1 and s1 != s2 and fused[0][2]["sink"] is not None \
                and wg[0][2]["sink"] is not None, "one SlabSink per conv"
            for s in (fused[0][2]["sink"], wg[0][2]["sink"]):
                assert s.used == s.rows and s.buf is None, "every sized slab row taken and reduced"
            assert reduces == [id(fused[0][2]["sink"]), id(wg[0][2]["sink"])], "one reduction per conv"
        else:
            assert s2 == s1 == {id(None)} and reduces == [], "eight accumulating launches per conv"
        assert _on_side(B, wg)
    elif name == "enc0-ragged60":
        assert K.bwd_fused_eligible(32, 32, W) and not K.bwd_fused_eligible(32, 32, W, whole=True)
        assert bc == 1 and bp == 0 and len(fused) == 1 and not folded and fused[0][2]["mask"] is True and len(wg) == 1
    elif name == "enc0-odd-height":
        assert H % 2 == 1 and K.bwd_fused_eligible(32, 32, W)
        assert bc == 0 and bp == 1 and len(fused) == 1 and not folded and len(wg) == 1
        assert tuple(c.pooled.shape[2:]) == (H // 2, W // 2)
        assert not bool(E.pool_route(c.dpooled, c.q, H, W)[:, :, H - 1].any()), "the last row gets no pool gradient"
    elif name.startswith("enc1"):
        fold = K.bwd_fused_eligible(64, 64, W, whole=True) and K.bwd_pool_foldable(64, 64)
        assert K.bwd_fused_eligible(32, 64, W) and K.bwd_fused_eligible(64, 64, W) and not B.dual_level(1, H, W)
        assert len(fused) == 2 and len(folded) == int(fold) and bc == int(not fold) and bp == 0 and not wg
        assert fused[0][2]["mask"] is True and fused[1][2]["mask"] is False, "conv2 masked by a, conv1's dx unmasked"
        dense = name == "enc1-dense-skip"
        assert skip.permute(0, 2, 3, 1).stride(2) == (C if dense else 2 * C), "dense skip / concat-buffer half"
    elif name in ("enc2-gemm-side-stream", "enc3-deep"):
        Cin = c.x.shape[1]
        assert not K.bwd_fused_eligible(C, C, W) and not K.bwd_fused_eligible(Cin, C, W)
        if name == "enc3-deep":
            assert K.wgrad_band_eligible(C, C, (N, H, W)) and K.wgrad_band_eligible(C, Cin, (N, H, W))
        assert not fused and bc == 1 and bp == 0 and len(wg) == 2 and _on_side(B, wg), "side-stream weight gradients"
        ig = rec.of("igemm")
        assert len(ig) == 4 and [i[2].get("mask") is not None for i in ig] == [False, False, True, False]
        assert ig[2][2]["persistent"] is False and ig[3][2]["persistent"] is False, "dgrads while the side stream is busy"
    else:
        raise AssertionError(f"no branch evidence written for {name}")


@pytest.mark.parametrize("case", ENC_CASES, ids=_ids(ENC_CASES))
def test_encoder_block_exact(eng16, monkeypatch, case):
    from distributedpytorch_amd.ops import kernels as K
    name, l = case[0], case[1]
    c = enc_case(case)
    B = eng16.B
    if name == "enc0-chunks-no-sink":
        monkeypatch.setattr(K, "CHUNK_SINK", False)
    if name == "enc1-dense-skip":
        monkeypatch.setattr(B, "dense_skips", {1})
    reduces = []
    orig = K.SlabSink.reduce
    monkeypatch.setattr(K.SlabSink, "reduce", lambda s: (reduces.append(id(s)), orig(s))[1])
    rec = Rec(monkeypatch, K)
    skip = _run_enc(eng16, l, c)
    _enc_evidence(name, rec, B, K, c, skip, reduces)


# ------------------------------------------------------------------------------------------- bottleneck
def _run_mid(eng, c, halves=False):
    pre = "mid.conv_block"
    eng.load(_dc(pre, c, "w"), _dc(pre, c, "0"))
    Gx, x = eng.x(c.x, grad=True)
    if halves:
        a = eng.B.mid_a(x)
        y = eng.B.mid_b(a)
        eng.eq(a, c.a, "conv1 output")
    else:
        y = eng.B.mid(x)
    y.backward(eng.g(c.g))
    snap = eng.snapshot()
    torch.cuda.synchronize()
    Gx.check("bottleneck input")
    eng.eq(y, c.y, "output")
    eng.eq(x.grad, c.dx, "input gradient")
    eng.check_grads(_dc(pre, c, "g"), snap)


@pytest.mark.parametrize("case", MID_CASES, ids=_ids(MID_CASES))
def test_mid_block_exact(eng16, monkeypatch, case):
    from distributedpytorch_amd.ops import kernels as K
    c = mid_case(case)
    N, _, H, W = c.x.shape
    rec = Rec(monkeypatch, K)
    _run_mid(eng16, c)
    ig, wg = rec.of("igemm"), rec.of("wgrad")
    assert rec.n("conv_bwd_fused") == rec.n("wgrad_multi") == 0 and len(ig) == 4 and len(wg) == 2 and _on_side(eng16.B, wg)
    assert [i[2]["persistent"] for i in ig[2:]] == [False, False], "no persistent grid while the side stream is busy"
    if case[0] == "mid-generic-3x5":
        grid = (N, H, W)
        assert not any(f(512, nc, grid) for f in (K.wgrad_band_eligible, K.wgrad_band128_eligible, K.wgrad_gemm_eligible)
                       for nc in (256, 512)) and not K.wgrad_multi_eligible(512, 512, W), "generic fallbacks end to end"
    else:
        assert K.wgrad_band_eligible(512, 512, (N, H, W)) and K.wgrad_band_eligible(512, 256, (N, H, W))


# ------------------------------------------------------------------------------------------- decoder
def _full_cat(half, C):
    """The [N, H, W, 2C] buffer of which the NHWC view ``half`` is the first C channels."""
    return torch.as_strided(half, tuple(half.shape[:3]) + (2 * C,), half.stride(), half.storage_offset())


def _run_dec(eng, i, c, kind, halves=False, rec=None):
    pre, upre = f"decoder.conv{i + 1}.conv_block", f"decoder.deconv{i + 1}"
    eng.load({**_dc(pre, c, "w"), **_up(upre, c, "w")}, {**_dc(pre, c, "0"), **_up(upre, c, "0")})
    B = eng.B
    C = DEC_C[i]
    Gx, x = eng.x(c.x, grad=True)
    Gs = None
    if kind == "own":
        # the skip as this engine's encoder hands it over (a concat-buffer half, or dense at the dual level), its
        # values replaced by the case's; the encoder's backward never runs (autograd.grad stops at the skip)
        l = 3 - i
        N, _, Hs, Ws = c.skip.shape
        skip, _ = B.enc(l, torch.zeros(N, Hs, Ws, eng.cpad if l == 0 else ENC_CH[l][0], dtype=eng.dtype,
                                       device="cuda").permute(0, 3, 1, 2))
        # (.data: the same storage under a version counter of its own -- autograd forbids in-place writes to an output
        # view of a multi-output Function, and nothing here differentiates through the encoder)
        skip.data.permute(0, 2, 3, 1).copy_(E.nhwc(c.skip).to(eng.dtype))
        if rec is not None:
            rec.calls.clear()      # the encoder forward that produced the skip is no evidence
    else:
        Gs, skip = eng.x(c.skip, grad=True, trail=16 if kind == "strided" else 0)
    if halves:
        a = B.dec_a(i, x, skip)
        y = B.dec_b(i, a)
        eng.eq(a, c.a, "conv1 output")
    else:
        y = B.dec(i, x, skip)
    dx, dskip = torch.autograd.grad(y, [x, skip], eng.g(c.g))
    snap = eng.snapshot()
    torch.cuda.synchronize()
    Gx.check("decoder input")
    if Gs is not None:
        Gs.check("skip")
    eng.eq(y, c.y, "output")
    eng.eq(dx, c.dx_unmasked if eng.f32 else c.dx, "input gradient")
    eng.eq(dskip, c.dskip, "skip gradient")
    eng.check_grads({**_dc(pre, c, "g"), **_up(upre, c, "g")}, snap)
    return skip


def _dec_evidence(name, rec, B, K, c, i, skip):
    C = DEC_C[i]
    N, _, h, w = c.x.shape
    H, W = 2 * h, 2 * w
    c1 = B.dec_convs[i][0]
    fused, wg, ig = rec.of("conv_bwd_fused"), rec.of("wgrad"), rec.of("igemm")
    if i in (0, 1):
        assert not B.halves_fusable(c1, C, W) and not B.fusable(c1, None, W) and not B.dual_level(3 - i, H, W)
        assert not K.wgrad_up_eligible(C, 2 * C, (N, h, w)), "small batch: the split-K transposed-conv weight gradient"
        assert not fused and rec.n("deconv_bwd_fused") == 0
        assert rec.n("igemm", split=C) == 1 and rec.of("igemm", split=C)[0][2]["y2"] is not None, "conv_dgrad_split"
        assert [k[2]["kind"] for k in wg] == [0, 0, 1] and _on_side(B, wg)
        assert rec.n("igemm", KH=2, stride=2) == 1, "transposed-conv dgrad"
        if name.endswith("own-half"):
            # zero-copy: the transposed conv wrote into the encoder's own buffer, next to the skip
            E.assert_exact(_full_cat(skip.permute(0, 2, 3, 1), C)[..., C:], E.bf16(E.nhwc(c.up)), "up half of the own buffer")
    elif i == 2:
        assert B.halves_fusable(c1, C, W) and not B.fusable(c1, None, W) and K.bwd_fused_eligible(64, 64, W)
        assert (128, 64) in K.DECONV_BWD_SHAPES and rec.n("deconv_bwd_fused") == 1 and not wg
        assert len(fused) == 3, "conv2's fused backward, then one pass per concat half"
        lo, hi = fused[1], fused[2]
        assert lo[1][5] is not None and hi[1][5] is None, "the bias gradient comes with the first half only"
        assert lo[1][1].shape[3] == hi[1][1].shape[3] == C and hi[1][1].data_ptr() - lo[1][1].data_ptr() == 2 * C
        assert lo[2]["mask"] is False and hi[2]["mask"] is False
    else:
        dual = name.startswith("dec3-dual")
        assert B.dual_level(0, H, W) and (64, 32) in K.DECONV_BWD_SHAPES and rec.n("deconv_bwd_fused") == 1 and not wg
        assert len(fused) == 2 and fused[1][2]["split"] == C and fused[1][2]["dx2"] is not None
        fwd_x2 = [g for g in ig if g[2].get("x2") is not None]
        if dual:
            assert len(fwd_x2) == 1 and fused[1][2]["x2"] is not None, "dual input: forward and fused backward read [skip | up]"
        else:
            assert not fwd_x2 and fused[1][2].get("x2") is None, "a strided / cropped skip takes the concat path"
            assert B.fusable(c1, None, W)


@pytest.mark.parametrize("case", DEC_CASES, ids=_ids(DEC_CASES))
def test_decoder_block_exact(eng16, monkeypatch, case):
    from distributedpytorch_amd.ops import kernels as K
    name, i, kind = case[0], case[1], case[6]
    c = dec_case(case)
    if case[7]:
        top, left = c.crop
        assert (top, left) == (0, 1) and not bool(c.dskip[:, :, 8:].any()) and not bool(c.dskip[:, :, :, 0].any())
    rec = Rec(monkeypatch, K)
    skip = _run_dec(eng16, i, c, kind, rec=rec)
    _dec_evidence(name, rec, eng16.B, K, c, i, skip)


# ------------------------------------------------------------------------------------------- half blocks
def _run_halves(eng, case):
    _, kind, i = case[:3]
    c = half_case(case)
    if kind == "enc":
        _run_enc(eng, i, c, halves=True)
    elif kind == "mid":
        _run_mid(eng, c, halves=True)
    else:
        _run_dec(eng, i, c, "foreign", halves=True)
    return c


@pytest.mark.parametrize("case", HALF_CASES, ids=_ids(HALF_CASES))
def test_half_blocks_exact(eng16, monkeypatch, case):
    """``enc_a`` + ``enc_b`` / ``mid_a`` + ``mid_b`` / ``dec_a`` + ``dec_b`` against the whole block's reference; the
    evidence is which backward each half took: the fused one (``bwd_conv``) or weight gradient + dgrad."""
    from distributedpytorch_amd.ops import kernels as K
    name, kind, i = case[:3]
    B = eng16.B
    rec = Rec(monkeypatch, K)
    c = _run_halves(eng16, case)
    fused, wg = rec.of("conv_bwd_fused"), rec.of("wgrad")
    assert rec.n("wgrad_multi") == 0
    if name == "enc1-halves":
        W = c.x.shape[3]
        fold = K.bwd_fused_eligible(64, 64, W, whole=True) and K.bwd_pool_foldable(64, 64)
        assert B.fusable(B.enc_convs[1][0], None, W) and B.fusable(B.enc_convs[1][1], B.enc_convs[1][0], W)
        assert len(fused) == 2 and not wg and [f[2].get("pool") is not None for f in fused] == [bool(fold), False]
        assert rec.n("pool_bwd_code") == int(not fold) and fused[1][2]["mask"] is False
    elif name == "mid-halves":
        assert not B.fusable(B.mid_convs[1], B.mid_convs[0], c.x.shape[3]) and not fused
        assert len(wg) == 2 and _on_side(B, wg) and rec.n("igemm") == 4
    elif name == "dec3-halves":
        W = 2 * c.x.shape[3]
        assert B.dual_level(0, 2 * c.x.shape[2], W) and B.fusable(B.dec_convs[3][1], B.dec_convs[3][0], W)
        assert len(fused) == 2 and not wg and rec.n("deconv_bwd_fused") == 1
        assert fused[0][2]["mask"] is True and fused[1][2]["split"] == 32 and fused[1][2]["x2"] is not None
    elif name == "dec0-halves":
        C, W = DEC_C[0], 2 * c.x.shape[3]
        assert not B.fusable(B.dec_convs[0][0], None, W) and not B.halves_fusable(B.dec_convs[0][0], C, W)
        assert not fused and [k[2]["kind"] for k in wg] == [0, 0, 1] and rec.n("igemm", split=C) == 1
        assert rec.n("deconv_bwd_fused") == 0
    else:
        raise AssertionError(f"no branch evidence written for {name}")


# ------------------------------------------------------------------------------------------- deferred wgrads
@pytest.mark.parametrize("cap", ["default-cap", "low-cap"])
@pytest.mark.parametrize("case", DEFER_CASES, ids=_ids(DEFER_CASES))
def test_deferred_weight_gradients_sum_over_microbatches(eng16, monkeypatch, case, cap):
    """Three microbatches (2, 1, 2 images) inside a defer window: start value + the exact sum over all five images,
    one ``wgrad_multi`` launch per eligible conv -- more, each over the microbatches it has, under a low memory cap --
    and the compute stream joins the merged launches' stream when the window closes."""
    from distributedpytorch_amd.ops import kernels as K
    name, l, H, W, eligible = case
    c = defer_case(case)
    B = eng16.B
    Cin, C = ENC_CH[l]
    assert K.wgrad_multi_eligible(C, C, W) == K.wgrad_multi_eligible(C, Cin, W) == eligible
    assert not K.bwd_fused_eligible(C, C, W), "the level's weight gradients go through conv_wgrad"
    pre = f"encoder.conv{l + 1}.conv_block"
    eng16.load(_dc(pre, c, "w"), _dc(pre, c, "0"))
    waits = []
    orig_wait = torch.cuda.Stream.wait_stream
    monkeypatch.setattr(torch.cuda.Stream, "wait_stream",
                        lambda s, o: (waits.append((s.cuda_stream, o.cuda_stream)), orig_wait(s, o))[1])
    rec = Rec(monkeypatch, K)
    monkeypatch.setattr(B, "defer_wgrad", 3)
    monkeypatch.setattr(B, "n_multi_launches", 0)
    if cap == "low-cap":
        # room for one microbatch's operands of one conv, not for two: partial merges
        monkeypatch.setattr(B, "defer_cap_bytes", 2 * H * W * 2 * C * 2 + 1)
    B.open_defer_window()
    try:
        n0 = 0
        outs = []
        for n in DEFER_SIZES:
            sl = slice(n0, n0 + n)
            n0 += n
            Gx, x = eng16.x(c.x[sl], grad=True)
            skip, pooled = B.enc(l, x)
            torch.autograd.backward([skip, pooled], [eng16.g(c.dskip[sl]), eng16.g(c.dpooled[sl])])
            outs.append((sl, skip, pooled, x))
        assert (B.n_multi_launches > 0) == eligible
        before = len(waits)
    finally:
        B.close_defer_window()
    snap = eng16.snapshot()
    torch.cuda.synchronize()
    for sl, skip, pooled, x in outs:
        eng16.eq(skip, c.y[sl], "skip")
        eng16.eq(pooled, c.pooled[sl], "pooled")
        eng16.eq(x.grad, c.dx[sl], "input gradient")
    eng16.check_grads(_dc(pre, c, "g"), snap)
    multi = rec.of("wgrad_multi")
    assert len(multi) == B.n_multi_launches
    if not eligible:
        assert not multi and rec.n("wgrad") == 6, "per-microbatch launches"
        return
    assert rec.n("wgrad") == 0
    cur = torch.cuda.current_stream().cuda_stream
    assert all(m[3] == B.side2.cuda_stream for m in multi), "merged launches on their own stream"
    assert (cur, B.side2.cuda_stream) in waits[before:], "close_defer_window joins the merged launches' stream"
    images = sorted(sum(t.shape[0] for t in m[1][0]) for m in multi)
    if cap == "default-cap":
        assert B.n_multi_launches == 2 and images == [5, 5], "one launch per conv over all three microbatches"
    else:
        assert 2 < B.n_multi_launches <= 6 and sum(images) == 10 and images[0] < 5, "partial merges under the cap"


# ------------------------------------------------------------------------------------------- the trunk
def _run_trunk(eng, c):
    from distributedpytorch_amd.models.blocks import n_blocks, run_segment
    eng.load(c.P, c.G0)
    skips = {}
    env = run_segment(eng.B, 0, n_blocks(4) - 1, 4, {"x": c.img.float().cuda()}, emit=skips.__setitem__)
    assert sorted(env) == ["x"] and sorted(skips) == ["skip0", "skip1", "skip2", "skip3"]
    y = env["x"]
    y.backward(eng.g(c.g))
    snap = eng.snapshot()
    torch.cuda.synchronize()
    return y, skips, snap


@pytest.mark.parametrize("regime", E.REGIMES)
def test_trunk_exact_and_repeatable(eng16, regime):
    """Encoder -> mid -> decoder as the trainer drives them (``run_segment``: ``prep``, the skip hand-over, concat
    buffers alive across levels): the last decoder output, the four skips and all 46 parameter gradients (the
    head's two keep their start values), then a second run from the same state, bit-equal."""
    c = E.trunk_case(regime, *TRUNK)
    y, skips, snap = _run_trunk(eng16, c)
    eng16.eq(y, c.y, "last decoder output")
    for l in range(4):
        eng16.eq(skips[f"skip{l}"], c.stored[f"skip{l}"], f"skip{l}")
    assert set(c.G) == set(eng16.params)
    eng16.check_grads(c.G, snap)
    y = y.detach().clone()
    y2, _, snap2 = _run_trunk(eng16, c)
    assert torch.equal(y2, y) and all(torch.equal(snap2[n], snap[n]) for n in snap), "second run differs"


# ------------------------------------------------------------------------------------------- fp32 engine
# The fp32 engine takes every level, so every ``small`` case above runs through it too.  Its Functions have no
# dispatch of their own except the concat (``_UpCat`` into the encoder's buffer, or ``_Deconv`` + cat for a cropped
# skip); the forms are chosen in ``ops.fp32`` (halo-staged against plain).  The evidence is therefore what the
# wrappers hand the library: ``F32Rec`` reads the ``halo`` field of every weight-gradient and conv launch.
class F32Rec:
    def __init__(self, monkeypatch, L):
        self.wgrad, self.igemm = [], []
        ow, oi = L.dpa_wgrad_f32, L.dpa_igemm_f32

        def wgrad(aref, st):
            a = aref._obj
            self.wgrad.append(dict(halo=a.halo, Nc=a.Nc, M=a.M, KH=a.KH))
            return ow(aref, st)

        def igemm(aref, st):
            a = aref._obj
            self.igemm.append(dict(halo=a.halo, KH=a.KH, Ngemm=a.Ngemm, Cs=a.Cs))
            return oi(aref, st)

        monkeypatch.setattr(L, "dpa_wgrad_f32", wgrad)
        monkeypatch.setattr(L, "dpa_igemm_f32", igemm)

    def conv_wgrads(self):
        return [w["halo"] for w in self.wgrad if w["KH"] == 3]


def _small(cases):
    return [c for c in cases if "small" in c[1:3]]           # the regime follows the id, or the id and the level


@pytest.mark.parametrize("halo", ["halo", "plain"])
@pytest.mark.parametrize("case", _small(ENC_CASES), ids=_ids(_small(ENC_CASES)))
def test_f32_encoder_block_exact(eng32, hip_lib, monkeypatch, case, halo):
    """Every small encoder case; the weight-gradient form each conv's launch was handed (conv2, then conv1; per
    chunkless call: the fp32 engine has no image chunks) against the one the case names, and the conv form flag."""
    from distributedpytorch_amd.ops import fp32 as F32
    name, l = case[0], case[1]
    c = enc_case(case)
    h64 = 2 if F32.WGRAD3_HALVES else 1          # 64 input channels: two 32-column halves per block
    expect = {"enc0-pool-fold": (1, None), "enc0-chunks-sinks": (1, None), "enc0-chunks-no-sink": (1, None),
              "enc0-ragged60": (0, None), "enc0-odd-height": (0, None), "enc1-cat-half": (h64, 1),
              "enc1-dense-skip": (h64, 1), "enc2-gemm-side-stream": (0, h64), "enc3-deep": (0, 0)}[name]
    if halo == "plain":
        monkeypatch.setattr(F32, "USE_WGRAD_HALO", False)
        monkeypatch.setattr(F32, "CONV_HALO", 0)
        expect = tuple(None if e is None else 0 for e in expect)
    else:
        assert F32.USE_WGRAD_HALO and F32.CONV_HALO, "the halo forms are the default"
    if name == "enc1-dense-skip":
        monkeypatch.setattr(eng32.B, "dense_skips", {1})
    rec = F32Rec(monkeypatch, hip_lib)
    skip = _run_enc(eng32, l, c)
    got = rec.conv_wgrads()
    assert len(got) == 2 and all(e is None or e == g for e, g in zip(expect, got)), (got, expect)
    assert expect[1] is not None or got[1] in (0, 3), "the first layer: its 4-channel form or the generic one"
    assert len(rec.igemm) == (4 if l > 0 else 3) and {i["halo"] for i in rec.igemm} == {F32.CONV_HALO}
    C = c.y.shape[1]
    assert skip.permute(0, 2, 3, 1).stride(2) == (C if name == "enc1-dense-skip" else 2 * C)


@pytest.mark.parametrize("case", _small(MID_CASES), ids=_ids(_small(MID_CASES)))
def test_f32_mid_block_exact(eng32, hip_lib, monkeypatch, case):
    rec = F32Rec(monkeypatch, hip_lib)
    _run_mid(eng32, mid_case(case))
    assert rec.conv_wgrads() == [0, 0] and len(rec.igemm) == 4, "256 / 512 input channels: the plain tiles"


@pytest.mark.parametrize("case", _small(DEC_CASES), ids=_ids(_small(DEC_CASES)))
def test_f32_decoder_block_exact(eng32, hip_lib, monkeypatch, case):
    """Every small decoder case: ``_UpCat`` takes the encoder's own buffer without a copy and copies a foreign or
    strided skip; a cropped skip goes through ``_Deconv`` + cat and never asks for a concat buffer."""
    name, i, kind = case[0], case[1], case[6]
    B = eng32.B
    cats = []
    orig = B.cat_for
    monkeypatch.setattr(B, "cat_for", lambda sk, width: (lambda out: (cats.append((sk.data_ptr(), out.data_ptr())), out)[1])(orig(sk, width)))
    rec = F32Rec(monkeypatch, hip_lib)
    _run_dec(eng32, i, dec_case(case), kind)
    assert [w["KH"] for w in rec.wgrad] == [3, 3, 2], "conv2, conv1, then the transposed conv"
    if case[7]:
        assert not cats, "cropped skip: no concat buffer"
    else:
        assert len(cats) == 1 and (cats[0][0] == cats[0][1]) == (kind == "own"), "zero copy only for the engine's own half"


@pytest.mark.parametrize("case", HALF_CASES, ids=_ids(HALF_CASES))
def test_f32_half_blocks_exact(eng32, hip_lib, monkeypatch, case):
    rec = F32Rec(monkeypatch, hip_lib)
    _run_halves(eng32, case)
    assert [w["KH"] for w in rec.wgrad] == ([3, 3, 2] if case[1] == "dec" else [3, 3])


def test_f32_trunk_exact_and_repeatable(eng32):
    test_trunk_exact_and_repeatable(eng32, "small")
