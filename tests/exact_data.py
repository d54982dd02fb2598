"""Integer test data on which the conv / weight-gradient / pool kernels have ONE correct answer, bit for bit.

Products of small bf16 integers are exact in fp32 and every partial sum stays an integer below 2^24, so the
fp32 accumulator holds the exact mathematical result in any summation order, under any split-K and in any
slab reduction.  A bf16 output must then equal ``round_to_nearest_even_bf16(exact)`` and an fp32 output the
exact value: a wrong index, a dropped term, a stray halo read, a wrong tie-break or a wrong rounding mode is
a ``torch.equal`` failure, not a shift inside a tolerance.

Two regimes:

``small``  activations / gradients in {-1, 0, 1}, weights in {-1, 0, 1} thinned to density min(1, 96 / K)
           (K = reduction length), biases in [-4, 4]: every reference value is a small integer that bf16 holds
           exactly -- nothing rounds, the test is purely about indexing.
``round``  outputs need more than 8 significant bits, exact ties included: forward convs use dense ternary
           weights, activations in {-3..3} and integer biases of magnitude in [256, 1024) (so a shallow K
           rounds too); dgrads, which have no bias, use gradients in [-64, 64].

References are float64 on the CPU (``F.conv2d`` / ``F.conv_transpose2d`` and their autograd, ``F.max_pool2d``
indices for the tie rule), rounded once at the end with ``.to(torch.bfloat16)`` where the kernel stores bf16.
The preconditions that make the comparison exact are asserted on the REFERENCE (never on a kernel output) by
the ``*_case`` builders below; a precondition that does not hold fails the test.  The builders are cached: a
case's data and reference are computed once per process and must not be modified by a test.

Whole blocks (tests/test_exact_blocks.py) use the same construction one level up: ``double_conv_case``,
``enc_block_case``, ``dec_block_case`` and ``trunk_case`` chain the float64 references and round to bf16 exactly at
the tensors the bf16 engine stores, so a block's outputs, input gradients and parameter gradients are unique too.

All tensors here are NCHW float64 on the CPU unless a name says otherwise; ``nhwc`` / ``nchw`` convert.
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

REGIMES = ("small", "round")
POISON = 4096.0          # finite guard value around inputs (0 * POISON == 0: an over-read lane times a zero weight is legal)
SENTINEL = 24576.0       # guard value around (and under) outputs; exactly representable in bf16
CODE_SENTINEL = 0xEE     # guard value of uint8 window-code outputs (no kernel writes bits 6-7)
ACC_LIMIT = float(2 ** 24)


# ------------------------------------------------------------------------------------------- generators
def rng(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


def integers(g: torch.Generator, shape, lo: int, hi: int) -> torch.Tensor:
    """Uniform integers in [lo, hi] as float64."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def ternary(g: torch.Generator, shape, density: float = 1.0) -> torch.Tensor:
    """Uniform {-1, 0, 1}, kept with probability ``density`` (zero otherwise)."""
    t = integers(g, shape, -1, 1)
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=g) < density).double()
    return t


def acts(g, shape, regime: str, relu: bool = False) -> torch.Tensor:
    a = integers(g, shape, -1, 1) if regime == "small" else integers(g, shape, -3, 3)
    return a.clamp_min(0) if relu else a


def grads(g, shape, regime: str) -> torch.Tensor:
    return integers(g, shape, -1, 1) if regime == "small" else integers(g, shape, -64, 64)


def weights(g, shape, K: int, regime: str) -> torch.Tensor:
    return ternary(g, shape, min(1.0, 96.0 / K) if regime == "small" else 1.0)


def bias(g, C: int, regime: str) -> torch.Tensor:
    if regime == "small":
        return integers(g, (C,), -4, 4)
    return integers(g, (C,), 256, 1023) * (integers(g, (C,), 0, 1) * 2 - 1)


# ------------------------------------------------------------------------------------------- layouts
def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2).contiguous()


def bf16(t: torch.Tensor) -> torch.Tensor:
    """The one rounding a bf16-storing kernel may apply to an exact value (round to nearest even)."""
    return t.to(torch.bfloat16)


def pad_channels(x: torch.Tensor, Cs: int) -> torch.Tensor:
    """NCHW x with its channels zero-padded to ``Cs`` (the first layer's 3 -> 8 / 4)."""
    if x.shape[1] == Cs:
        return x
    out = torch.zeros(x.shape[0], Cs, *x.shape[2:], dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


# ------------------------------------------------------------------------------------------- preconditions
def require_integers(*ts) -> None:
    for t in ts:
        assert torch.equal(t, t.round()), "test data must be integers"


class AccInexact(AssertionError):
    """A sum of |terms| reaches 2^24 (:func:`require_acc_exact`)."""


def require_acc_exact(bound: torch.Tensor, what: str) -> None:
    """``bound`` = the sum of |terms| (+ |bias|) per output: below 2^24 every partial sum, in any order, is an
    integer fp32 holds exactly."""
    m = float(bound.max())
    if not m < ACC_LIMIT:
        raise AccInexact(f"{what}: sum of |terms| reaches {m:.0f} >= 2^24 -- fp32 partial sums would not be exact")


def require_small(ref: torch.Tensor, what: str) -> None:
    """``small`` regime: the reference is its own bf16 rounding (nothing rounds anywhere)."""
    assert torch.equal(bf16(ref).double(), ref), f"{what}: small-regime reference is not exact in bf16"


def rounding_census(ref: torch.Tensor):
    """(exact ties, inexact outputs) of rounding ``ref`` (exact in fp32) to bf16: a tie has the fp32 low
    half-word 0x8000, an inexact output any non-zero low half-word."""
    r32 = ref.float()
    assert torch.equal(r32.double(), ref), "reference not exact in fp32"
    low = r32.contiguous().view(torch.int32) & 0xFFFF
    return int((low == 0x8000).sum()), int((low != 0).sum())


def require_round(ref: torch.Tensor, what: str) -> None:
    ties, inexact = rounding_census(ref)
    assert ties >= 8 and inexact >= 64, f"{what}: round-regime reference has {ties} ties / {inexact} inexact outputs (need 8 / 64)"


def require_regime(ref: torch.Tensor, regime: str, what: str) -> None:
    (require_small if regime == "small" else require_round)(ref, what)


# ------------------------------------------------------------------------------------------- pooling
def pool_ref(x: torch.Tensor):
    """2x2 / s2 max-pool (floor) of NCHW x: (pooled, q) with q the window position (2 i + j) of torch's argmax
    -- the first maximum in scan order tl, tr, bl, br."""
    W = x.shape[3]
    p, idx = F.max_pool2d(x, 2, 2, return_indices=True)
    h, w = idx // W, idx % W
    return p, ((h % 2) * 2 + (w % 2))


def pool_route(dpool: torch.Tensor, q: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Max-pool backward: dpool scattered to position q of each window over an (H, W) grid; pixels outside the
    pooled area (odd H / W) get zero."""
    N, C, Ho, Wo = dpool.shape
    out = torch.zeros(N, C, H, W, dtype=dpool.dtype)
    for k in range(4):
        out[:, :, k // 2:2 * Ho:2, k % 2:2 * Wo:2] = dpool * (q == k)
    return out


def pool_codes_ref(x: torch.Tensor) -> torch.Tensor:
    """The bf16 engine's window code (csrc/conv_args.h pool_code): argmax position | (value > 0) bits 2..5 for
    tl, tr, bl, br; uint8 NCHW [N, C, H/2, W/2]."""
    _, q = pool_ref(x)
    Ho, Wo = q.shape[2:]
    code = q.clone()
    for k in range(4):
        code = code | ((x[:, :, k // 2:2 * Ho:2, k % 2:2 * Wo:2] > 0).long() << (2 + k))
    return code.to(torch.uint8)


def require_pool_ties(x: torch.Tensor, what: str) -> None:
    """At least a quarter of the windows tie at a positive maximum; every window position wins somewhere."""
    p, q = pool_ref(x)
    Ho, Wo = p.shape[2:]
    hits = sum((x[:, :, k // 2:2 * Ho:2, k % 2:2 * Wo:2] == p).long() for k in range(4))
    tied = ((hits >= 2) & (p > 0)).double().mean().item()
    assert tied >= 0.25, f"{what}: only {tied:.1%} of the pool windows tie at a positive maximum"
    for k in range(4):
        assert bool((q == k).any()), f"{what}: window position {k} never wins"
    assert bool(((q > 0) & (hits >= 2)).any()), f"{what}: no tie whose first maximum is not the top-left pixel"


def pool_input(g, shape) -> torch.Tensor:
    """Post-ReLU-like integers in [0, 3]: most windows tie, a tenth are all zero."""
    return integers(g, shape, 0, 3)


# ------------------------------------------------------------------------------------------- references
def conv_fwd_ref(x, w, b, relu: bool = True):
    """conv3x3 pad 1 (+ bias, + ReLU)."""
    y = F.conv2d(x, w, b, padding=1)
    return F.relu(y) if relu else y


def conv_grads_ref(x, w, g):
    """(dx, dw, db) of y = conv3x3(x, w) + b, pad 1, for the output gradient g (autograd)."""
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = torch.zeros(w.shape[0], dtype=x.dtype, requires_grad=True)
    return torch.autograd.grad(F.conv2d(xr, wr, br, padding=1), (xr, wr, br), g)


def deconv_fwd_ref(x, w, b):
    """ConvTranspose2d(k2, s2) + bias; w [Cin, Cout, 2, 2]."""
    return F.conv_transpose2d(x, w, b, stride=2)


def deconv_grads_ref(x, w, g):
    """(dx, dw, db) of y = ConvTranspose2d(k2, s2)(x) + b for the output gradient g (autograd)."""
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = torch.zeros(w.shape[1], dtype=x.dtype, requires_grad=True)
    return torch.autograd.grad(F.conv_transpose2d(xr, wr, br, stride=2), (xr, wr, br), g)


# ------------------------------------------------------------------------------------------- conv cases
def _abs_conv_bound(x, w, b=None):
    y = F.conv2d(x.abs(), w.abs(), None, padding=1)
    return y if b is None else y + b.abs().view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def conv_fwd_case(regime: str, N: int, H: int, W: int, Cin: int, Cout: int, seed: int = 0) -> SimpleNamespace:
    """y = relu(conv3x3(x, w) + b), pad 1.  Fields x, w, b, y (float64)."""
    g = rng(1000 + seed)
    x = acts(g, (N, Cin, H, W), regime)
    w = weights(g, (Cout, Cin, 3, 3), 9 * Cin, regime)
    b = bias(g, Cout, regime)
    require_integers(x, w, b)
    require_acc_exact(_abs_conv_bound(x, w, b), "conv fwd")
    y = conv_fwd_ref(x, w, b)
    require_regime(y, regime, f"conv fwd {(N, H, W, Cin, Cout)}")
    return SimpleNamespace(x=x, w=w, b=b, y=y)


@functools.lru_cache(maxsize=None)
def conv_dgrad_case(regime: str, N: int, H: int, W: int, Cin: int, Cout: int, seed: int = 0) -> SimpleNamespace:
    """dx = conv3x3^T(g, w); dxm = dx * (x > 0) with x a ReLU output.  Fields x, w, g, dx, dxm."""
    gen = rng(2000 + seed)
    x = acts(gen, (N, Cin, H, W), regime, relu=True)
    w = weights(gen, (Cout, Cin, 3, 3), 9 * Cout, regime)
    g = grads(gen, (N, Cout, H, W), regime)
    require_integers(x, w, g)
    require_acc_exact(F.conv_transpose2d(g.abs(), w.abs(), padding=1), "conv dgrad")
    dx, _, _ = conv_grads_ref(x, w, g)
    dxm = dx * (x > 0)
    what = f"conv dgrad {(N, H, W, Cin, Cout)}"
    require_regime(dx, regime, what)
    require_regime(dxm, regime, what + " masked")
    return SimpleNamespace(x=x, w=w, g=g, dx=dx, dxm=dxm)


@functools.lru_cache(maxsize=None)
def conv_wgrad_case(N: int, H: int, W: int, Cin: int, Cout: int, seed: int = 0, amp_x: int = 1,
                    amp_g: int = 1) -> SimpleNamespace:
    """gw = dL/dw, gb = dL/db of conv3x3 pad 1 from (x, g), on top of integer start values gw0 / gb0
    (accumulate semantics).  Everything is exact in fp32.  Fields x, g, gw0, gb0, gw, gb."""
    gen = rng(3000 + seed)
    x = integers(gen, (N, Cin, H, W), -amp_x, amp_x)
    g = integers(gen, (N, Cout, H, W), -amp_g, amp_g)
    gw0 = integers(gen, (Cout, Cin, 3, 3), -8, 8)
    gb0 = integers(gen, (Cout,), -8, 8)
    assert N * H * W * amp_x * amp_g + 8 < ACC_LIMIT, "conv wgrad: sum of |terms| could reach 2^24"
    _, dw, db = conv_grads_ref(x, torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64), g)
    return SimpleNamespace(x=x, g=g, gw0=gw0, gb0=gb0, gw=gw0 + dw, gb=gb0 + db)


@functools.lru_cache(maxsize=None)
def conv_bwd_case(regime: str, N: int, H: int, W: int, Cin: int, Cout: int, seed: int = 0) -> SimpleNamespace:
    """Everything the fused conv backward returns: dx / dxm as :func:`conv_dgrad_case`, gw / gb on top of gw0 /
    gb0 as :func:`conv_wgrad_case`, from one (x, w, g)."""
    c = conv_dgrad_case(regime, N, H, W, Cin, Cout, seed)
    gen = rng(4000 + seed)
    gw0 = integers(gen, (Cout, Cin, 3, 3), -8, 8)
    gb0 = integers(gen, (Cout,), -8, 8)
    require_acc_exact(c.g.abs().sum((0, 2, 3)) * c.x.abs().max() + 8, "conv bwd wgrad")
    _, dw, db = conv_grads_ref(c.x, c.w, c.g)
    return SimpleNamespace(x=c.x, w=c.w, g=c.g, dx=c.dx, dxm=c.dxm, gw0=gw0, gb0=gb0, gw=gw0 + dw, gb=gb0 + db)


# ------------------------------------------------------------------------------------------- transposed conv
@functools.lru_cache(maxsize=None)
def deconv_fwd_case(regime: str, N: int, h: int, w: int, Cin: int, Cout: int, seed: int = 0) -> SimpleNamespace:
    """y = ConvTranspose2d(k2, s2)(x) + b (no ReLU).  Fields x, w [Cin, Cout, 2, 2], b, y."""
    gen = rng(5000 + seed)
    x = acts(gen, (N, Cin, h, w), regime)
    wt = weights(gen, (Cin, Cout, 2, 2), Cin, regime)
    b = bias(gen, Cout, regime)
    require_integers(x, wt, b)
    require_acc_exact(F.conv_transpose2d(x.abs(), wt.abs(), b.abs(), stride=2), "deconv fwd")
    y = deconv_fwd_ref(x, wt, b)
    require_regime(y, regime, f"deconv fwd {(N, h, w, Cin, Cout)}")
    return SimpleNamespace(x=x, w=wt, b=b, y=y)


@functools.lru_cache(maxsize=None)
def deconv_bwd_case(regime: str, N: int, h: int, w: int, Cin: int, Cout: int, seed: int = 0) -> SimpleNamespace:
    """Backward of the transposed conv from the output gradient g [N, Cout, 2h, 2w] with x a ReLU output:
    dx, dxm = dx * (x > 0), gw [Cin, Cout, 2, 2] / gb on top of integer gw0 / gb0."""
    gen = rng(6000 + seed)
    x = acts(gen, (N, Cin, h, w), regime, relu=True)
    wt = weights(gen, (Cin, Cout, 2, 2), 4 * Cout, regime)
    g = grads(gen, (N, Cout, 2 * h, 2 * w), regime)
    gw0 = integers(gen, (Cin, Cout, 2, 2), -8, 8)
    gb0 = integers(gen, (Cout,), -8, 8)
    require_integers(x, wt, g)
    require_acc_exact(F.conv2d(g.abs(), wt.abs(), stride=2), "deconv dgrad")
    require_acc_exact(g.abs().sum((0, 2, 3)) * max(1.0, float(x.abs().max())) + 8, "deconv wgrad")
    dx, dw, db = deconv_grads_ref(x, wt, g)
    dxm = dx * (x > 0)
    what = f"deconv dgrad {(N, h, w, Cin, Cout)}"
    require_regime(dx, regime, what)
    require_regime(dxm, regime, what + " masked")
    return SimpleNamespace(x=x, w=wt, g=g, dx=dx, dxm=dxm, gw0=gw0, gb0=gb0, gw=gw0 + dw, gb=gb0 + db)


# ------------------------------------------------------------------------------------------- pool cases
@functools.lru_cache(maxsize=None)
def pool_case(N: int, H: int, W: int, C: int, seed: int = 0) -> SimpleNamespace:
    """Tie-rich pooling: x in [0, 3]; pooled, q (winner), code (bf16 engine's byte), and the backward
    g = (dskip + route(dpool)) * (x > 0) WITHOUT multiplying ties away; route alone as ``routed``."""
    gen = rng(7000 + seed)
    x = pool_input(gen, (N, C, H, W))
    require_pool_ties(x, f"pool {(N, H, W, C)}")
    pooled, q = pool_ref(x)
    dpool = integers(gen, pooled.shape, -64, 64)
    dpool[dpool == 0] = 65                      # a misrouted gradient is never hidden by a zero
    dskip = integers(gen, x.shape, -32, 32)
    routed = pool_route(dpool, q, H, W)
    return SimpleNamespace(x=x, pooled=pooled, q=q, code=pool_codes_ref(x), dpool=dpool, dskip=dskip, routed=routed,
                           g=(dskip + routed) * (x > 0), g_noskip=routed * (x > 0))


@functools.lru_cache(maxsize=None)
def conv_bwd_pool_case(N: int, H: int, W: int, seed: int = 0) -> SimpleNamespace:
    """The pool-folded fused backward of an encoder conv2 (32 -> 32): the conv-output gradient is
    g = (dskip + route(dpool)) * (y > 0), formed from tie-rich window codes (:func:`pool_case`; ``skip``) or
    without a skip gradient (``noskip``); dx is masked by the conv input x.  First-level mode: dx is conv1's
    output gradient -- a bf16 tensor in the unfused engine -- so conv1's weight / bias gradients gw1 / gb1 come
    from the bf16-ROUNDED dx and the 3 real channels of the 8-channel input x1."""
    C = 32
    pc = pool_case(N, H, W, C, seed)
    gen = rng(8000 + seed)
    x = acts(gen, (N, C, H, W), "small", relu=True)
    w = weights(gen, (C, C, 3, 3), 9 * C, "small")
    x1 = pad_channels(integers(gen, (N, 3, H, W), 0, 3), 8)
    gw0, gb0 = integers(gen, (C, C, 3, 3), -8, 8), integers(gen, (C,), -8, 8)
    gw10, gb10 = integers(gen, (C, 3, 3, 3), -8, 8), integers(gen, (C,), -8, 8)
    out = SimpleNamespace(pool=pc, x=x, w=w, x1=x1, gw0=gw0, gb0=gb0, gw10=gw10, gb10=gb10)
    for name, g in (("skip", pc.g), ("noskip", pc.g_noskip)):
        require_acc_exact(F.conv_transpose2d(g.abs(), w.abs(), padding=1), "pool-folded dgrad")
        require_acc_exact(g.abs().sum((0, 2, 3)) + 8, "pool-folded wgrad")
        dx, dw, db = conv_grads_ref(x, w, g)
        dxm = dx * (x > 0)
        g1 = bf16(dxm).double()
        require_acc_exact(g1.abs().sum((0, 2, 3)) * 3 + 8, "first-level wgrad")
        _, dw1, db1 = conv_grads_ref(x1[:, :3], torch.zeros(C, 3, 3, 3, dtype=torch.float64), g1)
        setattr(out, name, SimpleNamespace(g=g, dxm=dxm, gw=gw0 + dw, gb=gb0 + db, gw1=gw10 + dw1, gb1=gb10 + db1))
    return out


@functools.lru_cache(maxsize=None)
def conv_pool_case(N: int, H: int, W: int, Cin: int, Cout: int, seed: int = 0) -> SimpleNamespace:
    """A conv whose ReLU output is tie-rich (about two ternary terms per output, bias in [0, 2]): the input of
    the row-streaming kernel's fused max-pool + window codes.  Fields x, w, b, y."""
    gen = rng(9000 + seed)
    x = acts(gen, (N, Cin, H, W), "small")
    w = ternary(gen, (Cout, Cin, 3, 3), 3.0 / (9 * Cin))
    b = integers(gen, (Cout,), 0, 2)
    y = conv_fwd_ref(x, w, b)
    require_small(y, "conv + pool")
    require_pool_ties(y, f"conv + pool {(N, H, W, Cin, Cout)}")
    return SimpleNamespace(x=x, w=w, b=b, y=y)


# ------------------------------------------------------------------------------------------- fp32 engine cases
# fp32 stores are exact, so there is nothing to round: the ``small`` construction (thinned ternary weights) at
# larger amplitudes -- activations in [-32, 32], gradients in [-4, 4], biases up to 2^10.
@functools.lru_cache(maxsize=None)
def f32_conv_case(N: int, H: int, W: int, Cin: int, Cout: int, seed: int = 0) -> SimpleNamespace:
    """conv3x3 pad 1 forward (bias + ReLU) and backward, every value an integer fp32 holds exactly.  Fields x (a
    ReLU-free input), w, b, y = relu(conv + b), g, dx, dxm = dx * (xm > 0) for a separate mask source xm, and
    gw / gb on top of gw0 / gb0."""
    gen = rng(10000 + seed)
    x = integers(gen, (N, Cin, H, W), -32, 32)
    xm = integers(gen, (N, Cin, H, W), -1, 1)
    w = ternary(gen, (Cout, Cin, 3, 3), min(1.0, 96.0 / (9 * max(Cin, Cout))))
    b = integers(gen, (Cout,), -1024, 1024)
    g = integers(gen, (N, Cout, H, W), -4, 4)
    gw0, gb0 = integers(gen, (Cout, Cin, 3, 3), -8, 8), integers(gen, (Cout,), -8, 8)
    require_acc_exact(_abs_conv_bound(x, w, b), "fp32 conv fwd")
    require_acc_exact(F.conv_transpose2d(g.abs(), w.abs(), padding=1), "fp32 conv dgrad")
    require_acc_exact(g.abs().sum((0, 2, 3)) * 32 + 8, "fp32 conv wgrad")
    y = conv_fwd_ref(x, w, b)
    dx, dw, db = conv_grads_ref(x, w, g)
    return SimpleNamespace(x=x, xm=xm, w=w, b=b, y=y, g=g, dx=dx, dxm=dx * (xm > 0), gw0=gw0, gb0=gb0, gw=gw0 + dw,
                           gb=gb0 + db)


@functools.lru_cache(maxsize=None)
def f32_deconv_case(N: int, h: int, w: int, Cin: int, Cout: int, seed: int = 0) -> SimpleNamespace:
    """ConvTranspose2d(k2, s2) forward (+ bias) and backward on exact fp32 integers.  Fields x, w [Cin, Cout, 2, 2],
    b, y, g, dx, gw / gb on top of gw0 / gb0."""
    gen = rng(11000 + seed)
    x = integers(gen, (N, Cin, h, w), -32, 32)
    wt = ternary(gen, (Cin, Cout, 2, 2), min(1.0, 96.0 / max(Cin, 4 * Cout)))
    b = integers(gen, (Cout,), -1024, 1024)
    g = integers(gen, (N, Cout, 2 * h, 2 * w), -4, 4)
    gw0, gb0 = integers(gen, (Cin, Cout, 2, 2), -8, 8), integers(gen, (Cout,), -8, 8)
    require_acc_exact(F.conv_transpose2d(x.abs(), wt.abs(), b.abs(), stride=2), "fp32 deconv fwd")
    require_acc_exact(F.conv2d(g.abs(), wt.abs(), stride=2), "fp32 deconv dgrad")
    require_acc_exact(g.abs().sum((0, 2, 3)) * 32 + 8, "fp32 deconv wgrad")
    y = deconv_fwd_ref(x, wt, b)
    dx, dw, db = deconv_grads_ref(x, wt, g)
    return SimpleNamespace(x=x, w=wt, b=b, y=y, g=g, dx=dx, gw0=gw0, gb0=gb0, gw=gw0 + dw, gb=gb0 + db)


# ------------------------------------------------------------------------------------------- block references
# Whole blocks of the engines (models/hip_unet.py, models/hip_unet_f32.py) in float64, rounded to bf16 exactly
# where the bf16 engine STORES a tensor: the transposed conv's output, each conv's ReLU output, the max-pool
# output (no rounding: a maximum of stored values), the gradient formed by the pool backward, the gradient between
# the two convs of a block, and every gradient a block returns.  Weight and bias gradients are fp32 sums of
# products of stored (bf16) tensors and are never rounded.  ``rnd=False`` switches every rounding off (the
# reference is then the plain mathematical block: tests/test_exact_data_cpu.py compares it with fp32 autograd);
# ``what`` switches the precondition checks on (integers, every sum of |terms| below 2^24).
def _rt(t: torch.Tensor, rnd: bool) -> torch.Tensor:
    return bf16(t).double() if rnd else t


def _fwd(x, w, b, rnd, what):
    if what:
        require_integers(x, w, b)
        require_acc_exact(_abs_conv_bound(x, w, b), what + " forward")
    return _rt(conv_fwd_ref(x, w, b), rnd)


def _bwd(x, w, g, what):
    """(dx, dw, db) of a conv3x3 from the conv-output gradient g, unrounded."""
    if what:
        require_integers(x, w, g)
        require_acc_exact(F.conv_transpose2d(g.abs(), w.abs(), padding=1), what + " dgrad")
        require_acc_exact(g.abs().sum((0, 2, 3)) * max(1.0, float(x.abs().max())) + 8, what + " wgrad")
    return conv_grads_ref(x, w, g)


def double_conv_fwd_ref(x, w1, b1, w2, b2, rnd: bool = True, what: str = ""):
    """(a, y) = (relu(conv1(x)), relu(conv2(a))), each stored in bf16."""
    a = _fwd(x, w1, b1, rnd, what and what + " conv1")
    return a, _fwd(a, w2, b2, rnd, what and what + " conv2")


def double_conv_bwd_ref(x, a, w1, w2, gy, rnd: bool = True, what: str = ""):
    """Backward of a DoubleConv from ``gy``, the gradient of conv2's OUTPUT (the ReLU mask of y already applied,
    as every bf16 block Function receives it): g1 = bf16(dgrad2(gy) * (a > 0)) is the stored gradient between the
    convs, dx = bf16(dgrad1(g1)) is NOT masked (the consumer -- pool backward, concat split -- masks it).
    Returns a namespace g1, dx, dw1, db1, dw2, db2."""
    da, dw2, db2 = _bwd(a, w2, gy, what and what + " conv2")
    g1 = _rt(da * (a > 0), rnd)
    dx, dw1, db1 = _bwd(x, w1, g1, what and what + " conv1")
    return SimpleNamespace(g1=g1, dx=_rt(dx, rnd), dw1=dw1, db1=db1, dw2=dw2, db2=db2)


def enc_block_ref(x, w1, b1, w2, b2, dskip, dpooled, rnd: bool = True, what: str = ""):
    """Encoder block (``_EncFn`` / ``_EncBFn``): skip = y, pooled = maxpool2(y) (floor; first maximum wins).
    Backward from (dskip, dpooled), both UNMASKED: the pool backward forms and stores
    g2 = bf16((dskip + route(dpooled)) * (y > 0)) -- the only place the skip's ReLU mask is applied -- then the
    DoubleConv backward; dx is unmasked (level 0 returns none).  Fields a, y, pooled, q, code (even H, W), g2 +
    those of :func:`double_conv_bwd_ref`."""
    a, y = double_conv_fwd_ref(x, w1, b1, w2, b2, rnd, what)
    H, W = y.shape[2:]
    pooled, q = pool_ref(y)
    g2 = _rt((dskip + pool_route(dpooled, q, H, W)) * (y > 0), rnd)
    r = double_conv_bwd_ref(x, a, w1, w2, g2, rnd, what)
    r.a, r.y, r.pooled, r.q, r.g2 = a, y, pooled, q, g2
    r.code = pool_codes_ref(y) if H % 2 == 0 and W % 2 == 0 else None
    return r


def crop_offsets(Hs: int, Ws: int, h2: int, w2: int):
    """(top, left) of the skip's centre crop, as ``_DecFn.forward`` computes them (Python's round: half to even)."""
    return int(round((Hs - h2) / 2.0)), int(round((Ws - w2) / 2.0))


def dec_block_ref(x, skip, wt, bt, w1, b1, w2, b2, g, rnd: bool = True, what: str = ""):
    """Decoder block (``_DecFn`` / ``_DecAFn`` + second half): up = bf16(deconv(x) + bt) (no ReLU), conv1 over
    [crop(skip) | up], conv2.  ``g`` is the gradient of y; the reference multiplies it by (y > 0) itself, so a
    test may hand the engine ``g * (y > 0)`` (the bf16 engine expects the mask applied) or ``g``.  The concat
    gradient bf16(dgrad1(g1)) is stored unmasked as its two halves: dskip (UNMASKED, zero outside the crop window
    of a larger skip) and gup; the transposed-conv dx = bf16(deconv^T(gup) * (x > 0)) IS masked by the block
    input (a ReLU output); ``dx_unmasked`` is what an engine that leaves the mask to the consumer returns."""
    if what:
        require_integers(x, wt, bt)
        require_acc_exact(F.conv_transpose2d(x.abs(), wt.abs(), bt.abs(), stride=2), what + " deconv forward")
    up = _rt(deconv_fwd_ref(x, wt, bt), rnd)
    C = up.shape[1]
    h2, w2_ = up.shape[2:]
    Hs, Ws = skip.shape[2:]
    top, left = crop_offsets(Hs, Ws, h2, w2_)
    cat = torch.cat([skip[:, :, top:top + h2, left:left + w2_], up], 1)
    a, y = double_conv_fwd_ref(cat, w1, b1, w2, b2, rnd, what)
    gy = g * (y > 0)
    r = double_conv_bwd_ref(cat, a, w1, w2, gy, rnd, what)
    gup = r.dx[:, C:]
    if what:
        require_acc_exact(F.conv2d(gup.abs(), wt.abs(), stride=2), what + " deconv dgrad")
        require_acc_exact(gup.abs().sum((0, 2, 3)) * max(1.0, float(x.abs().max())) + 8, what + " deconv wgrad")
    dxu, dwt, dbt = deconv_grads_ref(x, wt, gup)
    dskip = torch.zeros_like(skip)
    dskip[:, :, top:top + h2, left:left + w2_] = r.dx[:, :C]
    r.up, r.a, r.y, r.gy, r.gup, r.dskip = up, a, y, gy, gup, dskip
    r.dx, r.dx_unmasked, r.dwt, r.dbt = _rt(dxu * (x > 0), rnd), _rt(dxu, rnd), dwt, dbt
    return r


def _live(t: torch.Tensor, what: str) -> None:
    p = float((t > 0).double().mean())
    assert 0.25 <= p <= 0.75, f"{what}: {p:.1%} of a ReLU output is positive (need 25 % .. 75 %)"


def _dense_grad(t: torch.Tensor, what: str) -> None:
    p = float((t != 0).double().mean())
    assert p >= 0.05, f"{what}: only {p:.1%} of a reference parameter gradient is non-zero"


def _starts(gen, **shapes):
    """Integer start values in [-8, 8] for the accumulate semantics of every parameter gradient."""
    return {k: integers(gen, tuple(s), -8, 8) for k, s in shapes.items()}


GRAD_AMPS = (64, 56, 48, 40, 32, 28, 24, 20, 16, 14, 12, 10, 8, 6, 4, 3, 2, 1)


def _largest_amp(build):
    """``build(G)`` for the largest gradient amplitude G of GRAD_AMPS at which every sum of |terms| of the
    reference's backward (asserted by ``build`` itself, on the actual data) stays below 2^24: the ``round`` regime
    wants gradients as large as exactness allows, so that the stored gradients need more than 8 bits too.  Each
    amplitude draws its gradient from a generator of its own, so the result does not depend on the ones tried."""
    for G in GRAD_AMPS:
        try:
            return build(G)
        except AccInexact:
            if G == 1:
                raise


def _dc_params(gen, regime, Cin, Cmid, Cout):
    """DoubleConv parameters.  ``small``: conv1 thinned to ~24 ternary taps per output, conv2 to ~12, biases in
    [-2, 2].  ``round``: dense ternary weights and conv1 biases of magnitude [256, 1024) (:func:`bias`), so a,
    y and every gradient behind them need more than 8 significant bits."""
    if regime == "small":
        w1 = ternary(gen, (Cmid, Cin, 3, 3), min(1.0, 24.0 / (9 * Cin)))
        w2 = ternary(gen, (Cout, Cmid, 3, 3), min(1.0, 12.0 / (9 * Cmid)))
        return w1, integers(gen, (Cmid,), -2, 2), w2, integers(gen, (Cout,), -2, 2)
    return (ternary(gen, (Cmid, Cin, 3, 3)), bias(gen, Cmid, "round"), ternary(gen, (Cout, Cmid, 3, 3)),
            integers(gen, (Cout,), -2, 2))


def _intermediates_round(raw, what):
    """``round``: the stored intermediates a and g1 need more than 8 bits in at least 64 places each, so an engine
    that kept one of them in fp32, or rounded it twice, differs from the reference."""
    for n in ("a", "g1"):
        k = rounding_census(getattr(raw, n))[1]
        assert k >= 64, f"{what}: only {k} values of {n} round"


def _check_stored(regime, what, small=(), rounded=()):
    """``small``: nothing rounds in any stored tensor.  ``round``: the listed outputs meet require_round."""
    if regime == "small":
        for name, t in small:
            require_small(t, f"{what} {name}")
    else:
        for name, t in rounded:
            require_round(t, f"{what} {name}")


@functools.lru_cache(maxsize=None)
def double_conv_case(regime: str, N: int, H: int, W: int, Cin: int, Cmid: int, Cout: int, seed: int = 0):
    """A DoubleConv (``_MidFn``, the two ``_ConvHalfFn`` halves): x in {0, 1}; fields x, w1, b1, w2, b2, a, y,
    the output gradient ``g`` ALREADY multiplied by (y > 0) (the convention of ``_MidFn.backward``: its consumer
    applied the mask), g1, dx (unmasked), and gw1 / gb1 / gw2 / gb2 on top of the integer starts gw10 / gb10 /
    gw20 / gb20.  ``raw`` holds the unrounded values of the stored tensors a, y, g1, dx (their rounding census)."""
    gen = rng(12000 + seed)
    what = f"double conv {regime} {(N, H, W, Cin, Cmid, Cout)}"
    x = integers(gen, (N, Cin, H, W), 0, 1)
    w1, b1, w2, b2 = _dc_params(gen, regime, Cin, Cmid, Cout)
    a, y = double_conv_fwd_ref(x, w1, b1, w2, b2, True, what)
    s = _starts(gen, gw10=w1.shape, gb10=b1.shape, gw20=w2.shape, gb20=b2.shape)

    def backward(G):
        g = integers(rng(12500 + 100 * seed + G), y.shape, -G, G) * (y > 0)
        return g, double_conv_bwd_ref(x, a, w1, w2, g, True, what)

    g, r = backward(1) if regime == "small" else _largest_amp(backward)
    raw = SimpleNamespace(a=conv_fwd_ref(x, w1, b1), y=conv_fwd_ref(a, w2, b2),
                          g1=conv_grads_ref(a, w2, g)[0] * (a > 0), dx=conv_grads_ref(x, w1, r.g1)[0])
    _live(a, what + " a"), _live(y, what + " y")
    for n in ("dw1", "dw2", "db1", "db2"):
        _dense_grad(getattr(r, n), f"{what} {n}")
    assert bool((r.dx != 0).any()), what + ": dx is all zero"
    _check_stored(regime, what, small=[(n, getattr(raw, n)) for n in ("a", "y", "g1", "dx")],
                  rounded=[("y", raw.y), ("dx", raw.dx)])
    if regime == "round":
        _intermediates_round(raw, what)
    return SimpleNamespace(x=x, w1=w1, b1=b1, w2=w2, b2=b2, a=a, y=y, g=g, g1=r.g1, dx=r.dx, raw=raw, **s,
                           gw1=s["gw10"] + r.dw1, gb1=s["gb10"] + r.db1, gw2=s["gw20"] + r.dw2, gb2=s["gb20"] + r.db2)


@functools.lru_cache(maxsize=None)
def enc_block_case(regime: str, N: int, H: int, W: int, Cin: int, C: int, seed: int = 0):
    """An encoder block (:func:`enc_block_ref` for the masking convention): x in {0, 1} (the 3-channel network
    input for Cin = 3, which gets no gradient: ``dx`` is then None); fields as :func:`double_conv_case` plus
    pooled, q, code (None unless H and W are even), dskip, dpooled (no zeros: a misrouted pool gradient always
    shows) and g2.  |dskip| + |dpooled| <= 2 G <= 128 (G <= 64, :func:`_largest_amp`) is exact in bf16, so the order of the add cannot matter."""
    gen = rng(13000 + seed)
    what = f"enc block {regime} {(N, H, W, Cin, C)}"
    x = integers(gen, (N, Cin, H, W), 0, 1)
    w1, b1, w2, b2 = _dc_params(gen, regime, Cin, C, C)
    a, y = double_conv_fwd_ref(x, w1, b1, w2, b2)
    s = _starts(gen, gw10=w1.shape, gb10=b1.shape, gw20=w2.shape, gb20=b2.shape)

    def backward(G):
        gg = rng(13500 + 100 * seed + G)
        dskip = integers(gg, y.shape, -G, G)
        dpooled = integers(gg, (N, C, H // 2, W // 2), 1, G) * (integers(gg, (N, C, H // 2, W // 2), 0, 1) * 2 - 1)
        assert 2 * G <= 128
        return dskip, dpooled, enc_block_ref(x, w1, b1, w2, b2, dskip, dpooled, True, what)

    dskip, dpooled, r = backward(1) if regime == "small" else _largest_amp(backward)
    raw_dx = conv_grads_ref(x, w1, r.g1)[0]
    raw = SimpleNamespace(a=conv_fwd_ref(x, w1, b1), y=conv_fwd_ref(a, w2, b2),
                          g1=conv_grads_ref(a, w2, r.g2)[0] * (a > 0), dx=raw_dx)
    _live(a, what + " a"), _live(y, what + " y")
    for n in ("dw1", "dw2", "db1", "db2"):
        _dense_grad(getattr(r, n), f"{what} {n}")
    need_dx = Cin != 3
    require_small(r.g2, what + " g2")               # exact in both regimes (see above)
    _check_stored(regime, what, small=[(n, getattr(raw, n)) for n in ("a", "y", "g1", "dx")],
                  rounded=[("y", raw.y)] + ([("dx", raw.dx)] if need_dx else []))
    if regime == "round":
        _intermediates_round(raw, what)
    if need_dx:
        assert bool((r.dx != 0).any()), what + ": dx is all zero"
    return SimpleNamespace(x=x, w1=w1, b1=b1, w2=w2, b2=b2, a=a, y=y, pooled=r.pooled, q=r.q, code=r.code, dskip=dskip,
                           dpooled=dpooled, g2=r.g2, g1=r.g1, dx=r.dx if need_dx else None, raw=raw, **s,
                           gw1=s["gw10"] + r.dw1, gb1=s["gb10"] + r.db1, gw2=s["gw20"] + r.dw2, gb2=s["gb20"] + r.db2)


@functools.lru_cache(maxsize=None)
def dec_block_case(regime: str, N: int, h: int, w: int, C: int, seed: int = 0, Hs: int = 0, Ws: int = 0):
    """A decoder block 2C -> C (:func:`dec_block_ref` for the masking convention): x [N, 2C, h, w] and skip
    [N, C, Hs, Ws] are ReLU outputs in {0, 1} (Hs x Ws defaults to 2h x 2w; larger = the centre-crop variant, with
    ``dskip`` zero outside the window).  The transposed conv is thinned to ~8 ternary taps per output with a bias
    in [-2, 2] in BOTH regimes: with an ``up`` of magnitude 2^8 and more the conv outputs behind it grow so large
    that the weight-gradient sums (|g| times them) leave room only for gradients too small to round themselves, so
    ``up`` is exact here and the ``round`` regime starts at conv1's bias: a, y, g1, the concat gradient and dx round.  Fields x, skip, wt, bt, w1,
    b1, w2, b2, up, a, y, g (already times (y > 0)), g1, dskip, gup, dx (masked by x > 0), dx_unmasked, and the
    six parameter gradients gwt / gbt / gw1 / gb1 / gw2 / gb2 on top of integer starts (``gwt0`` ...)."""
    gen = rng(14000 + seed)
    Hs, Ws = Hs or 2 * h, Ws or 2 * w
    what = f"dec block {regime} {(N, h, w, C, Hs, Ws)}"
    x = integers(gen, (N, 2 * C, h, w), 0, 1)
    skip = integers(gen, (N, C, Hs, Ws), 0, 1)
    wt = ternary(gen, (2 * C, C, 2, 2), min(1.0, 8.0 / (2 * C)))
    bt = integers(gen, (C,), -2, 2)
    w1, b1, w2, b2 = _dc_params(gen, regime, 2 * C, C, C)
    up = deconv_fwd_ref(x, wt, bt)
    require_small(up, what + " up")
    top, left = crop_offsets(Hs, Ws, 2 * h, 2 * w)
    cat = torch.cat([skip[:, :, top:top + 2 * h, left:left + 2 * w], up], 1)
    a, y = double_conv_fwd_ref(cat, w1, b1, w2, b2)

    def backward(G):
        g = integers(rng(14500 + 100 * seed + G), y.shape, -G, G) * (y > 0)
        return g, dec_block_ref(x, skip, wt, bt, w1, b1, w2, b2, g, True, what)

    g, r = backward(1) if regime == "small" else _largest_amp(backward)
    s = _starts(gen, gwt0=wt.shape, gbt0=bt.shape, gw10=w1.shape, gb10=b1.shape, gw20=w2.shape, gb20=b2.shape)
    raw_cat = conv_grads_ref(cat, w1, r.g1)[0]
    raw = SimpleNamespace(a=conv_fwd_ref(cat, w1, b1), y=conv_fwd_ref(a, w2, b2),
                          g1=conv_grads_ref(a, w2, g)[0] * (a > 0), dcat=raw_cat,
                          dx=deconv_grads_ref(x, wt, r.gup)[0] * (x > 0))
    _live(a, what + " a"), _live(y, what + " y")
    for n in ("dwt", "dbt", "dw1", "dw2", "db1", "db2"):
        _dense_grad(getattr(r, n), f"{what} {n}")
    assert bool((r.dx != 0).any()) and bool((r.dskip != 0).any()), what + ": dx or dskip is all zero"
    assert not torch.equal(r.dx, r.dx_unmasked)
    _check_stored(regime, what, small=[(n, getattr(raw, n)) for n in ("a", "y", "g1", "dcat", "dx")],
                  rounded=[("y", raw.y), ("dx", raw.dx)])
    if regime == "round":
        _intermediates_round(raw, what)
    return SimpleNamespace(x=x, skip=skip, wt=wt, bt=bt, w1=w1, b1=b1, w2=w2, b2=b2, up=r.up, a=a, y=y, g=g, g1=r.g1,
                           dskip=r.dskip, gup=r.gup, dx=r.dx, dx_unmasked=r.dx_unmasked, raw=raw, crop=(top, left), **s,
                           gwt=s["gwt0"] + r.dwt, gbt=s["gbt0"] + r.dbt, gw1=s["gw10"] + r.dw1, gb1=s["gb10"] + r.db1,
                           gw2=s["gw20"] + r.dw2, gb2=s["gb20"] + r.db2)


# ------------------------------------------------------------------------------------------- the trunk
TRUNK_WIDTHS = (32, 64, 128, 256)        # the ``unet`` preset; the bottleneck is 512 wide


def trunk_names(depth: int = 4):
    """State-dict prefixes of the trunk's layers in forward order: [(prefix, kind)], kind conv / deconv."""
    out = []
    for l in range(depth):
        out += [(f"encoder.conv{l + 1}.conv_block.0", "conv"), (f"encoder.conv{l + 1}.conv_block.2", "conv")]
    out += [("mid.conv_block.0", "conv"), ("mid.conv_block.2", "conv")]
    for i in range(depth):
        out += [(f"decoder.deconv{i + 1}", "deconv"), (f"decoder.conv{i + 1}.conv_block.0", "conv"),
                (f"decoder.conv{i + 1}.conv_block.2", "conv")]
    return out


def trunk_ref(P, img, g, rnd: bool = True, what: str = ""):
    """Encoder -> mid -> decoder of the ``unet`` configuration without the head, as ``run_segment`` drives the
    block Functions, from the parameter dict ``P`` (state-dict names).  ``g``: gradient of the last decoder
    output, multiplied by (y > 0) here.  Gradients between blocks follow the engine's conventions: a decoder
    block returns dx masked by its input's ReLU (so the block below receives a masked gradient, as ``_MidFn`` and
    ``_DecFn`` expect) and dskip unmasked; ``_MidFn`` and ``_EncFn`` (l > 0) return unmasked gradients, which the
    encoder level above masks in its pool backward together with the skip gradient.
    Returns (stored, grads): every stored tensor by name (skip{l}, pooled{l}, enc{l}.a, mid.a, mid.y, dec{i}.up /
    .a / .y, and the backward's dec{i}.dx / .dskip / .g1, mid.dx, enc{l}.g2 / .g1 / .dx) and the unrounded
    gradient of every parameter (state-dict names)."""
    D = len(TRUNK_WIDTHS)
    st, gr = {}, {}
    dc = lambda p: (P[p + ".0.weight"], P[p + ".0.bias"], P[p + ".2.weight"], P[p + ".2.bias"])   # noqa: E731
    x = img
    enc_in = []
    for l in range(D):
        enc_in.append(x)
        a, y = double_conv_fwd_ref(x, *dc(f"encoder.conv{l + 1}.conv_block"), rnd, what and f"{what} enc{l}")
        st[f"enc{l}.a"], st[f"skip{l}"] = a, y
        x, _ = pool_ref(y)
        st[f"pooled{l}"] = x
    mid_in = x
    st["mid.a"], st["mid.y"] = double_conv_fwd_ref(x, *dc("mid.conv_block"), rnd, what and what + " mid")
    # a decoder block's backward needs the gradient from the level above: the whole forward first
    x = st["mid.y"]
    fw = []
    for i in range(D):
        wt, bt = P[f"decoder.deconv{i + 1}.weight"], P[f"decoder.deconv{i + 1}.bias"]
        skip = st[f"skip{D - 1 - i}"]
        up = _rt(deconv_fwd_ref(x, wt, bt), rnd)
        a, y = double_conv_fwd_ref(torch.cat([skip, up], 1), *dc(f"decoder.conv{i + 1}.conv_block"), rnd, "")
        fw.append(x)
        st[f"dec{i}.up"], st[f"dec{i}.a"], st[f"dec{i}.y"] = up, a, y
        x = y
    gy = g
    dskips = {}
    for i in reversed(range(D)):
        p = f"decoder.conv{i + 1}.conv_block"
        r = dec_block_ref(fw[i], st[f"skip{D - 1 - i}"], P[f"decoder.deconv{i + 1}.weight"],
                          P[f"decoder.deconv{i + 1}.bias"], *dc(p), gy, rnd, what and f"{what} dec{i}")
        assert torch.equal(r.y, st[f"dec{i}.y"])
        st[f"dec{i}.dx"], st[f"dec{i}.dskip"], st[f"dec{i}.g1"] = r.dx, r.dskip, r.g1
        gr[f"decoder.deconv{i + 1}.weight"], gr[f"decoder.deconv{i + 1}.bias"] = r.dwt, r.dbt
        gr[p + ".0.weight"], gr[p + ".0.bias"], gr[p + ".2.weight"], gr[p + ".2.bias"] = r.dw1, r.db1, r.dw2, r.db2
        dskips[D - 1 - i] = r.dskip
        gy = r.dx                          # masked by (x > 0): the block below gets its output gradient masked
    r = double_conv_bwd_ref(mid_in, st["mid.a"], P["mid.conv_block.0.weight"], P["mid.conv_block.2.weight"], gy, rnd,
                            what and what + " mid")
    st["mid.g1"], st["mid.dx"] = r.g1, r.dx
    p = "mid.conv_block"
    gr[p + ".0.weight"], gr[p + ".0.bias"], gr[p + ".2.weight"], gr[p + ".2.bias"] = r.dw1, r.db1, r.dw2, r.db2
    dpooled = r.dx
    for l in reversed(range(D)):
        p = f"encoder.conv{l + 1}.conv_block"
        y, a = st[f"skip{l}"], st[f"enc{l}.a"]
        _, q = pool_ref(y)
        g2 = _rt((dskips[l] + pool_route(dpooled, q, *y.shape[2:])) * (y > 0), rnd)
        r = double_conv_bwd_ref(enc_in[l], a, P[p + ".0.weight"], P[p + ".2.weight"], g2, rnd, what and f"{what} enc{l}")
        st[f"enc{l}.g2"], st[f"enc{l}.g1"], st[f"enc{l}.dx"] = g2, r.g1, r.dx
        gr[p + ".0.weight"], gr[p + ".0.bias"], gr[p + ".2.weight"], gr[p + ".2.bias"] = r.dw1, r.db1, r.dw2, r.db2
        dpooled = r.dx
    return st, gr


@functools.lru_cache(maxsize=None)
def trunk_case(regime: str, N: int, H: int, W: int, seed: int = 0):
    """The whole trunk of ``unet`` (widths 32 .. 512, nine DoubleConvs, four transposed convs, no head): input in
    [0, 3], ternary weights thinned to ~3 (``small``) or ~4 (``round``) taps per output, biases in {0, 1},
    output gradient in {-1, 0, 1}.  ``small``: no stored tensor rounds.  ``round``: the activations grow past 2^8
    in the last two decoder blocks, whose up / a / y tensors round (the last decoder output in at least 64
    places); with a gradient in {-1, 0, 1} NO stored gradient of the backward rounds in either regime -- gradient
    rounding is pinned by the ``round`` block cases, not here.  The parameter gradients differ between the regimes
    through the rounded activations.  Fields img, P (parameters), g (times (y > 0)), y (last decoder output),
    stored, G0 (integer start of every parameter gradient, the head's included) and G (start + reference)."""
    gen = rng(15000 + seed)
    what = f"trunk {regime} {(N, H, W)}"
    taps = 3.0 if regime == "small" else 4.0
    P = {}
    chans = {}
    cin = 3
    for l, wd in enumerate(TRUNK_WIDTHS):
        chans[f"encoder.conv{l + 1}.conv_block.0"], chans[f"encoder.conv{l + 1}.conv_block.2"] = (wd, cin), (wd, wd)
        cin = wd
    chans["mid.conv_block.0"], chans["mid.conv_block.2"] = (2 * cin, cin), (2 * cin, 2 * cin)
    cin = 2 * cin
    for i, wd in enumerate(reversed(TRUNK_WIDTHS)):
        chans[f"decoder.deconv{i + 1}"] = (cin, wd)
        chans[f"decoder.conv{i + 1}.conv_block.0"], chans[f"decoder.conv{i + 1}.conv_block.2"] = (wd, 2 * wd), (wd, wd)
        cin = wd
    for name, kind in trunk_names():
        c0, c1 = chans[name]
        if kind == "conv":
            P[name + ".weight"] = ternary(gen, (c0, c1, 3, 3), min(1.0, taps / (9 * c1)))
            P[name + ".bias"] = integers(gen, (c0,), 0, 1)
        else:
            P[name + ".weight"] = ternary(gen, (c0, c1, 2, 2), min(1.0, taps / c0))
            P[name + ".bias"] = integers(gen, (c1,), 0, 1)
    img = integers(gen, (N, 3, H, W), 0, 3)
    y = trunk_ref(P, img, torch.zeros(N, TRUNK_WIDTHS[0], H, W, dtype=torch.float64))[0]["dec3.y"]
    g = integers(gen, y.shape, -1, 1) * (y > 0)
    stored, grads = trunk_ref(P, img, g, True, what)
    raw_y = conv_fwd_ref(stored["dec3.a"], P["decoder.conv4.conv_block.2.weight"], P["decoder.conv4.conv_block.2.bias"])
    if regime == "small":
        for k, t in stored.items():
            if t is not None:
                require_small(t, f"{what} {k}")
        require_small(raw_y, what + " y before rounding")
        _, unrounded = trunk_ref(P, img, g, False)
        for k in grads:
            assert torch.equal(grads[k], unrounded[k]), f"{what}: {k} depends on a rounding"
    else:
        assert rounding_census(raw_y)[1] >= 64, what + ": the last decoder output does not round"
    for k, t in grads.items():
        _dense_grad(t, f"{what} {k}")
    G0 = {k: integers(gen, tuple(t.shape), -8, 8) for k, t in grads.items()}
    G0["segmap.weight"], G0["segmap.bias"] = integers(gen, (1, TRUNK_WIDTHS[0], 1, 1), -8, 8), integers(gen, (1,), -8, 8)
    G = {k: G0[k] + grads.get(k, 0) for k in G0}
    return SimpleNamespace(img=img, P=P, g=g, y=y, stored=stored, G0=G0, G=G)


# ------------------------------------------------------------------------------------------- guarded GPU buffers
class Guarded:
    """An NHWC tensor ``view`` [N, H, W, C] inside a larger allocation the test owns: one guard image before and
    one after, ``lead`` / ``trail`` guard channels on either side (a concat half), all pre-filled with ``fill``.
    ``data`` (NHWC, any float dtype, CPU) initialises the view; without it the view holds ``fill`` too, so an
    element the kernel never writes shows as a mismatch.  :meth:`check` asserts the guards are untouched."""

    def __init__(self, N, H, W, C, dtype, fill, lead: int = 0, trail: int = 0, data=None, device="cuda"):
        self.fill, self.sl = fill, (slice(1, N + 1), slice(None), slice(None), slice(lead, lead + C))
        self.buf = torch.full((N + 2, H, W, lead + C + trail), fill, dtype=dtype, device=device)
        self.view = self.buf[self.sl]
        if data is not None:
            assert tuple(data.shape) == (N, H, W, C), (tuple(data.shape), (N, H, W, C))
            self.view.copy_(data.to(dtype))
            self.data = self.view.clone()
        else:
            self.data = None

    def check(self, what: str) -> None:
        c = self.buf.clone()
        c[self.sl] = self.fill
        bad = c != self.fill
        if bool(bad.any()):
            idx = bad.nonzero()[:6].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} guard elements overwritten, first (image+1, h, w, c): {idx}")
        if self.data is not None:
            assert torch.equal(self.view, self.data), f"{what}: the kernel modified an input"


class GuardedFlat:
    """A flat tensor ``view`` [n] between two 64-element guard runs (fp32 weight / bias gradients)."""

    def __init__(self, n, dtype, fill, data=None, device="cuda"):
        self.fill, self.n = fill, n
        self.buf = torch.full((n + 128,), fill, dtype=dtype, device=device)
        self.view = self.buf[64:64 + n]
        if data is not None:
            self.view.copy_(data.reshape(-1).to(dtype))

    def check(self, what: str) -> None:
        g = torch.cat([self.buf[:64], self.buf[64 + self.n:]])
        assert bool((g == self.fill).all()), f"{what}: guard elements around a flat output overwritten"


# ------------------------------------------------------------------------------------------- comparison
def _histogram(v: torch.Tensor, m: int) -> str:
    cnt = torch.bincount(v % m, minlength=m)
    top = cnt.argsort(descending=True)[:8]
    return "{" + ", ".join(f"{int(r)}: {int(cnt[r])}" for r in sorted(top.tolist()) if cnt[r] > 0) + "}"


def mismatch_report(got: torch.Tensor, ref: torch.Tensor, what: str) -> str:
    bad = got != ref
    idx = bad.nonzero()
    n = idx.shape[0]
    lines = [f"{what}: {n} of {got.numel()} elements differ (shape {tuple(got.shape)}, {got.dtype})"]
    names = "(n, h, w, c)" if got.dim() == 4 else "index"
    for i in idx[:8].tolist():
        lines.append(f"  {names} {tuple(i)}: got {got[tuple(i)].item()!r}, expected {ref[tuple(i)].item()!r}")
    if got.dim() == 4 and n:
        N, H, W, C = got.shape
        ni, h, w, c = idx.unbind(1)
        for m in (32, 64, 128):
            lines.append(f"  w mod {m}: {_histogram(w, m)}")
        lines.append(f"  first row: {int((h == 0).sum())}, last row: {int((h == H - 1).sum())}, first column: "
                     f"{int((w == 0).sum())}, last column: {int((w == W - 1).sum())}, last 8 channels: "
                     f"{int((c >= C - 8).sum())}")
        lines.append(f"  per image: {torch.bincount(ni, minlength=N).tolist()}, rows hit: {h.unique().tolist()[:16]}, "
                     f"c mod 32: {_histogram(c, 32)}")
        d = (got.double() - ref.double())[bad]
        lines.append(f"  got - expected: min {float(d.min())!r}, max {float(d.max())!r}")
    return "\n".join(lines)


def assert_exact(got: torch.Tensor, ref: torch.Tensor, what: str) -> None:
    """``got`` (any device) must equal ``ref`` element for element (0.0 == -0.0); same shape and dtype.  The
    failure message says where the mismatches are, so that the bug can be located without a second run."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, tuple(got.shape), got.dtype, tuple(ref.shape), ref.dtype)
    if not torch.equal(got, ref):
        raise AssertionError(mismatch_report(got, ref, what))
