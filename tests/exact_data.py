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


def require_acc_exact(bound: torch.Tensor, what: str) -> None:
    """``bound`` = the sum of |terms| (+ |bias|) per output: below 2^24 every partial sum, in any order, is an
    integer fp32 holds exactly."""
    m = float(bound.max())
    assert m < ACC_LIMIT, f"{what}: sum of |terms| reaches {m:.0f} >= 2^24 -- fp32 partial sums would not be exact"


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
