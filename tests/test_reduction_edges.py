"""The per-channel reductions next to the conv GEMMs at their edges: BatchNorm statistics / apply / backward in
both engines (csrc/norm_up.hip), the fp32 bilinear x2 and channel sums -- each against a float64 reference
computed on the CPU from the very tensor the kernel read (the bf16-rounded values for the bf16 engine).

Rules of this file: every channel is compared on its own scale (never normalised by a maximum over channels);
"coverage" cases (grid-stride loops, ragged ends, several blocks in y) use small index-dependent integers whose
partial sums stay below 2^24, so any summation order is exact in fp32 and a dropped, duplicated or mis-indexed
element shows as an inequality; bounds are derived from the arithmetic and written next to their use.

The bf16 BatchNorm coverage and the host bindings are in test_reduction_edges_bf16.py, the head / loss and slab
plumbing cases in test_reduction_edges_head.py; both import the helpers below."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # fp32 unit roundoff


# ------------------------------------------------------------------------------------------ helpers
def ints(P, C, a=7, b=3, m=9):
    """[P, C] index-dependent integers in [-(m // 2), m // 2] as float32."""
    p = torch.arange(P, dtype=torch.int32).view(P, 1)
    c = torch.arange(C, dtype=torch.int32).view(1, C)
    return ((a * p + b * c) % m - m // 2).float()


def ulp_bf16(v):
    """Spacing of bf16 at |v| (0 at 0)."""
    _, e = torch.frexp(v.abs().double())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8) * (v != 0)


def ulp_f32(v):
    _, e = torch.frexp(v.abs().double())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 24) * (v != 0)


def within(got, ref, tol, what):
    """|got - ref| <= tol elementwise (float64, CPU); returns the largest |err| / tol for the record."""
    got, ref, tol = got.detach().double().cpu(), ref.double().cpu(), tol.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    err = (got - ref).abs()
    bad = err > tol
    if bad.any():
        i = int((err - tol).argmax())
        idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; worst at {idx}: got "
                             f"{got[idx].item():.9g} ref {ref[idx].item():.9g} err {err[idx].item():.3g} "
                             f"tol {tol[idx].item():.3g}")
    return float((err / tol.clamp_min(1e-300)).max())


def rel_per_channel(got, ref, rtol, what, floor=None):
    """Per channel: |got_c - ref_c| <= rtol |ref_c| (+ floor_c)."""
    ref = ref.double().cpu()
    tol = rtol * ref.abs() + (0 if floor is None else floor.double().cpu())
    return within(got, ref, tol, what)


def bn_ref64(z64, g64, gamma64, beta64, eps):
    """float64 training-mode batch norm of [P, C] and its autograd: mean, biased var, y (no ReLU), dz, dgamma, dbeta."""
    zr = z64.clone().requires_grad_(True)
    ga, be = gamma64.clone().requires_grad_(True), beta64.clone().requires_grad_(True)
    y = F.batch_norm(zr, None, None, ga, be, training=True, eps=eps)
    dz = dgam = dbet = None
    if g64 is not None:
        dz, dgam, dbet = torch.autograd.grad(y, (zr, ga, be), g64)
    return z64.mean(0), z64.var(0, unbiased=False), y.detach(), dz, dgam, dbet


def make_bn(C, gamma, beta, dtype_dev="cuda", **kw):
    bn = torch.nn.BatchNorm2d(C, **kw)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        if bn.running_mean is not None:
            bn.running_mean.fill_(0.3)
            bn.running_var.fill_(1.7)
    return bn.to(dtype_dev)


def gammas(C):
    """Negative, small and ordinary scales."""
    base = torch.tensor([-0.7, 1e-2, 1.0, 1.5, -1.2, 0.3, 2.0, -1e-2])
    return base.repeat(-(-C // 8))[:C].clone()


def betas(C):
    return torch.linspace(-0.5, 0.5, C)


def place(t, dtype, sliced):
    """[N, H, W, C] CPU float -> device tensor of ``dtype``: dense, or the upper half of a 2C-wide buffer filled
    with a sentinel pattern.  Returns (view, buffer or None, buffer clone or None)."""
    N, H, W, C = t.shape
    if not sliced:
        return t.to(dtype).cuda().contiguous(), None, None
    buf = ints(N * H * W, 2 * C, 5, 11, 13).view(N, H, W, 2 * C).to(dtype).cuda()
    buf[..., C:] = t.to(dtype).cuda()
    return buf[..., C:], buf, buf.clone()


def untouched(buf, keep, C, what, whole=False):
    """The lower half (or the whole buffer, for an input) is bit-identical to its clone."""
    if buf is None:
        return
    a, b = (buf, keep) if whole else (buf[..., :C], keep[..., :C])
    assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                       b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), f"{what}: neighbour half changed"


RATIOS = {}     # largest observed error / bound per quantity (printed; the numbers quoted in the comments below)


def note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"[ratio] {key}: {r:.3f}")


def check_bn_apply(y, z64, mean64, invstd64, gamma64, beta64, relu, out_dtype, what):
    """y = relu?(fma(z, sc, sh)), sc = fl(gamma invstd), sh = fl(beta - mean sc): with the (mean, invstd) the kernel
    itself used, four fp32 roundings touch each of the terms z sc, mean sc, beta at most once each, so
        |y - ((z - mean) invstd gamma + beta)| <= 4 * 2^-24 (|z sc| + |mean sc| + |beta|)
    plus, for the bf16 engine, one bf16 rounding of the stored value.  Largest observed ratio to this bound on an
    MI355X: 0.47 (fp32), 1.00 (bf16: the rounding of the store, ties included)."""
    sc = gamma64 * invstd64
    ref = (z64 - mean64) * sc + beta64
    tol = 4 * U * ((z64 * sc).abs() + (mean64 * sc).abs() + beta64.abs())
    if relu:
        ref = ref.clamp_min(0)
    if out_dtype == torch.bfloat16:
        tol = tol + 0.5 * ulp_bf16(ref)
    note(what.split(":")[0] + ".y", within(y.reshape(ref.shape), ref, tol, what))


def check_bn_bwd_f32(dz, z64, g64, saved, gamma64, dgam, dbet, P, what):
    """fp32 dz = fma(c0, g, fma(c1, z, c2)) with c0 = sc, c1 = b = -sc invstd sgx / P, c2 = -sc sg / P - b mean,
    from the kernel's own saved (mean, invstd) and the sums (sg, sgx) it returned: every term of
    sc g + b z - b mean - sc sg / P carries at most 8 fp32 roundings (3 products and 1 / P in b, one more in b mean,
    two fmas), so |dz - exact| <= 8 * 2^-24 (|sc g| + |b z| + |b mean| + |sc sg / P|).
    Largest observed ratio on an MI355X: 0.34."""
    mean, invstd = saved[:gamma64.numel()].double().cpu(), saved[gamma64.numel():].double().cpu()
    sg, sgx = dbet.double().cpu(), dgam.double().cpu()
    sc = gamma64 * invstd
    b = -sc * invstd * sgx / P
    ref = sc * g64 + b * z64 - b * mean - sc * sg / P
    tol = 8 * U * ((sc * g64).abs() + (b * z64).abs() + (b * mean).abs() + (sc * sg / P).abs())
    note(what.split(":")[0] + ".dz", within(dz.reshape(ref.shape), ref, tol, what))


def check_bn_bwd_bf16(dz, z64, g64, gamma64, beta64, eps, dgam, dbet, P, what, dgam_tol=None):
    """bf16 engine against float64 autograd: dz within 2 bf16 ulp of the reference's magnitude per element, on top
    of what the kernel's fp32 arithmetic can resolve where the three terms of dz = c0 g + c1 z + c2 cancel
    (c0 = sc, c1 = -sc invstd sum(g xhat) / P, c2 = -sc sum(g) / P - c1 mean): 8 fp32 roundings of each term taken
    raw, 8 * 2^-24 (|c0 g| + |c1 z| + |c1 mean| + |sc sum(g) / P|), as in check_bn_bwd_f32.  Largest observed ratio
    to this bound on an MI355X: 0.25 on the plain path at every shape and |mean| / sigma up to 1000 (the half ulp of
    the bf16 store), 0.50 on the fused path with its ``dgam_tol``.
    dgamma / dbeta: rtol 1e-3 per channel on top of one fp32 ulp of sum |term| (no fp32 summation does better).
    ``dgam_tol`` (fused partials): the per-channel absolute tolerance of sum g xhat asserted by the caller, carried
    into dz through its xhat term; dgamma itself is then not checked."""
    mean, var, _, dz_ref, dgam_ref, dbet_ref = bn_ref64(z64, g64, gamma64, beta64, eps)
    invstd = (var + eps).rsqrt()
    xhat = (z64 - mean) * invstd
    sc = gamma64 * invstd
    c1 = -sc * invstd * dgam_ref / P
    tol = 2 * ulp_bf16(dz_ref) + 8 * U * ((sc * g64).abs() + (c1 * z64).abs() + (c1 * mean).abs() + (sc * dbet_ref / P).abs())
    if dgam_tol is not None:
        tol = tol + (sc * xhat / P).abs() * dgam_tol
    note(what + ".dz", within(dz.reshape(dz_ref.shape), dz_ref, tol, what + ": dz"))
    if dgam_tol is None:
        rel_per_channel(dgam, dgam_ref, 1e-3, what + ": dgamma", floor=U * (g64 * xhat).abs().sum(0))
    rel_per_channel(dbet, dbet_ref, 1e-3, what + ": dbeta", floor=U * g64.abs().sum(0))
    return dz_ref, dgam_ref, dbet_ref


# ------------------------------------------------------------------------------------------ A. fp32 BN
F32_BN_SHAPES = [(2, 5, 7, 4),          # G = 1, R = 256, a single block
                 (1, 9, 13, 12),        # C / 4 = 3: G = 1, grid.y = 3
                 (3, 16, 16, 32),       # ordinary
                 (1, 67, 65, 512),      # G = 32, grid.y = 4; P = 4355 > 512 * 8: the stride loop runs
                 (1, 363, 362, 4)]      # P = 131406 > 512 * 256: the stride loop at G = 1


def bn_inputs(N, H, W, C, integer, seed):
    P = N * H * W
    if integer:
        return ints(P, C), ints(P, C, 5, 2, 7)
    gen = torch.Generator().manual_seed(seed)
    m = torch.linspace(0.5, 2.0, C) * torch.tensor([1.0, -1.0]).repeat(-(-C // 2))[:C]   # |mean| >= 0.5
    s = torch.linspace(0.5, 2.0, C).flip(0)
    return torch.randn(P, C, generator=gen) * s + m, torch.randn(P, C, generator=gen)


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("N,H,W,C", F32_BN_SHAPES)
def test_f32_bn_fwd_bwd(hip_lib, N, H, W, C, sliced):
    from distributedpytorch_amd.ops import fp32 as F32
    P = N * H * W
    integer = P > 4000
    z, g = bn_inputs(N, H, W, C, integer, seed=C + P)
    z64, g64 = z.double(), g.double()
    gamma, beta = gammas(C), betas(C)
    g64_, b64_ = gamma.double(), beta.double()
    bn = make_bn(C, gamma, beta)
    eps = bn.eps
    zd, zbuf, zkeep = place(z.view(N, H, W, C), torch.float32, sliced)
    gd, gbuf, gkeep = place(g.view(N, H, W, C), torch.float32, sliced)
    yd, ybuf, ykeep = place(torch.zeros(N, H, W, C), torch.float32, sliced)
    mean, var, _, _, dgam_ref, dbet_ref = bn_ref64(z64, g64, g64_, b64_, eps)
    invstd = (var + eps).rsqrt()

    # training, no ReLU: statistics, running statistics, y
    y, saved = F32.bn_fwd(zd, bn, True, relu=False, y=yd)
    torch.cuda.synchronize()
    assert y.data_ptr() == yd.data_ptr() and int(bn.num_batches_tracked) == 1
    sv = saved.double().cpu()
    if integer:     # exact sums: the mean is float32(sum z / P) up to the double rounding of pivot + s / P
        within(sv[:C], mean.float(), ulp_f32(mean.float()), "f32 saved mean (integer)")
    rel_per_channel(sv[:C], mean, 1e-5, "f32 saved mean", floor=0.5 * ulp_f32(mean))
    rel_per_channel(sv[C:], invstd, 1e-5, "f32 invstd")
    # rtol 1e-5 of the result, on top of the four fp32 roundings of (1 - m) rm + m mean on its summands
    rel_per_channel(bn.running_mean, 0.9 * 0.3 + 0.1 * mean, 1e-5, "f32 running_mean",
                    floor=4 * U * (0.9 * 0.3 + (0.1 * mean).abs()))
    rel_per_channel(bn.running_var, 0.9 * 1.7 + 0.1 * var * P / (P - 1), 1e-5, "f32 running_var")
    check_bn_apply(y, z64, sv[:C], sv[C:], g64_, b64_, False, torch.float32, "f32: train y")
    untouched(ybuf, ykeep, C, "y")

    # training with ReLU (second step), then eval with the running statistics now in the module
    y, saved2 = F32.bn_fwd(zd, bn, True, relu=True, y=yd)
    torch.cuda.synchronize()
    assert int(bn.num_batches_tracked) == 2 and torch.equal(saved2, saved)
    check_bn_apply(y, z64, sv[:C], sv[C:], g64_, b64_, True, torch.float32, "f32: train relu y")
    rm, rv = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    rinv = 1.0 / (rv + eps).float().sqrt().double()          # the kernel's 1 / sqrtf(var + eps): 2 more roundings
    for relu in (False, True):
        y, none = F32.bn_fwd(zd, bn, False, relu=relu, y=yd)
        torch.cuda.synchronize()
        assert none is None and int(bn.num_batches_tracked) == 2
        tol_extra = 3 * U * ((z64 - rm) * rinv * g64_).abs()
        sc = g64_ * rinv
        ref = (z64 - rm) * sc + b64_
        tol = 4 * U * ((z64 * sc).abs() + (rm * sc).abs() + b64_.abs()) + tol_extra
        note("f32.eval_y", within(y.reshape(P, C), ref.clamp_min(0) if relu else ref, tol, f"f32: eval y relu={relu}"))
    assert torch.equal(bn.running_mean.double().cpu(), rm) and torch.equal(bn.running_var.double().cpu(), rv)
    untouched(ybuf, ykeep, C, "y")
    untouched(zbuf, zkeep, C, "z", whole=True)

    # backward: zero start (the kernel's own sums), then accumulation onto a non-zero start (bit-exact add)
    dgam, dbet = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dz = F32.bn_bwd(gd, zd, saved, bn, dgam, dbet)
    torch.cuda.synchronize()
    xhat = (z64 - mean) * invstd
    if integer:
        assert torch.equal(dbet.double().cpu(), g64.sum(0)), "f32 dbeta (integer): not the exact sum"
    rel_per_channel(dgam, dgam_ref, 1e-4, "f32 dgamma", floor=U * (g64 * xhat).abs().sum(0))
    rel_per_channel(dbet, dbet_ref, 1e-4, "f32 dbeta", floor=U * g64.abs().sum(0))
    check_bn_bwd_f32(dz, z64, g64, saved, g64_, dgam, dbet, P, "f32: dz")
    dgam2, dbet2 = torch.full((C,), -1.5, device="cuda"), torch.full((C,), 0.25, device="cuda")
    dz2 = F32.bn_bwd(gd, zd, saved, bn, dgam2, dbet2)
    torch.cuda.synchronize()
    assert torch.equal(dz2, dz) and torch.equal(dgam2, dgam - 1.5) and torch.equal(dbet2, dbet + 0.25)
    untouched(gbuf, gkeep, C, "g", whole=True)
    untouched(zbuf, zkeep, C, "z", whole=True)


# ------------------------------------------------------------------------------------------ A. fp32 bilinear x2
def up_ref64(x_nhwc64):
    return F.interpolate(x_nhwc64.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear",
                         align_corners=False).permute(0, 2, 3, 1)


@pytest.mark.parametrize("N,h,w,C,half", [(1, 1, 1, 4, False), (1, 1, 5, 8, False), (2, 7, 1, 4, False),
                                          (2, 4, 6, 32, False), (1, 33, 31, 64, True)])
def test_f32_up2_fwd_bwd(hip_lib, N, h, w, C, half):
    """The weights are dyadic (1/4, 3/4, 1/16, ...), so every product is exact and only the three additions of the
    forward round: |y - ref| <= 4 * 2^-24 sum |w_i x_i| (observed ratio 0.67).  The backward gathers at most 16
    taps with one fma each: 16 * 2^-24 sum |w_i g_i| (observed 0.22)."""
    from distributedpytorch_amd.ops import fp32 as F32
    gen = torch.Generator().manual_seed(N * 100 + h)
    x = torch.randn(N, h, w, C, generator=gen)
    g = torch.randn(N, 2 * h, 2 * w, C, generator=gen)
    x64 = x.double().requires_grad_(True)
    ref = up_ref64(x64)
    (dx_ref,) = torch.autograd.grad(ref, (x64,), g.double())
    xa = x.double().abs().requires_grad_(True)
    mag = up_ref64(xa)
    (dmag,) = torch.autograd.grad(mag, (xa,), g.double().abs())
    yd, ybuf, ykeep = place(torch.zeros(N, 2 * h, 2 * w, C), torch.float32, half)
    gd, gbuf, gkeep = place(g, torch.float32, half)
    y = F32.up2_fwd(x.cuda(), yd)
    dx = F32.up2_bwd(gd)
    torch.cuda.synchronize()
    note("up2.y", within(y, ref.detach(), 4 * U * mag.detach(), "up2_fwd_f32"))
    note("up2.dx", within(dx, dx_ref, 16 * U * dmag, "up2_bwd_f32"))
    untouched(ybuf, ykeep, C, "y")
    untouched(gbuf, gkeep, C, "g", whole=True)


def test_f32_up2_stride_loop_exact(hip_lib):
    """2 * 513 * 2 * 1025 * (8 / 4) = 4 206 600 items > 16384 * 256: the grid-stride loop takes a second iteration.
    Small integers times dyadic weights are exact, so the result equals float64 bit for bit."""
    from distributedpytorch_amd.ops import fp32 as F32
    N, h, w, C = 1, 513, 1025, 8
    x = ints(N * h * w, C).view(N, h, w, C)
    ref = up_ref64(x.double())
    y = F32.up2_fwd(x.cuda())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), ref)


# ------------------------------------------------------------------------------------------ A. fp32 channel sums
@pytest.mark.parametrize("C", [1, 4, 64, 256, 512])
def test_f32_channel_sum(hip_lib, C):
    """P = 1, 255 and past the grid cap (1024 blocks x 256 / C pixel rows), dense and as a strided slice, onto a
    non-zero ``out``: integer inputs, exact sums."""
    from distributedpytorch_amd.ops import fp32 as F32
    cap = 1024 * max(1, 256 // C)
    for P in (1, 255, cap + 37):
        v = ints(P, C)
        want = (v.double().sum(0) + (torch.arange(C) % 5 - 2).double())
        for sliced in ([True] if C < 4 else [False, True]):       # a 1-channel tensor is only addressable as a slice
            if sliced:
                wide = max(2 * C, 4)
                buf = ints(P, wide, 5, 11, 13).view(1, 1, P, wide).cuda()
                lo = wide - C if C >= 4 else 0
                buf[..., lo:lo + C] = v.view(1, 1, P, C).cuda()
                gd = buf[..., lo:lo + C]
            else:
                gd = v.view(1, 1, P, C).cuda()
            outs = []
            for _ in range(2):
                out = (torch.arange(C) % 5 - 2).float().cuda()
                F32.channel_sum(gd, out)
                torch.cuda.synchronize()
                outs.append(out)
            assert torch.equal(outs[0].double().cpu(), want), (C, P, sliced)
            assert torch.equal(outs[0], outs[1])


def test_f32_channel_sum_rejects_c24(hip_lib):
    from distributedpytorch_amd.ops import fp32 as F32
    out = torch.zeros(24, device="cuda")
    with pytest.raises(RuntimeError, match=r"channel_sum_f32 failed: hip error 1 "):     # hipErrorInvalidValue
        F32.channel_sum(torch.ones(1, 2, 3, 24, device="cuda"), out)
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0


# ------------------------------------------------------------------------------------------ B. conditioning
COND = [(0.0, 1.0), (10.0, 1.0), (100.0, 1.0), (1000.0, 1.0), (-300.0, 1.0), (3.0, 1e-2), None]   # None: constant


def cond_data(engine, seed=0):
    """(2, 32, 64, 32): channel c ~ N(m, s) cycling through COND ((3, 1e-2) fp32 only; the constant channel is
    100.5 in bf16, 100.3 in fp32), rounded to the engine's storage type."""
    P, C = 2 * 32 * 64, 32
    gen = torch.Generator().manual_seed(seed)
    kinds = [k for k in COND if not (engine == "bf16" and k == (3.0, 1e-2))]
    z = torch.empty(P, C)
    const = []
    for c in range(C):
        k = kinds[c % len(kinds)]
        if k is None:
            z[:, c] = 100.5 if engine == "bf16" else 100.3
            const.append(c)
        else:
            z[:, c] = torch.randn(P, generator=gen) * k[1] + k[0]
    if engine == "bf16":
        z = z.to(torch.bfloat16).float()
    g = torch.randn(P, C, generator=gen)
    if engine == "bf16":
        g = g.to(torch.bfloat16).float()
    return z, g, const, [kinds[c % len(kinds)] for c in range(C)]


def test_f32_bn_statistics_conditioning(hip_lib):
    """Shifted channels (|mean| / sigma up to 1000, and a constant channel) in the fp32 engine: the mean within
    2^-22 max |z_c|, invstd and the unbiased running_var (momentum 1: the batch value itself) to rtol 1e-5 per
    channel.  Raw sums  sum z^2 / P - (sum z / P)^2  lose 2^-24 (mean / sigma)^2 and fail this from |mean| / sigma
    ~ 30; the kernels sum about a per-channel pivot."""
    from distributedpytorch_amd.ops import fp32 as F32
    N, H, W, C = 2, 32, 64, 32
    P = N * H * W
    z, g, const, kinds = cond_data("fp32")
    z64, g64 = z.double(), g.double()
    gamma, beta = gammas(C), betas(C)
    bn = make_bn(C, gamma, beta, momentum=1.0)
    mean, var, _, _, dgam_ref, dbet_ref = bn_ref64(z64, g64, gamma.double(), beta.double(), bn.eps)
    invstd = (var + bn.eps).rsqrt()
    zd = z.view(N, H, W, C).cuda()
    y, saved = F32.bn_fwd(zd, bn, True, relu=True)
    torch.cuda.synchronize()
    sv = saved.double().cpu()
    for c in range(C):
        print(f"[cond f32] c={c} kind={kinds[c]} mean err {abs(sv[c] - mean[c]).item():.3g} invstd rel "
              f"{abs(sv[C + c] / invstd[c] - 1).item():.3g} rvar rel "
              f"{abs(bn.running_var[c].item() / max(var[c].item() * P / (P - 1), 1e-300) - 1):.3g}")
    within(sv[:C], mean, 2.0 ** -22 * z64.abs().amax(0), "f32 mean (conditioning)")
    rel_per_channel(sv[C:], invstd, 1e-5, "f32 invstd (conditioning)")
    rel_per_channel(bn.running_var, var * P / (P - 1), 1e-5, "f32 running_var (conditioning)")
    rel_per_channel(sv[C:][const], torch.full((len(const),), bn.eps, dtype=torch.float64).rsqrt(), 1e-5,
                    "f32 invstd of the constant channel")
    check_bn_apply(y, z64, sv[:C], sv[C:], gamma.double(), beta.double(), True, torch.float32, "f32cond: y")
    within(y.reshape(P, C)[:, const], beta.double()[const].clamp_min(0).expand(P, -1),
           (4 * U * (2 * (z64 * gamma.double() * sv[C:]).abs() + beta.double().abs()))[:, const],
           "f32 constant channel: y = relu(beta)")
    # backward on the same data: its sums are centred by ``saved``
    dgam, dbet = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dz = F32.bn_bwd(g.view(N, H, W, C).cuda(), zd, saved, bn, dgam, dbet)
    torch.cuda.synchronize()
    xhat = (z64 - mean) * invstd
    rel_per_channel(dgam, dgam_ref, 1e-4, "f32 dgamma (conditioning)", floor=U * (g64 * xhat).abs().sum(0))
    rel_per_channel(dbet, dbet_ref, 1e-4, "f32 dbeta (conditioning)", floor=U * g64.abs().sum(0))
    check_bn_bwd_f32(dz, z64, g64, saved, gamma.double(), dgam, dbet, P, "f32cond: dz")


def test_bf16_bn_statistics_conditioning(hip_lib):
    """The same for the bf16 engine at its own tolerances (mean rtol 1e-5 / atol 1e-6, invstd and running_var rtol
    1e-3), against float64 statistics of the bf16-rounded data.  Raw fp32 sums fail at |mean| / sigma = 1000."""
    from distributedpytorch_amd.ops import kernels as K
    N, H, W, C = 2, 32, 64, 32
    P = N * H * W
    z, g, const, kinds = cond_data("bf16")
    z64, g64 = z.double(), g.double()
    gamma, beta = gammas(C), betas(C)
    bn = make_bn(C, gamma, beta, momentum=1.0)
    mean, var = z64.mean(0), z64.var(0, unbiased=False)
    invstd = (var + bn.eps).rsqrt()
    zd = z.view(N, H, W, C).to(torch.bfloat16).cuda()
    y = torch.empty_like(zd)
    saved = K.bn_fwd(zd, y, bn, train=True, relu=True)
    torch.cuda.synchronize()
    sv = saved.double().cpu()
    for c in range(C):
        print(f"[cond bf16] c={c} kind={kinds[c]} mean rel {abs(sv[c] / mean[c] - 1).item():.3g} invstd rel "
              f"{abs(sv[C + c] / invstd[c] - 1).item():.3g} rvar rel "
              f"{abs(bn.running_var[c].item() / max(var[c].item() * P / (P - 1), 1e-300) - 1):.3g}")
    within(sv[:C], mean, 1e-5 * mean.abs() + 1e-6, "bf16 mean (conditioning)")
    rel_per_channel(sv[C:], invstd, 1e-3, "bf16 invstd (conditioning)")
    rel_per_channel(bn.running_var, var * P / (P - 1), 1e-3, "bf16 running_var (conditioning)")
    rel_per_channel(sv[C:][const], torch.full((len(const),), bn.eps, dtype=torch.float64).rsqrt(), 1e-3,
                    "bf16 invstd of the constant channel")
    check_bn_apply(y, z64, sv[:C], sv[C:], gamma.double(), beta.double(), True, torch.bfloat16, "bf16cond: y")
    bref = beta.to(torch.bfloat16).double()      # relu(beta) as stored
    within(y.reshape(P, C)[:, const], beta.double()[const].clamp_min(0).expand(P, -1),
           (4 * U * (2 * (z64 * gamma.double() * sv[C:]).abs() + beta.double().abs()) + ulp_bf16(bref))[:, const],
           "bf16 constant channel: y = relu(beta)")
    dgam, dbet = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dz = K.bn_bwd(g.view(N, H, W, C).to(torch.bfloat16).cuda(), zd, saved, bn, dgam, dbet)
    torch.cuda.synchronize()
    check_bn_bwd_bf16(dz, z64, g64, gamma.double(), beta.double(), bn.eps, dgam, dbet, P, "bf16 (conditioning)")


def test_conv_epilogue_statistics_at_ratio_10(hip_lib):
    """The conv epilogues' slabs carry raw sums (pivot 0): the fused-statistics path is specified to |mean| / sigma
    ~ 10.  A bias of 10 standard deviations of the conv output, (1, 7, 64, 64 -> 32): the bf16 tolerances hold."""
    from distributedpytorch_amd.ops import kernels as K
    N, H, W, Cin, Cout = 1, 7, 64, 64, 32
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(N, Cin, H, W, generator=gen).to(torch.bfloat16).float()
    w = (torch.randn(Cout, Cin, 3, 3, generator=gen) * (2.0 / (9 * Cin)) ** 0.5).to(torch.bfloat16).float()
    std = F.conv2d(x, w, None, padding=1).std().item()
    b = torch.full((Cout,), 10.0 * std) * torch.tensor([1.0, -1.0]).repeat(Cout // 2)
    kf = K.round_up(9 * Cin, 32)
    packed = torch.zeros(Cout, kf)
    packed[:, :9 * Cin] = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    packed = packed.to(torch.bfloat16).cuda().reshape(-1)
    xh = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()
    bn = make_bn(Cout, gammas(Cout), betas(Cout), momentum=1.0)
    z = torch.empty(N, H, W, Cout, dtype=torch.bfloat16, device="cuda")
    stats = []
    K.igemm(xh, packed, z, Ngemm=Cout, Kpad=kf, KH=3, KW=3, stride=1, pad=1, Cs=Cin, out_grid=(N, H, W), bias=b.cuda(),
            relu=False, bn_stats=stats)
    assert len(stats) == 2 and stats[1] > 0, "streaming epilogue did not produce the statistics"
    y = torch.empty_like(z)
    saved = K.bn_fwd(z, y, bn, train=True, stats=stats)
    torch.cuda.synchronize()
    z64 = z.double().cpu().reshape(-1, Cout)
    P = z64.shape[0]
    mean, var = z64.mean(0), z64.var(0, unbiased=False)
    assert 8 < (mean.abs() / var.sqrt()).min().item() and (mean.abs() / var.sqrt()).max().item() < 13
    sv = saved.double().cpu()
    within(sv[:Cout], mean, 1e-5 * mean.abs() + 1e-6, "fused-statistics mean")
    rel_per_channel(sv[Cout:], (var + bn.eps).rsqrt(), 1e-3, "fused-statistics invstd")
    rel_per_channel(bn.running_var, var * P / (P - 1), 1e-3, "fused-statistics running_var")
