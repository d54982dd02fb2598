"""BatchNorm of the bf16 engine at its edges (csrc/norm_up.hip through ops/kernels.py): grid-stride loops and ragged
ends with exact integer inputs, channel-slice inputs, negative / small / zero scales on the plain and the
fused-partials backward, and the host-side semantics both engines share with torch (momentum=None, eval without
running statistics).  Helpers and rules: test_reduction_edges.py."""
import pytest
import torch
import torch.nn.functional as F

from test_reduction_edges import (U, betas, bn_ref64, check_bn_apply, check_bn_bwd_bf16, gammas, ints, make_bn, place,
                                  rel_per_channel, ulp_bf16, ulp_f32, untouched, within)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ C. bf16 BN coverage
@pytest.mark.parametrize("N,H,W,C", [(1, 131, 129, 64),      # P = 16899 > 512 * 32, ragged: bn_partial's stride loop
                                     (1, 9, 13, 96)])        # C / 8 = 12: G = 4, grid.y = 3
def test_bf16_bn_integer_coverage(hip_lib, N, H, W, C):
    from distributedpytorch_amd.ops import kernels as K
    P = N * H * W
    z, g = ints(P, C), ints(P, C, 5, 2, 7)
    z64, g64 = z.double(), g.double()
    gamma, beta = gammas(C), betas(C)
    bn = make_bn(C, gamma, beta)
    zd = z.view(N, H, W, C).to(torch.bfloat16).cuda()
    y = torch.empty_like(zd)
    saved = K.bn_fwd(zd, y, bn, train=True, relu=True)
    dgam, dbet = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dz = K.bn_bwd(g.view(N, H, W, C).to(torch.bfloat16).cuda(), zd, saved, bn, dgam, dbet)
    torch.cuda.synchronize()
    sv = saved.double().cpu()
    mean, var = z64.mean(0), z64.var(0, unbiased=False)
    within(sv[:C], mean.float(), ulp_f32(mean.float()), "bf16 saved mean (integer)")
    rel_per_channel(sv[C:], (var + bn.eps).rsqrt(), 1e-5, "bf16 invstd (integer: exact sums)")
    assert torch.equal(dbet.double().cpu(), g64.sum(0)), "bf16 dbeta (integer): not the exact sum"
    check_bn_apply(y, z64, sv[:C], sv[C:], gamma.double(), beta.double(), True, torch.bfloat16, "bf16int: y")
    check_bn_bwd_bf16(dz, z64, g64, gamma.double(), beta.double(), bn.eps, dgam, dbet, P, "bf16 (integer)")


@pytest.mark.parametrize("pool", [False, True], ids=["apply", "pool"])
def test_bf16_bn_elementwise_stride_loops(hip_lib, pool):
    """(1, 513, 1025, 64): P * 8 items > 16384 * 256, so bn_apply_kernel and bn_bwd_apply_kernel take a second
    iteration of their grid-stride loops.  ``pool`` (even H, W: 514 x 1026): the fused BN + max-pool pass at the same
    size -- it has one item per 2 x 2 window (P / 4 * 8 = 1.05 M here), so its own loop would need a tensor four
    times this one; this case covers its indexing at full width, more than 4096 blocks and a ragged last block.
    Integer z and g: exact sums, every element of y / dz checked against float64, the pooled tensor against
    max_pool2d of the stored y."""
    from distributedpytorch_amd.ops import kernels as K
    N, H, W, C = (1, 514, 1026, 64) if pool else (1, 513, 1025, 64)
    P = N * H * W
    assert pool or P * (C // 8) > 16384 * 256
    z = ints(P, C)
    gamma, beta = gammas(C), betas(C)
    bn = make_bn(C, gamma, beta)
    zd = z.view(N, H, W, C).to(torch.bfloat16).cuda()
    y = torch.empty_like(zd)
    if pool:
        pooled = torch.empty(N, H // 2, W // 2, C, dtype=torch.bfloat16, device="cuda")
        code = torch.empty(N, H // 2, W // 2, C, dtype=torch.uint8, device="cuda")
        saved = K.bn_fwd(zd, y, bn, train=True, relu=True, pool=pooled, pcode=code)
    else:
        saved = K.bn_fwd(zd, y, bn, train=True, relu=True)
    torch.cuda.synchronize()
    sv = saved.double().cpu()
    z64 = z.double()
    mean = z64.mean(0)
    within(sv[:C], mean.float(), ulp_f32(mean.float()), "saved mean (integer)")
    rel_per_channel(sv[C:], (z64.var(0, unbiased=False) + bn.eps).rsqrt(), 1e-5, "invstd (integer)")
    check_bn_apply(y, z64, sv[:C], sv[C:], gamma.double(), beta.double(), True, torch.bfloat16, "bf16big: y")
    if pool:
        yc = y.float().cpu()
        assert torch.equal(pooled.float().cpu(), F.max_pool2d(yc.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        p2 = torch.empty_like(pooled)
        c2 = torch.empty_like(code)
        K.maxpool2(y, p2, c2)
        torch.cuda.synchronize()
        assert torch.equal(p2, pooled) and torch.equal(c2, code)
        return
    del z64
    g = ints(P, C, 5, 2, 7)
    dgam, dbet = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dz = K.bn_bwd(g.view(N, H, W, C).to(torch.bfloat16).cuda(), zd, saved, bn, dgam, dbet)
    torch.cuda.synchronize()
    assert torch.equal(dbet.double().cpu(), g.double().sum(0)), "dbeta (integer): not the exact sum"
    check_bn_bwd_bf16(dz, z.double(), g.double(), gamma.double(), beta.double(), bn.eps, dgam, dbet, P, "bf16 (big)")


@pytest.mark.parametrize("N,H,W,C", [(2, 9, 13, 32), (1, 131, 129, 64)])
def test_bf16_bn_bwd_strided_inputs(hip_lib, N, H, W, C):
    """g and z as the upper halves of 2C-wide tensors (ld != C) in bn_bwd and bn_bwd_coef: bit-equal to dense."""
    from distributedpytorch_amd.ops import kernels as K
    gen = torch.Generator().manual_seed(11)
    z = torch.randn(N, H, W, C, generator=gen) * 1.5 + 0.7
    g = torch.randn(N, H, W, C, generator=gen)
    bn = make_bn(C, gammas(C), betas(C))
    res = []
    for sliced in (False, True):
        zd, zbuf, zkeep = place(z, torch.bfloat16, sliced)
        gd, gbuf, gkeep = place(g, torch.bfloat16, sliced)
        y = torch.empty(N, H, W, C, dtype=torch.bfloat16, device="cuda")
        saved = K.bn_fwd(zd, y, bn, train=True)
        dg1, db1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        dz = K.bn_bwd(gd, zd, saved, bn, dg1, db1)
        dg2, db2 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        coef3 = K.bn_bwd_coef(gd, zd, saved, bn, dg2, db2).clone()
        torch.cuda.synchronize()
        untouched(zbuf, zkeep, C, "z", whole=True)
        untouched(gbuf, gkeep, C, "g", whole=True)
        assert torch.equal(dg1, dg2) and torch.equal(db1, db2)
        res.append((y, saved.clone(), dz, dg1, db1, coef3))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # and the coefficients reproduce dz: dz = bf16(fma(c0, g, fma(c1, z, c2)))
    _, _, dz, _, _, coef3 = res[0]
    c3 = coef3.double().cpu().view(3, C)
    ref = c3[0] * g.to(torch.bfloat16).double() + c3[1] * z.to(torch.bfloat16).double() + c3[2]
    terms = (c3[0] * g.double()).abs() + (c3[1] * z.double()).abs() + c3[2].abs()
    within(dz, ref, 0.5 * ulp_bf16(ref) + 2 * U * terms, "dz from coef3")


def _gamma_case(K, gamma, beta, fused, seed=6, shape=(2, 5, 128, 32, 32)):
    """BN backward of (z, g): plain (g random) or fused (g = the streaming dgrad's output masked by y = relu(bn(z)),
    its epilogue's (sum g, sum g y) partials as ``stats``).  Returns everything on the CPU."""
    from test_hip_kernels import _pack_one
    N, H, W, C1, C2 = shape
    gen = torch.Generator().manual_seed(seed)
    z = (torch.randn(N, H, W, C1, generator=gen) * 1.5 + 0.2).to(torch.bfloat16).cuda()
    bn = make_bn(C1, gamma, beta)
    y = torch.empty_like(z)
    saved = K.bn_fwd(z, y, bn, train=True)
    stats = None
    if fused:
        w2 = torch.randn(C2, C1, 3, 3, generator=gen) * (2.0 / (9 * C1)) ** 0.5
        g2 = torch.randn(N, H, W, C2, generator=gen).to(torch.bfloat16).cuda()
        packed, ng, kp = _pack_one(1, w2)
        g = torch.empty(N, H, W, C1, dtype=torch.bfloat16, device="cuda")
        stats = []
        K.igemm(g2, packed, g, Ngemm=ng, Kpad=kp, KH=3, KW=3, stride=1, pad=1, Cs=C2, out_grid=(N, H, W), mask=y,
                bn_stats=stats)
        assert len(stats) == 2 and stats[1] > 0, "dgrad epilogue did not produce the BN partials"
    else:
        g = torch.randn(N, H, W, C1, generator=gen).to(torch.bfloat16).cuda()
    dgam, dbet = torch.zeros(C1, device="cuda"), torch.zeros(C1, device="cuda")
    dz = K.bn_bwd(g, z, saved, bn, dgam, dbet, stats=stats)
    torch.cuda.synchronize()
    P = N * H * W
    return (z.double().cpu().view(P, C1), g.double().cpu().view(P, C1), y.double().cpu().view(P, C1), dz, dgam, dbet,
            bn.eps, P)


def test_bf16_bn_bwd_gamma_plain(hip_lib):
    """Negative and small scales on the plain backward, per channel against float64 autograd."""
    from distributedpytorch_amd.ops import kernels as K
    C = 32
    gamma, beta = gammas(C), betas(C)
    z64, g64, _, dz, dgam, dbet, eps, P = _gamma_case(K, gamma, beta, fused=False)
    check_bn_bwd_bf16(dz, z64, g64, gamma.double(), beta.double(), eps, dgam, dbet, P, "bf16 plain, gamma mix")


FUSED_SGX_ERR = 2.7e-4     # measured on an MI355X (2.68e-4): error of the recovered sum g xhat / sum |g xhat| at gamma = 1


def test_bf16_bn_bwd_gamma_fused(hip_lib):
    """The fused-partials backward recovers sum g xhat = (sum g y - beta sum g) / gamma, which carries the bf16
    rounding of y divided by gamma.  Its error relative to the channel's scale sum |g xhat| is measured against
    float64 at gamma = 1 (same z, beta, upstream gradient) and must stay within the value recorded on an MI355X,
    FUSED_SGX_ERR; a channel with scale gamma is allowed that recorded value x (1 / |gamma|) x 2."""
    from distributedpytorch_amd.ops import kernels as K
    C = 32
    gamma = gammas(C)
    beta = betas(C)
    beta[gamma.abs() < 0.1] = beta[gamma.abs() < 0.1].abs() + 0.05     # else relu(bn(z)) masks those channels entirely

    def run(gam):
        z64, g64, _, dz, dgam, dbet, eps, P = _gamma_case(K, gam, beta, fused=True)
        mean, var, _, _, dgam_ref, _ = bn_ref64(z64, g64, gam.double(), beta.double(), eps)
        xhat = (z64 - mean) * (var + eps).rsqrt()
        scale = (g64 * xhat).abs().sum(0)
        assert (scale > 0).all(), "a channel's gradient is masked everywhere: nothing to test there"
        return dict(z64=z64, g64=g64, dz=dz, dgam=dgam.double().cpu(), dbet=dbet, eps=eps, P=P, dgam_ref=dgam_ref,
                    scale=scale)

    r1 = run(torch.ones(C))
    e1 = ((r1["dgam"] - r1["dgam_ref"]).abs() / r1["scale"]).max().item()
    print(f"[fused sgx] relative error at gamma = 1: {e1:.3g}")
    assert 0 < e1 <= FUSED_SGX_ERR, e1
    r = run(gamma)
    allowed = 2 * FUSED_SGX_ERR / gamma.double().abs() * r["scale"]
    within(r["dgam"], r["dgam_ref"], allowed, "fused dgamma, gamma mix")
    check_bn_bwd_bf16(r["dz"], r["z64"], r["g64"], gamma.double(), beta.double(), r["eps"], None, r["dbet"], r["P"],
                      "bf16 fused, gamma mix", dgam_tol=allowed)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_bf16_bn_bwd_gamma_zero(hip_lib, fused):
    """A channel with gamma exactly 0 (beta > 0, so its ReLU mask passes the gradient): dz = 0 on both paths; the
    plain path gives the reference dgamma, the fused path -- y = relu(beta) holds no xhat -- a finite one (0)."""
    from distributedpytorch_amd.ops import kernels as K
    C = 32
    gamma, beta = gammas(C), betas(C).abs() + 0.1
    zero = [3, 17]
    gamma[zero] = 0.0
    z64, g64, _, dz, dgam, dbet, eps, P = _gamma_case(K, gamma, beta, fused=fused)
    assert torch.isfinite(dz.float()).all() and torch.isfinite(dgam).all() and torch.isfinite(dbet).all()
    assert (g64[:, zero] != 0).any(), "the zero-gamma channels saw no gradient"
    assert dz.float().cpu().view(P, C)[:, zero].abs().max().item() == 0
    _, _, _, _, dgam_ref, dbet_ref = bn_ref64(z64, g64, gamma.double(), beta.double(), eps)
    rel_per_channel(dbet, dbet_ref, 1e-3, "dbeta", floor=U * g64.abs().sum(0))
    if fused:
        assert dgam.cpu()[zero].abs().max().item() == 0
    else:
        check_bn_bwd_bf16(dz, z64, g64, gamma.double(), beta.double(), eps, dgam, dbet, P, "bf16 plain, gamma 0")


# ------------------------------------------------------------------------------------------ C. host bindings
def _engine_bn_fwd(engine, z, bn, train):
    """(y [P, C] float64 on the CPU, saved or None) through either engine's binding."""
    if engine == "bf16":
        from distributedpytorch_amd.ops import kernels as K
        zd = z.to(torch.bfloat16).cuda()
        y = torch.empty_like(zd)
        saved = K.bn_fwd(zd, y, bn, train=train, relu=False)
    else:
        from distributedpytorch_amd.ops import fp32 as F32
        y, saved = F32.bn_fwd(z.cuda(), bn, train, relu=False)
    torch.cuda.synchronize()
    return y.double().cpu().reshape(-1, z.shape[-1]), saved


@pytest.mark.parametrize("engine", ["bf16", "fp32"])
def test_bn_momentum_none_is_cumulative_average(hip_lib, engine):
    """momentum=None: torch uses 1 / num_batches_tracked (a cumulative average).  Two consecutive training steps."""
    N, H, W, C = 2, 9, 13, 32
    gen = torch.Generator().manual_seed(5)
    zs = [torch.randn(N, H, W, C, generator=gen) * s + m for s, m in ((1.5, 0.7), (0.6, -1.1))]
    if engine == "bf16":
        zs = [z.to(torch.bfloat16).float() for z in zs]
    ref = torch.nn.BatchNorm2d(C, momentum=None).double()
    bn = torch.nn.BatchNorm2d(C, momentum=None).cuda()
    for z in zs:
        ref(z.double().permute(0, 3, 1, 2))
        _engine_bn_fwd(engine, z, bn, True)
    rtol = 1e-3 if engine == "bf16" else 1e-5
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 2
    rel_per_channel(bn.running_mean, ref.running_mean, 1e-5, f"{engine} running_mean", floor=torch.full((C,), 1e-6))
    rel_per_channel(bn.running_var, ref.running_var, rtol, f"{engine} running_var")


@pytest.mark.parametrize("engine", ["bf16", "fp32"])
def test_bn_eval_without_running_stats_uses_batch_statistics(hip_lib, engine):
    """track_running_stats=False: eval normalises with the batch statistics, as torch does (the host binding must
    not hand the kernel null running statistics to read)."""
    N, H, W, C = 2, 9, 13, 32
    gen = torch.Generator().manual_seed(6)
    z = torch.randn(N, H, W, C, generator=gen) * 1.5 + 0.7
    if engine == "bf16":
        z = z.to(torch.bfloat16).float()
    gamma, beta = gammas(C), betas(C)
    bn = make_bn(C, gamma, beta, track_running_stats=False).eval()
    ref = torch.nn.BatchNorm2d(C, track_running_stats=False).double().eval()
    with torch.no_grad():
        ref.weight.copy_(gamma)
        ref.bias.copy_(beta)
        y_ref = ref(z.double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(-1, C)
    y, saved = _engine_bn_fwd(engine, z, bn, False)
    assert saved is not None and bn.running_mean is None and bn.num_batches_tracked is None
    z64 = z.double().view(-1, C)
    mean, var = z64.mean(0), z64.var(0, unbiased=False)
    sv = saved.double().cpu()
    rtol = 1e-3 if engine == "bf16" else 1e-5
    rel_per_channel(sv[:C], mean, 1e-5, f"{engine} batch mean in eval", floor=torch.full((C,), 1e-6))
    rel_per_channel(sv[C:], (var + bn.eps).rsqrt(), rtol, f"{engine} batch invstd in eval")
    check_bn_apply(y, z64, sv[:C], sv[C:], gamma.double(), beta.double(), False,
                   torch.bfloat16 if engine == "bf16" else torch.float32, f"{engine}eval: y")
    # and against torch itself, with the statistics tolerance carried through (z - mean) invstd gamma
    sc = gamma.double() * (var + bn.eps).rsqrt()
    tol = (rtol + 1e-5) * ((z64 - mean) * sc).abs() + 1e-5 * (mean * sc).abs() + 1e-6 * sc.abs() + \
        (ulp_bf16(y_ref) if engine == "bf16" else 8 * U * ((z64 * sc).abs() + (mean * sc).abs() + beta.double().abs()))
    within(y, y_ref, tol, f"{engine} eval y vs torch")
