"""The segmentation head with its BCE / Dice partial sums in both engines (csrc/unet_aux.hip, csrc/fp32.hip) and
the slab plumbing (slab_fold, slab_sum, chan_sum_bf16) at their edges.  Same rules as test_reduction_edges.py:
float64 references on the CPU from the tensor the kernel read, every quantity on its own scale, exact integer
inputs wherever the point is that no element is dropped, duplicated or mis-indexed."""
import pytest
import torch
import torch.nn.functional as F

from test_reduction_edges import U, ints, rel_per_channel, ulp_bf16, within

pytestmark = pytest.mark.gpu

# tolerances of the existing head tests (test_hip_kernels.py / test_fp32_engine.py), applied per quantity
TOL = {"bf16": dict(S=1e-4, grad=1e-3), "fp32": dict(S=1e-5, grad=1e-4)}
DS = torch.tensor([0.5, -1.25, 0.75, 0.0])      # dyadic dL/dS: products with +-1 weights stay exact


def ulp_distance(a, b):
    """Distance in fp32 ulps between two float32 tensors of equal sign."""
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


def run_head(engine, y, w, b, t, dS, relu=True, **kw):
    """Forward and backward of one engine's head binding on [N, H, W, C] ``y`` (CPU float; bf16-exact for the bf16
    engine).  Everything comes back on the CPU: S [4], probs [P], gy [P, C], gw [C], gb [1]."""
    N, H, W, C = y.shape
    P = N * H * W
    if engine == "bf16":
        from distributedpytorch_amd.ops import kernels as K
        yd = y.to(torch.bfloat16).cuda()
        assert torch.equal(yd.float().cpu(), y), "the input is not bf16-exact"
        wd, bd, td = w.cuda(), b.cuda(), t.reshape(-1).float().cuda().contiguous()
        S, probs = K.head_fwd(yd, wd, bd, td, want_probs=True)
        gw, gb = torch.zeros(C, device="cuda"), torch.zeros(1, device="cuda")
        gy = K.head_bwd(yd, wd, bd, td, dS.cuda(), gw, gb, **kw)
    else:
        from distributedpytorch_amd.ops import fp32 as F32
        yd = y.cuda()
        wd, bd, td = w.cuda(), b.cuda(), t.reshape(-1).float().cuda()
        S, probs = F32.head_fwd(yd, wd, bd, td, want_probs=True)
        gy, gw, gb = F32.head_bwd(yd, wd, bd, td, dS.cuda(), relu=relu)
    torch.cuda.synchronize()
    return dict(S=S.double().cpu(), probs=probs.reshape(-1).cpu(), gy=None if gy is None else gy.reshape(P, C).cpu(),
                gw=gw.reshape(-1).cpu(), gb=gb.reshape(-1).cpu(), dev=dict(y=yd, w=wd, b=bd, t=td))


def head_ref64(y, w, b, t, dS, relu=True):
    """float64 head composed with the ReLU that produced y, its partial sums S and the gradients of dS . S."""
    x = y.double().reshape(-1, y.shape[-1]).clone().requires_grad_(True)
    w64, b64 = w.double().reshape(-1).clone().requires_grad_(True), b.double().reshape(-1).clone().requires_grad_(True)
    t64 = t.double().reshape(-1)
    z = (torch.relu(x) if relu else x) @ w64 + b64
    p = torch.sigmoid(z)
    one = (t64 == 1).double()
    bce = -(t64 * torch.log(p).clamp_min(-100) + (1 - t64) * torch.log1p(-p).clamp_min(-100))
    S = torch.stack([bce.sum(), (p * one).sum(), p.sum(), one.sum()])
    gx, gw, gb = torch.autograd.grad((S * dS.double()).sum(), (x, w64, b64))
    return dict(S=S.detach(), p=p.detach(), gy=gx, gw=gw, gb=gb, one=one, x=x.detach(), t=t64)


def check_head(engine, out, ref, w, b, dS, what):
    """S per quantity, probabilities per element (rtol 1e-5, the existing tests' number), gradients per element /
    channel at the engine's tolerance on top of what fp32 arithmetic can resolve where terms cancel: per pixel
    dz = d0 (p - t) rs + (d1 [t == 1] + d2) s carries <= 8 fp32 ulp of |d0| (p + t) + |d1 [t == 1] + d2| s (the
    probability itself is specified to 8 ulp) and the error of the logit, C fp32 roundings of |b| + sum |y w|,
    through |d dz / dz| <= (|d0| + |d1| + |d2|) s."""
    tol = TOL[engine]
    C = w.numel()
    w64, d = w.double().reshape(-1), dS.double()
    p, t, one, x = ref["p"], ref["t"], ref["one"], ref["x"]
    rel_per_channel(out["S"][:3], ref["S"][:3], tol["S"], what + ": S")
    assert out["S"][3].item() == ref["S"][3].item(), what + ": S3 (a count)"
    within(out["probs"], p, 1e-5 * p, what + ": probs")
    s = p * (1 - p)
    dlogit = C * U * (b.double().abs() + (x.abs() * w64.abs()).sum(1))
    A = 8 * U * (d[0].abs() * (p + t) + (d[1] * one + d[2]).abs() * s) + d[:3].abs().sum() * s * dlogit
    tol_gy = tol["grad"] * ref["gy"].abs() + A[:, None] * w64.abs()[None, :]
    if engine == "bf16":
        tol_gy = tol_gy + 0.5 * ulp_bf16(ref["gy"])
    if out["gy"] is not None:
        within(out["gy"], ref["gy"], tol_gy, what + ": gy")
    dzp = (d[0] * (p - t) * torch.where(s >= 1e-12, torch.ones_like(s), s * 1e12) + (d[1] * one + d[2]) * s).abs()
    per_pixel = A + 8 * U * dzp                # plus the fp32 summation of the per-pixel terms
    rel_per_channel(out["gw"], ref["gw"], tol["grad"], what + ": gw", floor=(per_pixel[:, None] * x.abs()).sum(0))
    rel_per_channel(out["gb"], ref["gb"], tol["grad"], what + ": gb", floor=per_pixel.sum().reshape(1))


# ------------------------------------------------------------------------------------------ D. widths
@pytest.mark.parametrize("C", [8, 16, 32, 64])
@pytest.mark.parametrize("engine", ["bf16", "fp32"])
def test_head_widths(hip_lib, engine, C):
    """Every template width at a ragged P = 2640; bf16 C = 32 / 64 also the BatchNorm forms: ``bn_stats`` partials
    against float64 sums of the returned gy, ``store=False`` and the on-load ``coef`` form bit for bit."""
    N, H, W = 2, 33, 40
    P = N * H * W
    gen = torch.Generator().manual_seed(100 + C)
    y = torch.relu(torch.randn(N, H, W, C, generator=gen))
    if engine == "bf16":
        y = y.to(torch.bfloat16).float()
    w = torch.randn(C, generator=gen) * 0.2
    b = torch.randn(1, generator=gen) * 0.1
    t = (torch.rand(P, generator=gen) > 0.6).float()
    out = run_head(engine, y, w, b, t, DS)
    check_head(engine, out, head_ref64(y, w, b, t, DS), w, b, DS, f"{engine} C={C}")
    if engine == "fp32":
        if C == 32:           # without the ReLU fold: y with negative entries, gy unmasked
            y2 = torch.randn(N, H, W, C, generator=gen)
            out = run_head(engine, y2, w, b, t, DS, relu=False)
            check_head(engine, out, head_ref64(y2, w, b, t, DS, relu=False), w, b, DS, "fp32 C=32 relu=False")
        return
    if C not in (32, 64):
        return
    from distributedpytorch_amd.ops import kernels as K
    dev = out["dev"]

    def bwd(yd, **kw):
        gw, gb = torch.zeros(C, device="cuda"), torch.zeros(1, device="cuda")
        stats = []
        gy = K.head_bwd(yd, dev["w"], dev["b"], dev["t"], DS.cuda(), gw, gb, bn_stats=stats, **kw)
        torch.cuda.synchronize()
        assert len(stats) == 2
        return gy, gw, gb, stats[0][:stats[1] * 2 * C].clone(), stats[1]

    gy, gw, gb, slab, rows = bwd(dev["y"])
    assert torch.equal(gy.reshape(P, C).cpu(), out["gy"]) and torch.equal(gw.cpu(), out["gw"]) and torch.equal(gb.cpu(), out["gb"])
    sums = slab.view(rows, 2, C).double().sum(0).cpu()
    g64, y64 = out["gy"].double(), y.double().reshape(P, C)
    rel_per_channel(sums[0], g64.sum(0), 1e-4, "bn partials: sum gy", floor=U * g64.abs().sum(0))
    rel_per_channel(sums[1], (g64 * y64).sum(0), 1e-4, "bn partials: sum gy y", floor=U * (g64 * y64).abs().sum(0))
    none, gw2, gb2, slab2, rows2 = bwd(dev["y"], store=False)
    assert none is None and rows2 == rows
    assert torch.equal(slab2, slab) and torch.equal(gw2, gw) and torch.equal(gb2, gb)
    # y = relu(bn(z)) formed on load with bn_apply's arithmetic == the head over the y that bn_fwd stored
    z = (torch.randn(N, H, W, C, generator=gen) * 1.3 + 0.2).to(torch.bfloat16).cuda()
    bn = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(-1.0, 1.5, C))
        bn.bias.copy_(torch.linspace(-0.5, 0.5, C))
    yz = torch.empty_like(z)
    coef = []
    K.bn_fwd(z, yz, bn, train=True, coef_out=coef)
    Sy, py = K.head_fwd(yz, dev["w"], dev["b"], dev["t"], want_probs=True)
    Sz, pz = K.head_fwd(z, dev["w"], dev["b"], dev["t"], want_probs=True, coef=coef[0])
    torch.cuda.synchronize()
    assert torch.equal(Sy, Sz) and torch.equal(py, pz)
    for a, c in zip(bwd(yz), bwd(z, coef=coef[0])):
        assert a == c if isinstance(a, int) else torch.equal(a, c)


# ------------------------------------------------------------------------------------------ D. stride loops
@pytest.mark.parametrize("engine,shape", [("bf16", (1, 513, 1025, 8)),        # P = 525825 > 2048 * 256
                                          ("fp32", (1, 1, 1024 * 128 + 37, 8))])   # 1024 blocks x 256 / (C / 4) pixels
def test_head_stride_loop(hip_lib, engine, shape):
    """Past the grid cap.  Channels 0 and 1 hold the same integer with weights +0.5 / -0.5 and every other weight
    is 0, so the logit is b and p = sigmoid(b) at every pixel; t and y depend on the index.  S3 (a count) is exact,
    S2 = P p and S1 = (sum t) p with the kernel's own p to rtol 1e-6, and every row of gy repeats the row of its
    class (t, y > 0) bit for bit."""
    N, H, W, C = shape
    P = N * H * W
    idx = torch.arange(P)
    y = ints(P, C) + 4                                  # a ReLU output: 0 .. 8
    y[:, 0] = y[:, 1] = (idx * 7 % 5).float()
    t = (idx * 7 % 3 == 0).float()
    w = torch.zeros(C)
    w[0], w[1] = 0.5, -0.5
    b = torch.tensor([0.375])
    out = run_head(engine, y.view(N, H, W, C), w, b, t, DS)
    ref = head_ref64(y, w, b, t, DS)
    n1 = int(t.sum())
    p0 = out["probs"][0]
    assert torch.equal(out["probs"], p0.expand(P)), "p differs between pixels"
    assert ulp_distance(p0.reshape(1), torch.sigmoid(b.double()).float()).item() <= 8
    S = out["S"]
    assert S[3].item() == n1
    assert abs(S[2].item() / (P * p0.double().item()) - 1) < 1e-6 and abs(S[1].item() / (n1 * p0.double().item()) - 1) < 1e-6
    rel_per_channel(S[:1], ref["S"][:1], TOL[engine]["S"], "S0")
    gy = out["gy"]
    assert gy[:, 2:].abs().max().item() == 0
    pos = y[:, 0] > 0
    i1, i0 = int(torch.nonzero(pos & (t == 1))[0]), int(torch.nonzero(pos & (t == 0))[0])
    want = torch.where(t == 1, gy[i1, 0], gy[i0, 0]) * pos
    assert torch.equal(gy[:, 0], want) and torch.equal(gy[:, 1], -want), "a row of gy differs from its class"
    check_head(engine, out, ref, w, b, DS, f"{engine} stride loop")


# ------------------------------------------------------------------------------------------ D. BCELoss semantics
def logit_rows(z, C=8):
    """[P, C] rows whose logit is exactly z under w = (+1, -1, 0, ...), b = 0: y0 = max(z, 0), y1 = max(-z, 0)."""
    y = torch.ones(z.numel(), C)
    y[:, 0], y[:, 1] = z.clamp_min(0), (-z).clamp_min(0)
    w = torch.zeros(C)
    w[0], w[1] = 1.0, -1.0
    return y, w, torch.zeros(1)


@pytest.mark.parametrize("engine", ["bf16", "fp32"])
def test_head_moderate_logits_soft_targets(hip_lib, engine):
    """Logits on a grid in [-6, 6] against hard and soft targets (this pins one = [t == 1] for t = 0.999)."""
    zg = torch.arange(-6.0, 6.25, 0.25)
    tv = torch.tensor([0.0, 1.0, 0.25, 0.5, 0.999])
    z = zg.repeat_interleave(tv.numel())
    t = tv.repeat(zg.numel())
    y, w, b = logit_rows(z)
    out = run_head(engine, y.view(1, 1, -1, 8), w, b, t, DS)
    check_head(engine, out, head_ref64(y, w, b, t, DS), w, b, DS, f"{engine} moderate")


@pytest.mark.parametrize("engine", ["bf16", "fp32"])
def test_head_saturated_logits_follow_bceloss(hip_lib, engine):
    """|z| in {20, 50, 80, 120} with hard targets, against torch's own fp32 sigmoid + BCELoss(reduction='sum') and
    its autograd: the log clamp at -100, (p - t) / max(p (1 - p), 1e-12) and no NaN / Inf anywhere.
    Left out on purpose: 15.5 < |z| < 18.5, where fp32 1 - p is a few ulps and the reference itself jumps between
    -16 and -100; and -103 < z < -88, where torch's probability is denormal while the kernels flush to zero."""
    zv = torch.tensor([20.0, -20.0, 50.0, -50.0, 80.0, -80.0, 120.0, -120.0])
    z = zv.repeat_interleave(2)
    t = torch.tensor([0.0, 1.0]).repeat(zv.numel())
    y, w, b = logit_rows(z)
    out = run_head(engine, y.view(1, 1, -1, 8), w, b, t, DS)
    for k in ("S", "probs", "gy", "gw", "gb"):
        assert torch.isfinite(out[k]).all(), k
    x = y.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    p32 = torch.sigmoid(torch.relu(x) @ wr + br)
    one = (t == 1).float()
    bce = F.binary_cross_entropy(p32, t, reduction="sum")
    L = DS[0] * bce + DS[1] * (p32 * one).sum() + DS[2] * p32.sum()
    gx, gw, gb = torch.autograd.grad(L, (x, wr, br))
    p32 = p32.detach()
    sat = (p32 == 0) | (p32 == 1)
    assert sat.sum().item() == 10                      # z = 20, 50, 80, +-120
    assert torch.equal(out["probs"][sat], p32[sat])
    p64 = torch.sigmoid(z.double()).float()
    d = ulp_distance(out["probs"][~sat], p64[~sat])
    print(f"[saturated {engine}] ulp distance at z = -20, -50, -80: {d.tolist()}")
    assert d.max().item() <= 4
    assert abs(out["S"][0].item() / bce.item() - 1) < 1e-6, (out["S"][0].item(), bce.item())
    torch.testing.assert_close(out["S"][1:3], torch.stack([(p32 * one).double().sum(), p32.double().sum()]), rtol=1e-6, atol=0)
    assert out["S"][3].item() == 8
    torch.testing.assert_close(out["gy"].float(), gx, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(out["gw"], gw, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(out["gb"], gb, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("engine", ["bf16", "fp32"])
def test_head_infinite_logits(hip_lib, engine):
    """z = +-inf and the largest finite logits (forward only: the weight gradient dz y is 0 * inf there): p is exactly
    1 / 0 and the loss terms are the clamp's 100 or 0, as with torch's sigmoid and BCELoss."""
    big = float(torch.finfo(torch.bfloat16).max)          # 3.39e38, bf16-exact: |z| log2(e) overflows
    z = torch.tensor([float("inf"), -float("inf"), big, -big]).repeat_interleave(2)
    t = torch.tensor([0.0, 1.0]).repeat(4)
    y, w, b = logit_rows(z)
    if engine == "bf16":
        from distributedpytorch_amd.ops import kernels as K
        S, probs = K.head_fwd(y.view(1, 1, -1, 8).to(torch.bfloat16).cuda(), w.cuda(), b.cuda(), t.cuda(), want_probs=True)
    else:
        from distributedpytorch_amd.ops import fp32 as F32
        S, probs = F32.head_fwd(y.view(1, 1, -1, 8).cuda(), w.cuda(), b.cuda(), t.cuda(), want_probs=True)
    torch.cuda.synchronize()
    p32 = torch.sigmoid(z)
    assert torch.equal(probs.reshape(-1).cpu(), p32) and torch.equal(p32, (z > 0).float())
    bce = F.binary_cross_entropy(p32, t, reduction="sum")
    assert bce.item() == 400.0
    assert torch.equal(S.cpu(), torch.tensor([400.0, 2.0, 4.0, 4.0]))


# measured on an MI355X over the grid below: 3 ulp in both engines (exp_hw, csrc/common.h); more than 8 is a bug
PROB_ULP = {"bf16": 3, "fp32": 3}


@pytest.mark.parametrize("engine", ["bf16", "fp32"])
def test_head_probability_accuracy(hip_lib, engine):
    """The largest distance in fp32 ulps between an engine's probabilities and the float64 sigmoid rounded to fp32,
    on a dense exact grid z = +-(c - f), c in {0, 0.25, ..., 30}, f in {0, 1, ..., 255} / 1024 (both bf16-exact,
    their difference exact in fp32)."""
    c = torch.arange(0, 30.25, 0.25).repeat_interleave(256)
    f = (torch.arange(256) / 1024.0).repeat(121)
    y = torch.ones(2 * c.numel(), 8)
    y[:, 0], y[:, 1] = torch.cat([c, f]), torch.cat([f, c])
    w = torch.zeros(8)
    w[0], w[1] = 1.0, -1.0
    z64 = y[:, 0].double() - y[:, 1].double()
    out = run_head(engine, y.view(1, 1, -1, 8), w, torch.zeros(1), torch.zeros(y.shape[0]), DS)
    d = ulp_distance(out["probs"], torch.sigmoid(z64).float())
    worst = int(d.argmax())
    print(f"[prob ulp {engine}] max {d.max().item()} at z = {z64[worst].item()}")
    assert d.max().item() <= PROB_ULP[engine] <= 8


# ------------------------------------------------------------------------------------------ E. slab plumbing
@pytest.mark.parametrize("K_", [4, 64, 2048])
@pytest.mark.parametrize("rows", [1, 512, 513, 1025, 70001])
def test_fold_slab(hip_lib, rows, K_):
    """_fold_slab / dpa_slab_fold: block b sums rows b R .. b R + R - 1 with R = ceil(rows / 512); the returned row
    count is ceil(rows / R).  Integer slab, exact against int64; twice, bit for bit."""
    from distributedpytorch_amd.ops import kernels as K
    r = torch.arange(rows, dtype=torch.int32).view(rows, 1)
    k = torch.arange(K_, dtype=torch.int32).view(1, K_)
    v = (7 * r + 3 * k) % 9 - 4
    slab = v.float().cuda().reshape(-1)
    R = -(-rows // 512)
    nout = -(-rows // R)
    full = rows // R * R
    want = v[:full].view(-1, R, K_).sum(1)
    if full < rows:
        want = torch.cat([want, v[full:].sum(0, keepdim=True)])
    outs = []
    for _ in range(2):
        out, n = K._fold_slab(slab, rows, K_)
        torch.cuda.synchronize()
        assert n == nout
        outs.append(out[:n * K_].clone())
    assert torch.equal(outs[0].cpu().double().view(nout, K_), want.double())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("K_", [1, 4, 33])
def test_slab_sum(hip_lib, rows, K_):
    from distributedpytorch_amd.ops import kernels as K
    v = ints(rows, K_)
    outs = [K._slab_sum(v.cuda().reshape(-1), rows, K_) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(outs[0].cpu().double(), v.double().sum(0)) and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("nblk", [1, 7, 512])
@pytest.mark.parametrize("C", [8, 64, 2048])
def test_chan_sum_bf16(hip_lib, C, nblk):
    """dpa_chan_sum_bf16 on a ragged P as a channel slice (ld = 2C), accumulated onto a non-zero ``out``: exact
    integer sums (a lo / hi swap of the bf16 pairs would exchange neighbouring channels), twice, bit for bit."""
    from distributedpytorch_amd.ops import kernels as K
    P = 1237
    v = ints(P, C)
    buf = ints(P, 2 * C, 5, 11, 13).view(1, 1, P, 2 * C).to(torch.bfloat16).cuda()
    buf[..., C:] = v.view(1, 1, P, C).to(torch.bfloat16).cuda()
    start = (torch.arange(C) % 5 - 2).float()
    outs = []
    for _ in range(2):
        out = start.clone().cuda()
        K._chan_sum_bf16(buf[..., C:], out, nblk=nblk)
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0].cpu().double(), v.double().sum(0) + start.double()) and torch.equal(outs[0], outs[1])
