"""The optimizer options of csrc/adam.hip on the GPU: the deterministic gradient norm, the Adam step with the clip
coefficient and the EMA fused in, their launchers' argument checks, and the strategies that use them (singleGPU eager
and graphed, DP, DDP over gloo on one device)."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from distributedpytorch_amd.optim import adam_reference, clip_coef_reference

from test_optim_ext_cpu import C, D, G_KW, G_LR, LR, N, WD, _decay, _golden, _inputs  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1            # hipErrorInvalidValue
UNET_PARAMS = 7_760_097
_CACHE = {}


@pytest.fixture(scope="module")
def ops(hip_lib):
    from distributedpytorch_amd import ops
    return ops


def _sizes(ops):
    big = 1 << 22                                   # past the grid cap: the block count no longer grows with n
    nb = ops.grad_sumsq_blocks(big)
    assert nb == ops.grad_sumsq_blocks(big * 2)
    return [1, 3, 4, 5, 1023, 1025, 4 * 256 * nb + 5, 2 * 4 * 256 * nb + 5, UNET_PARAMS]


def _aux(ops):
    return torch.zeros(ops.AUX_LEN, dtype=torch.float64, device="cuda")


def test_grad_sumsq_blocks_depend_on_n_only(ops):
    assert [ops.grad_sumsq_blocks(n) for n in (0, 1, 1024, 1025, 4 * 256 * 1024, 1 << 30)] == [1, 1, 1, 2, 1024, 1024]


def test_grad_sumsq_is_exact_on_integer_data(ops):
    """Integers in [-8, 8]: every square and every partial sum is an integer below 2^53, so fp64 never rounds."""
    aux = _aux(ops)
    for n in _sizes(ops):
        x = torch.randint(-8, 9, (n,), generator=torch.Generator().manual_seed(n))
        ops.grad_sumsq(x.float().cuda(), aux, 1.0)
        got = aux.cpu()
        want = int((x * x).sum())
        assert float(got[0]) == float(want) and int(got[0]) == want, (n, float(got[0]), want)
        assert float(got[1]) == pytest.approx(float(np.sqrt(np.float64(want))), rel=2.0 ** -52)


def test_grad_sumsq_accuracy_determinism_and_coef(ops):
    """randn data against numpy fp64 within n 2^-53 relative (the worst case of an n-term fp64 sum); two calls
    bitwise equal; coef = min(1, C / (norm + 1e-6)) in fp64 to 1e-15 relative; C = inf gives exactly 1."""
    for n in _sizes(ops):
        x = torch.randn(n, generator=torch.Generator().manual_seed(n))
        want = float(np.sum(np.square(x.numpy().astype(np.float64))))
        g = x.cuda()
        a1, a2, a3 = _aux(ops), _aux(ops), _aux(ops)
        cmax = 0.37 * np.sqrt(want)
        ops.grad_sumsq(g, a1, cmax)
        ops.grad_sumsq(g, a2, cmax, slab=torch.full((ops.grad_sumsq_blocks(n) + 3,), 7.0, dtype=torch.float64,
                                                    device="cuda"))
        ops.grad_sumsq(g, a3, float("inf"))
        a1, a2, a3 = a1.cpu(), a2.cpu(), a3.cpu()
        rel = abs(float(a1[0]) - want) / want
        print(f"grad_sumsq n={n}: rel err {rel:.3e} (bound {n * 2.0 ** -53:.3e})")
        assert rel <= n * 2.0 ** -53, (n, rel)
        assert torch.equal(a1, a2), n
        norm = float(a1[1])
        assert norm == pytest.approx(float(np.sqrt(np.float64(float(a1[0])))), rel=2.0 ** -52)
        c = min(1.0, cmax / (norm + 1e-6))
        assert abs(float(a1[2]) - c) <= 1e-15 * c and float(a1[2]) < 1.0
        assert float(a3[2]) == 1.0 and float(a3[0]) == float(a1[0])
        assert float(a1[2]) == pytest.approx(clip_coef_reference(x, cmax)[2], rel=1e-12)


def test_grad_sumsq_nonfinite_gives_nan_coef(ops):
    for bad in (float("inf"), float("nan")):
        g = torch.ones(1025, device="cuda")
        g[700] = bad
        aux = _aux(ops)
        ops.grad_sumsq(g, aux, 1.0)
        assert torch.isnan(aux[2]).item() and not torch.isfinite(aux[0]).item()


def _reference():
    """Four steps of the definition on the CPU inputs of test_optim_ext_cpu (computed once)."""
    if "ref" not in _CACHE:
        p0, gs = _inputs()
        p, m, v, e = p0.clone(), torch.zeros(N), torch.zeros(N), p0.clone()
        for t, g in enumerate(gs, 1):
            coef = clip_coef_reference(g, C)[2]
            adam_reference(p, g, m, v, LR, 0.9, 0.999, 1e-8, WD, 1 - 0.9 ** t, 1 - 0.999 ** t, coef=coef, ema=e,
                           ema_decay=_decay(t))
        _CACHE["ref"] = (p0, gs, p, m, v, e)
    return _CACHE["ref"]


def test_adam_x_host_and_device_state_match_the_reference(ops):
    p0, gs, rp, rm, rv, re_ = _reference()
    kw = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=WD)
    runs = []
    for dev_state in (False, True):
        p, e = p0.cuda(), p0.cuda()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        aux = _aux(ops)
        slab = torch.zeros(ops.grad_sumsq_blocks(N), dtype=torch.float64, device="cuda")
        state = torch.tensor([0.0, LR, 0.0, 0.0], dtype=torch.float64, device="cuda")
        for t, g in enumerate(gs, 1):
            g = g.cuda()
            g0 = g.clone()
            ops.grad_sumsq(g, aux, C, slab)
            if dev_state:
                ops.adam_step_dev(p, g, m, v, state, aux=aux, ema=e, clip=True, ema_decay=D, **kw)
            else:
                ops.adam_step(p, g, m, v, lr=LR, bc1=1 - 0.9 ** t, bc2=1 - 0.999 ** t, ema=e, aux=aux,
                              ema_decay=_decay(t), **kw)
            assert torch.equal(g, g0)                   # the gradient is scaled on the fly, not in place
        torch.cuda.synchronize()
        if dev_state:
            assert float(state[0]) == 4.0 and float(aux[3]) == 1.0 - _decay(4)
        for name, got, want in (("p", p, rp), ("m", m, rm), ("v", v, rv), ("ema", e, re_)):
            torch.testing.assert_close(got.cpu(), want, rtol=1e-5, atol=1e-6, msg=lambda s, n=name: f"{n}: {s}")
        runs.append((p, m, v, e))
    for a, b in zip(*runs):
        torch.testing.assert_close(b, a, rtol=1e-6, atol=1e-7)


MODES = ((False, False), (True, False), (False, True), (True, True))       # (coef == 1 from aux, EMA on)


def _unit_coef_steps(ops, p0, g, m0, v0, steps, dev_state, coef, ema):
    """``p, m, v`` after ``steps`` steps of the golden fixture's hyper-parameters on the same gradient, with the
    options that must not change them: the clip coefficient read from aux where it is exactly 1, the EMA."""
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    e = p0.clone() if ema else None
    aux = _aux(ops) if coef or ema else None
    if coef:
        ops.grad_sumsq(g, aux, float("inf"))
        assert float(aux[2]) == 1.0
    state = torch.tensor([0.0, G_LR, 0.0, 0.0], dtype=torch.float64, device="cuda")
    for k in range(1, steps + 1):
        if dev_state:
            ops.adam_step_dev(p, g, m, v, state, aux=aux, ema=e, clip=coef, ema_decay=D, **G_KW)
        else:
            ops.adam_step(p, g, m, v, lr=G_LR, bc1=1 - 0.9 ** k, bc2=1 - 0.999 ** k, aux=aux if coef else None,
                          ema=e, ema_decay=_decay(k), **G_KW)
    torch.cuda.synchronize()
    if dev_state:
        assert float(state[0]) == steps
    if ema:
        assert not torch.equal(e, p0)
    return p, m, v


def test_adam_x_with_unit_coef_is_bitwise_the_plain_kernel(ops):
    """The plain kernel is the one recorded in tests/golden/adam_plain_bits.npz (tools/record_adam_bits.py, from the
    tree that still had a separate plain kernel): with no options, with coef == 1 read from aux, with the EMA and
    with both, the host-state and the device-state form give those bits after three steps.  Then the modes against
    each other on a million elements (more than one block per CU, a tail of 3)."""
    z = _golden()
    inputs = [torch.from_numpy(z[k]).cuda() for k in ("p0", "g", "m0", "v0")]
    for dev_state in (False, True):
        form = "dev" if dev_state else "host"
        for coef, ema in MODES:
            got = _unit_coef_steps(ops, *inputs, 3, dev_state, coef, ema)
            for name, t in zip("pmv", got):
                assert torch.equal(t.cpu(), torch.from_numpy(z[f"{form}_{name}"])), (form, coef, ema, name)
    torch.manual_seed(0)
    p0, g = torch.randn(N, device="cuda"), torch.randn(N, device="cuda")
    m0, v0 = torch.randn(N, device="cuda").abs() * 0.1, torch.randn(N, device="cuda").abs() * 0.1
    for dev_state in (False, True):
        outs = [_unit_coef_steps(ops, p0, g, m0, v0, 2, dev_state, coef, ema) for coef, ema in MODES]
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert torch.equal(a, b)


def test_adam_x_zero_lr_keeps_p_and_halves_the_distance_to_ema(ops):
    gen = torch.Generator().manual_seed(1)
    n = 100_003
    p0 = torch.randint(-50, 51, (n,), generator=gen).float().cuda()
    e0 = torch.randint(-50, 51, (n,), generator=gen).float().cuda()
    g = torch.randn(n, generator=gen).cuda()
    p, e, m, v = p0.clone(), e0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    ops.adam_step(p, g, m, v, lr=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-8, bc1=0.1, bc2=0.001,
                  ema=e, ema_decay=0.5)
    assert torch.equal(p, p0)
    assert torch.equal(e, (p0 + e0) / 2)
    assert float(m.abs().max()) > 0


def test_launchers_refuse_bad_arguments(ops, hip_lib):
    n = 4096
    buf = torch.zeros(n + 4, device="cuda")
    p, g, m, v, e = (torch.zeros(n, device="cuda") for _ in range(5))
    aux = _aux(ops)
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, bc1=0.1, bc2=0.001)
    off = buf[1:n + 1]                                   # a one-float offset view: 4-byte aligned only
    assert off.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="invalid"):
        ops.grad_sumsq(off, aux, 1.0)
    for bad in (dict(p=off), dict(g=off), dict(ema=off)):
        a = dict(p=p, g=g, ema=e)
        a.update(bad)
        with pytest.raises(RuntimeError, match="invalid"):
            ops.adam_step(a["p"], a["g"], m, v, ema=a["ema"], ema_decay=0.5, **kw)
        state = torch.tensor([0.0, 1e-3, 0.0, 0.0], dtype=torch.float64, device="cuda")
        with pytest.raises(RuntimeError, match="invalid"):
            ops.adam_step_dev(a["p"], a["g"], m, v, state, aux=aux, ema=a["ema"], ema_decay=0.5, beta1=0.9,
                              beta2=0.999, eps=1e-8, weight_decay=0.0)
        assert float(state[0]) == 0.0                    # refused before the tick
    assert ops.grad_sumsq_blocks(n) == 4
    with pytest.raises(RuntimeError, match="invalid"):
        ops.grad_sumsq(g, aux, 1.0, slab=torch.zeros(3, dtype=torch.float64, device="cuda"))
    # raw launchers: n < 0, null pointers; n == 0 is a no-op
    L, vp, ll = hip_lib, ctypes.c_void_p, ctypes.c_longlong
    slab = torch.zeros(4, dtype=torch.float64, device="cuda")
    one = ctypes.c_double(1.0)
    f = ctypes.c_float
    aux.fill_(5.0)

    def sumsq(gp, nn, sp, ap):
        return L.dpa_grad_sumsq(vp(gp), ll(nn), vp(sp), ll(4), vp(ap), one, vp(0))

    def adam(pp, nn, auxp, clip):
        return L.dpa_adam_flat(vp(pp), vp(g.data_ptr()), vp(m.data_ptr()), vp(v.data_ptr()), vp(None), ll(nn),
                               f(1e-3), f(0.9), f(0.999), f(1e-8), f(0.0), f(0.1), f(0.001), ctypes.c_double(0.0),
                               vp(auxp), ctypes.c_int(clip), vp(0))

    assert sumsq(g.data_ptr(), -1, slab.data_ptr(), aux.data_ptr()) == INVALID
    assert sumsq(None, n, slab.data_ptr(), aux.data_ptr()) == INVALID
    assert sumsq(g.data_ptr(), n, None, aux.data_ptr()) == INVALID
    assert sumsq(g.data_ptr(), n, slab.data_ptr(), None) == INVALID
    assert sumsq(g.data_ptr(), 0, slab.data_ptr(), aux.data_ptr()) == 0
    assert adam(p.data_ptr(), -1, None, 0) == INVALID
    assert adam(None, n, None, 0) == INVALID
    assert adam(p.data_ptr(), n, None, 1) == INVALID     # clipping needs the aux block
    assert adam(p.data_ptr(), 0, None, 0) == 0
    assert adam(off.data_ptr(), n, None, 0) == INVALID   # the default step (no EMA, no aux, no clip) is checked too
    state = torch.tensor([0.0, 1e-3, 0.0, 0.0], dtype=torch.float64, device="cuda")

    def adam_dev(pp, nn, auxp, clip):
        return L.dpa_adam_flat_dev(vp(pp), vp(g.data_ptr()), vp(m.data_ptr()), vp(v.data_ptr()), vp(None), ll(nn),
                                   vp(state.data_ptr()), vp(auxp), ctypes.c_double(0.9), ctypes.c_double(0.999),
                                   f(1e-8), f(0.0), ctypes.c_double(0.0), ctypes.c_int(clip), vp(0))

    assert adam_dev(p.data_ptr(), -1, None, 0) == INVALID
    assert adam_dev(None, n, None, 0) == INVALID
    assert adam_dev(off.data_ptr(), n, None, 0) == INVALID
    assert adam_dev(p.data_ptr(), 0, None, 0) == 0
    assert adam_dev(p.data_ptr(), n, None, 1) == INVALID             # clipping needs the aux block
    torch.cuda.synchronize()
    assert float(state[0]) == 0.0                                    # refused (or n == 0) before the tick
    assert adam_dev(p.data_ptr(), n, None, 0) == 0                   # no clip, no EMA: no aux block needed
    torch.cuda.synchronize()
    assert float(state[0]) == 1.0
    assert torch.equal(aux.cpu(), torch.full((ops.AUX_LEN,), 5.0, dtype=torch.float64))    # nothing was launched
    assert float(p.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- strategies
def _batch(n=4, hw=64, seed=11):
    from distributedpytorch_amd.data.synthetic import synthetic_batch
    img, mask = synthetic_batch(n, hw, hw, 3, seed=seed)
    return img.cuda(), mask.float().unsqueeze(1).cuda()


def _pair(seed):
    from distributedpytorch_amd.models.unet import build_model
    torch.manual_seed(seed)
    a, b = build_model("unet"), build_model("unet")
    b.load_state_dict(a.state_dict())
    return a, b


def test_single_device_clip_matches_a_host_scaled_twin(hip_lib):
    """Three steps with C below the observed norm against a plain optimizer whose gradient the host scales by the
    fp64 coef before the step."""
    from distributedpytorch_amd.config import TrainConfig
    from distributedpytorch_amd.trainer import SingleDevice, _backward
    a, b = _pair(6)
    batches = [_batch(4, 64, seed=20 + k) for k in range(3)]
    twin = SingleDevice(TrainConfig(backend="hip", lr=1e-3), b, "cuda:0")

    def twin_backward(x, t):
        twin.optimizer.zero_grad()
        _backward(twin.forward_loss(x, t), float(x.shape[0]))        # as train_step seeds it
        return float(twin.space.grad.double().norm())

    norm0 = twin_backward(*batches[0])
    cmax = 0.05 * norm0
    st = SingleDevice(TrainConfig(backend="hip", lr=1e-3, clip_grad_norm=cmax), a, "cuda:0")
    for k, (x, t) in enumerate(batches):
        norm = norm0 if k == 0 else twin_backward(x, t)
        coef = min(1.0, cmax / (norm + 1e-6))
        twin.space.grad.mul_(torch.tensor(coef, dtype=torch.float64).float().item())
        twin.optimizer.step()
        st.train_step(x, t)
        got_norm, got_coef = st.optimizer.grad_norm()
        print(f"step {k}: norm {got_norm:.6g} (twin {norm:.6g}) coef {got_coef:.6g}")
        assert np.isfinite(got_norm) and got_coef < 1.0
        rel = 1e-12 if k == 0 else 1e-3        # same parameters and batch at step 0: the same gradient
        assert got_norm == pytest.approx(norm, rel=rel) and got_coef == pytest.approx(coef, rel=rel)
    torch.testing.assert_close(st.space.data, twin.space.data, rtol=1e-5, atol=1e-6)


def test_graphed_step_with_clip_and_ema_matches_eager(hip_lib):
    """--cuda-graph with both options: the captured step (norm, extended Adam) replayed gives the eager trajectory
    of parameters and EMA, including an LR change between replays and an eager fallback batch."""
    from distributedpytorch_amd.config import TrainConfig
    from distributedpytorch_amd.trainer import GraphedStep, SingleDevice
    a, b = _pair(4)
    batches = [_batch(4, 64) for _ in range(3)]
    cfg = dict(backend="hip", lr=1e-3, clip_grad_norm=1.0, ema_decay=0.3)
    ea = SingleDevice(TrainConfig(**cfg), a, "cuda:0")
    gb = SingleDevice(TrainConfig(**cfg), b, "cuda:0")
    ea.optimizer.enable_device_state()
    g = GraphedStep(gb, *batches[0])
    assert torch.equal(gb.optimizer.ema[0], ea.optimizer.ema[0])       # the warm-up step was rolled back
    assert torch.equal(gb.space.data, ea.space.data)
    la, lb = [], []
    for k in range(5):
        if k == 3:
            ea.optimizer.param_groups[0]["lr"] = gb.optimizer.param_groups[0]["lr"] = 3e-4
        x, t = batches[k % 3]
        la.append(ea.train_step(x, t))
        lb.append(g(x, t))
    xs, ts = _batch(2, 64)        # other shape -> eager step on the graphed strategy
    la.append(ea.train_step(xs, ts))
    assert not g.matches(xs, ts)
    lb.append(gb.train_step(xs, ts))
    torch.cuda.synchronize()
    assert gb.optimizer.step_count == ea.optimizer.step_count == 6
    for u, v in zip(la, lb):
        assert abs(u.item() - v.item()) <= 1e-5 * abs(u.item()), (la, lb)
    torch.testing.assert_close(gb.space.data, ea.space.data, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gb.optimizer.ema[0], ea.optimizer.ema[0], rtol=1e-5, atol=1e-6)
    assert not torch.equal(gb.optimizer.ema[0], gb.space.data)
    na, nb = ea.optimizer.grad_norm(), gb.optimizer.grad_norm()
    assert nb[0] == pytest.approx(na[0], rel=1e-3) and nb[1] <= 1.0


def test_dp_replicas_stay_bitwise_equal_with_clip_and_ema(hip_lib):
    from distributedpytorch_amd.config import TrainConfig
    from distributedpytorch_amd.trainer import DPStrategy
    a, _ = _pair(1)
    st = DPStrategy(TrainConfig(backend="hip", lr=1e-3, bucket_mb=1.0, clip_grad_norm=1.0, ema_decay=0.3), a,
                    ["cuda:0", "cuda:0"])
    for k in range(3):
        st.train_step(*_batch(4, 64, seed=30 + k))
    torch.cuda.synchronize()
    opt = st.optimizer
    assert torch.equal(st.dp.spaces[0].data, st.dp.spaces[1].data)
    assert torch.equal(opt.ema[0], opt.ema[1]) and not torch.equal(opt.ema[0], st.dp.spaces[0].data)
    assert torch.equal(opt._aux[0][:3], opt._aux[1][:3]) and np.isfinite(opt.grad_norm()[0])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_worker(rank, world, port, q):
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), DPA_SAME_DEVICE="1")
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from distributedpytorch_amd.config import TrainConfig
        from distributedpytorch_amd.models.unet import build_model
        from distributedpytorch_amd.trainer import DDPStrategy
        torch.manual_seed(0)
        cfg = TrainConfig(train_method="DDP", backend="hip", lr=1e-3, bucket_mb=1.0, clip_grad_norm=1.0,
                          ema_decay=0.3)
        st = DDPStrategy(cfg, build_model("unet"), torch.device("cuda:0"))
        for i in range(3):
            st.train_step(*_batch(4, 64, seed=200 + 10 * i + rank))
        torch.cuda.synchronize()
        norm, coef = st.optimizer.grad_norm()
        mine = [st.space.data.detach().cpu(), st.optimizer.ema[0].detach().cpu(),
                torch.tensor([norm, coef], dtype=torch.float64)]
        same = []
        for t in mine:
            out = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(out, t)
            same.append(all(torch.equal(out[0], o) for o in out[1:]))
        q.put((rank, same, norm, coef, bool(torch.equal(mine[0], mine[1])), None))
    except Exception as e:
        import traceback
        q.put((rank, [], 0.0, 0.0, True, repr(e) + traceback.format_exc()[-2000:]))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_ddp_ranks_stay_bitwise_equal_with_clip_and_ema(hip_lib):
    """Two ranks on cuda:0 over gloo: the norm is taken on the averaged gradient every rank holds, so parameters,
    EMA and the reported norm are the same bits on both."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=240) for _ in procs)
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    errs = [(r[0], r[-1]) for r in res if r[-1] is not None]
    assert not errs, errs
    for rank, same, norm, coef, ema_is_p, _ in res:
        assert same == [True, True, True], f"rank {rank}: parameters / ema / grad_norm differ across ranks: {same}"
        assert np.isfinite(norm) and 0.0 < coef <= 1.0 and not ema_is_p
