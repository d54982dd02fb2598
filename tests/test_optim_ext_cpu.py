"""Gradient-norm clipping and EMA weights in the fused optimizer step: definitions, optimizer state, trainer (CPU).

The definitions (``optim.clip_coef_reference``, ``optim.adam_reference``) are checked against
``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam`` + a hand-written EMA over several steps with different
gradient norms: from zero moments Adam's first step does not depend on the gradient's scale, so one step could not
tell whether the clip was applied.  The HIP kernels are checked against these definitions in
``test_optim_ext_gpu.py``.
"""
import dataclasses
import json
import logging
import math
import os

import numpy as np
import pytest
import torch

from distributedpytorch_amd.config import parse_args
from distributedpytorch_amd.models.unet import build_model
from distributedpytorch_amd.optim import FlatParameterSpace, FusedAdam, adam_reference, clip_coef_reference

N = 1_000_003
SCALES = (0.5, 4.0, 0.01, 2.0)          # norms of about 500, 4000, 10, 2000: steps 2 and 4 are clipped at C = 1000
C, WD, LR, D = 1000.0, 1e-8, 1e-3, 0.3  # D = 0.3: the schedule (1 + t) / (10 + t) passes it at t = 3

ARGS = ["--synthetic", "--synthetic-len", "16", "-v", "25", "--img-size", "32", "--model", "unet-tiny",
        "--backend", "torch", "--dtype", "fp32", "-b", "4", "--log-every", "1", "--lr", "1e-3"]
EXT = ["--clip-grad-norm", "1e3", "--ema-decay", "0.99"]

# tests/golden/adam_plain_bits.npz (tools/record_adam_bits.py): three steps of the default kernel on one gradient
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_plain_bits.npz")
G_N, G_LR = 1027, 1e-3
G_KW = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)


def _decay(t, d=D):
    return min(d, (1.0 + t) / (10.0 + t))


def _inputs():
    gen = torch.Generator().manual_seed(0)
    p0 = torch.randn(N, generator=gen)
    gs = [torch.randn(N, generator=gen) * s for s in SCALES]
    return p0, gs


def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_golden_adam_bits_are_what_the_reference_computes():
    """A corrupted or mis-recorded fixture would not land on the CPU definition (the tolerances of test_adam.py for
    kernel against reference).

    The launchers take the betas as C floats and the kernel forms 1 - beta in fp32, so the definition is given the
    betas as the kernel sees them: float32(0.999) is 0.99900001, and 1 - 0.99900001 differs from 0.001 by 1.3e-5
    relative, which is v's own error wherever (1 - b2) g^2 dominates it (|g| up to 1e2 here; with 0.999 as a Python
    float v misses rtol 1e-5 at 103 of the 1027 elements, max 1.7e-5).  With the rounded betas the largest relative
    errors are 3.8e-7 (p), 2.3e-6 (m) and 3.6e-7 (v).  The bias corrections stay 1 - 0.9 ** t and 1 - 0.999 ** t of
    the Python floats: the recording formed them so on the host (fp64, from the unrounded betas) and handed them to
    the launcher as numbers, and the device-state tick computes them in fp64 from double betas, so the kernel never
    sees a bias correction made from a float32 beta."""
    z = _golden()
    assert sorted(z) == sorted(["p0", "g", "m0", "v0"] + [f"{f}_{n}" for f in ("host", "dev") for n in "pmv"])
    for k, a in z.items():
        assert a.dtype == np.float32 and a.shape == (G_N,) and np.isfinite(a).all(), k
    assert (z["g"] == 0).sum() >= 3 and (z["v0"] == 0).sum() >= 3 and (z["v0"] >= 0).all()
    mag = np.abs(z["g"][z["g"] != 0])
    assert mag.min() < 1e-3 and mag.max() > 10.0                  # the gradient spans the magnitudes Adam sees
    p, g, m, v = (torch.from_numpy(z[k].copy()) for k in ("p0", "g", "m0", "v0"))
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    for t in (1, 2, 3):
        adam_reference(p, g, m, v, G_LR, b1, b2, 1e-8, G_KW["weight_decay"], 1 - 0.9 ** t, 1 - 0.999 ** t)
    for form in ("host", "dev"):
        for name, want in (("p", p), ("m", m), ("v", v)):
            torch.testing.assert_close(torch.from_numpy(z[f"{form}_{name}"]), want, rtol=1e-5, atol=1e-6,
                                       msg=lambda s, n=f"{form}_{name}": f"{n}: {s}")


def _torch_trajectory(p0, gs, clip):
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=LR, weight_decay=WD)
    ema = p0.clone()
    for t, g in enumerate(gs, 1):
        p.grad = g.clone()
        if clip:
            torch.nn.utils.clip_grad_norm_([p], C)
        opt.step()
        with torch.no_grad():
            ema = ema + (1.0 - _decay(t)) * (p.detach() - ema)
    return p.detach().clone(), ema


def test_references_match_torch_clip_adam_and_ema():
    p0, gs = _inputs()
    want_p, want_e = _torch_trajectory(p0, gs, clip=True)
    p, m, v, e = p0.clone(), torch.zeros(N), torch.zeros(N), p0.clone()
    coefs = []
    for t, g in enumerate(gs, 1):
        g_before = g.clone()
        sumsq, norm, coef = clip_coef_reference(g, C)
        assert norm == math.sqrt(sumsq)
        coefs.append(coef)
        adam_reference(p, g, m, v, LR, 0.9, 0.999, 1e-8, WD, 1 - 0.9 ** t, 1 - 0.999 ** t, coef=coef, ema=e,
                       ema_decay=_decay(t))
        assert torch.equal(g, g_before), "the gradient is scaled on the fly, not in place"
    assert coefs[0] == 1.0 and coefs[2] == 1.0 and coefs[1] < 0.3 and 0.4 < coefs[3] < 0.6, coefs
    torch.testing.assert_close(p, want_p, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(e, want_e, rtol=1e-5, atol=1e-6)
    # the same check tells a missing clip: the unclipped trajectory is three orders of magnitude further away
    raw_p, _ = _torch_trajectory(p0, gs, clip=False)
    assert float((raw_p - want_p).abs().max()) > 1e-4


def test_clip_coef_reference_edges():
    g = torch.tensor([3.0, 4.0])
    assert clip_coef_reference(g, float("inf")) == (25.0, 5.0, 1.0)
    s, n, c = clip_coef_reference(g, 1.0)
    assert c == 1.0 / (5.0 + 1e-6)
    for bad in (float("inf"), float("nan")):
        s, n, c = clip_coef_reference(torch.tensor([1.0, bad]), 1.0)
        assert math.isnan(c)


def _tiny_pair(**kw):
    torch.manual_seed(3)
    a, b = build_model("unet-tiny"), build_model("unet-tiny")
    b.load_state_dict(a.state_dict())
    sa, sb = FlatParameterSpace(a), FlatParameterSpace(b)
    return (a, sa, FusedAdam(sa, lr=1e-3, weight_decay=1e-8)), (b, sb, FusedAdam(sb, lr=1e-3, weight_decay=1e-8, **kw))


def _steps(pairs, n, seed=0, scale=(1.0,)):
    gen = torch.Generator().manual_seed(seed)
    for k in range(n):
        g = torch.randn(pairs[0][1].numel, generator=gen) * scale[k % len(scale)]
        for _, s, o in pairs:
            s.grad.copy_(g)
            o.step()


def test_measure_only_is_bitwise_the_plain_optimizer():
    plain, ext = _tiny_pair(clip_grad_norm=float("inf"))
    _steps([plain, ext], 3)
    assert torch.equal(ext[1].data, plain[1].data)
    assert torch.equal(ext[2].exp_avg_sq[0], plain[2].exp_avg_sq[0])
    norm, coef = ext[2].grad_norm()
    assert coef == 1.0 and norm == pytest.approx(float(ext[1].grad.double().norm()), rel=1e-12)
    assert plain[2].grad_norm() is None


def test_state_dict_keys_unchanged_when_off():
    plain, ext = _tiny_pair(clip_grad_norm=5.0)
    keys = {"step", "exp_avg", "exp_avg_sq", "names", "param_groups"}
    assert set(plain[2].state_dict()) == keys
    assert set(ext[2].state_dict()) == keys                   # clipping alone adds no state
    assert not plain[2].ema and not plain[2]._aux and not plain[2]._slab


def test_clipping_leaves_the_gradient_and_scales_the_step():
    plain, ext = _tiny_pair(clip_grad_norm=0.5)
    g = torch.randn(plain[1].numel, generator=torch.Generator().manual_seed(1))
    for _, s, o in (plain, ext):
        s.grad.copy_(g)
    ext[2].step()
    assert torch.equal(ext[1].grad, g)
    norm, coef = ext[2].grad_norm()
    assert coef == 0.5 / (norm + 1e-6) < 1.0
    plain[1].grad.mul_(torch.tensor(coef, dtype=torch.float64).float())      # the host-scaled twin
    plain[2].step()
    assert torch.equal(ext[1].data, plain[1].data)


def test_state_round_trip_and_the_three_load_cases():
    handler = _Records()
    logging.getLogger("dpa").addHandler(handler)
    try:
        src, ext = _tiny_pair(ema_decay=0.9)
        src = (src[0], src[1], FusedAdam(src[1], lr=1e-3, weight_decay=1e-8, ema_decay=0.9))
        _steps([src], 3, scale=(1.0, 3.0))
        sd = src[2].state_dict()
        assert [tuple(e.shape) for e in sd["ema"]] == [(src[1].numel,)] and not sd["ema"][0].is_cuda
        assert not torch.equal(sd["ema"][0], src[1].data)
        # "ema" present, EMA on: copied in, and the run continues on the same trajectory
        ext[1].data.copy_(src[1].data)
        ext[2].load_state_dict(sd)
        assert torch.equal(ext[2].ema[0], src[2].ema[0]) and not handler.records
        _steps([src, ext], 2, seed=5)
        assert torch.equal(ext[2].ema[0], src[2].ema[0]) and torch.equal(ext[1].data, src[1].data)
        # EMA on, "ema" absent: restarts from the loaded parameters, with a warning
        old = {k: v for k, v in src[2].state_dict().items() if k != "ema"}
        ext[2].load_state_dict(old)
        assert torch.equal(ext[2].ema[0], ext[1].data)
        assert any(r.levelno == logging.WARNING and "EMA" in r.getMessage() for r in handler.records)
        # "ema" present, EMA off: ignored
        plain, _ = _tiny_pair()
        plain[2].load_state_dict(src[2].state_dict())
        assert plain[2].step_count == src[2].step_count and not plain[2].ema
        assert "ema" not in plain[2].state_dict()
    finally:
        logging.getLogger("dpa").removeHandler(handler)


class _Records(logging.Handler):
    def __init__(self):
        super().__init__()
        self.records = []

    def emit(self, record):
        self.records.append(record)


def test_swap_ema_restores_bitwise_and_exports_the_average():
    _, (model, space, opt) = _tiny_pair(ema_decay=0.9)
    _steps([(model, space, opt)], 3)
    before, ema_before, version = space.data.clone(), opt.ema[0].clone(), space.version
    want = opt.ema_state_dict(model)
    assert list(want) == list(model.state_dict())
    with opt.swap_ema():
        assert space.version > version                        # kernels that cache packed weights re-pack
        inside = model.state_dict()
        for k in want:
            assert torch.equal(inside[k], want[k]), k
        assert torch.equal(space.data, ema_before) and torch.equal(opt.ema[0], before)
    assert torch.equal(space.data, before) and torch.equal(opt.ema[0], ema_before)
    assert space.version > version + 1
    for (n, p), o, k in zip(zip(space.names, space.params), space.offsets, space.numels):
        assert p.data_ptr() == space.data[o:o + k].data_ptr(), n   # still views of the flat buffer
    with pytest.raises(RuntimeError):
        with _tiny_pair()[0][2].swap_ema():
            pass


def test_device_state_cpu_matches_host_state_with_clip_and_ema():
    """Device-state mode (the HIP-graph form) gives the host-state trajectory, incl. an LR cut."""
    torch.manual_seed(3)
    a, b = build_model("unet-tiny"), build_model("unet-tiny")
    b.load_state_dict(a.state_dict())
    sa, sb = FlatParameterSpace(a), FlatParameterSpace(b)
    kw = dict(lr=1e-3, weight_decay=1e-8, clip_grad_norm=20.0, ema_decay=0.3)
    oa, ob = FusedAdam(sa, **kw), FusedAdam(sb, **kw)
    ob.enable_device_state()
    for k in range(5):
        if k == 2:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 2e-4
        g = torch.randn(sa.numel) * (0.1, 3.0, 0.5, 2.0, 0.05)[k]
        sa.grad.copy_(g)
        sb.grad.copy_(g)
        oa.step()
        ob.step()
    assert ob.step_count == oa.step_count == 5 and float(ob._dev_state[0][0]) == 5.0
    assert float(ob._aux[0][3]) == 1.0 - 0.3                  # the schedule reached its ceiling
    assert oa.grad_norm() == ob.grad_norm() and oa.grad_norm()[1] == 1.0
    torch.testing.assert_close(sb.data, sa.data, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(ob.ema[0], oa.ema[0], rtol=1e-6, atol=1e-7)
    assert not torch.equal(oa.ema[0], sa.data)


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def test_train_writes_ema_checkpoint_logs_norms_and_resumes(tmp_path, capsys):
    from distributedpytorch_amd.trainer import train
    a = train(parse_args(ARGS + EXT + ["-e", "2", "--out-dir", str(tmp_path / "a")]))
    raw, ema = _load(tmp_path / "a" / "checkpoints" / "singleGPU.pth"), _load(a["paths"]["checkpoint_ema"])
    assert a["paths"]["checkpoint_ema"].endswith("singleGPU_ema.pth")
    assert list(raw) == list(ema)
    assert any(not torch.equal(raw[k], ema[k]) for k in raw)
    recs = [json.loads(line) for line in open(tmp_path / "a" / "logs" / "singleGPU.jsonl")]
    tr, ep = [r for r in recs if r["kind"] == "train"], [r for r in recs if r["kind"] == "epoch"]
    assert tr and all(math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0 and 0 < r["clip_coef"] <= 1 for r in tr)
    assert len(ep) == 2 and all(0.0 <= r["val_dice_ema"] <= 1.0 and math.isfinite(r["val_loss_ema"]) for r in ep)
    assert "gnorm" in open(tmp_path / "a" / "logs" / "singleGPU.log").read()
    # evaluate.py scores the averaged weights with no change: -c singleGPU_ema
    import evaluate
    capsys.readouterr()
    loss, dice = evaluate.main(["-c", "singleGPU_ema", "--out-dir", str(tmp_path / "a"), "--synthetic", "--model",
                                "unet-tiny", "--img-size", "32", "--backend", "torch"])
    assert math.isfinite(loss) and "singleGPU_ema.pth" in capsys.readouterr().out
    # a run stopped after epoch 1 and resumed ends with the uninterrupted run's average
    train(parse_args(ARGS + EXT + ["-e", "1", "--out-dir", str(tmp_path / "b")]))
    assert "ema" in _load(tmp_path / "b" / "checkpoints" / "singleGPU_last.pt")["optimizer"]
    b = train(parse_args(ARGS + EXT + ["-e", "2", "--resume", "--out-dir", str(tmp_path / "b")]))
    assert a["step"] == b["step"] > 0
    ema_b = _load(tmp_path / "b" / "checkpoints" / "singleGPU_ema.pth")
    for k in ema:
        torch.testing.assert_close(ema_b[k], ema[k], rtol=1e-5, atol=1e-6, msg=k)


def test_train_without_the_flags_logs_and_writes_what_it_did(tmp_path):
    from distributedpytorch_amd.trainer import train
    out = train(parse_args(ARGS + ["-e", "1", "--out-dir", str(tmp_path)]))
    assert "checkpoint_ema" not in out["paths"] and not (tmp_path / "checkpoints" / "singleGPU_ema.pth").exists()
    for line in open(tmp_path / "logs" / "singleGPU.jsonl"):
        assert not {"grad_norm", "clip_coef", "val_dice_ema", "val_loss_ema"} & set(json.loads(line))


def test_dp_replicas_keep_identical_ema_cpu(tmp_path):
    from distributedpytorch_amd.trainer import train
    out = train(parse_args(ARGS + EXT + ["-t", "DP", "-e", "1", "--out-dir", str(tmp_path)]))
    opt = out["strategy"].optimizer
    assert len(opt.ema) == 2 and torch.equal(opt.ema[0], opt.ema[1])
    sd = _load(tmp_path / "checkpoints" / "DP_ema.pth")
    assert all(k.startswith("module.") for k in sd)


@pytest.mark.parametrize("flag", [["--clip-grad-norm", "1.0"], ["--ema-decay", "0.99"]])
def test_mp_refuses_the_flags(flag):
    from distributedpytorch_amd.trainer import build_strategy
    cfg = parse_args(ARGS + ["-t", "MP"] + flag)
    with pytest.raises(ValueError, match="-t MP"):
        build_strategy(cfg, build_model("unet-tiny"))


def test_flags_left_out_give_todays_config():
    base = parse_args(ARGS)
    assert base.clip_grad_norm == 0.0 and base.ema_decay == 0.0
    ext = parse_args(ARGS + ["--clip-grad-norm", "inf", "--ema-decay", "0.999"])
    assert ext.clip_grad_norm == float("inf") and ext.ema_decay == 0.999
    assert dataclasses.replace(ext, clip_grad_norm=0.0, ema_decay=0.0) == base
    for bad in (["--clip-grad-norm", "-1"], ["--ema-decay", "1.0"], ["--clip-grad-norm", "nan"]):
        with pytest.raises(SystemExit):
            parse_args(ARGS + bad)
