"""MI355X kernel ops (HIP, gfx950) with torch reference implementations for CPU / parity tests.

Each public op takes torch tensors.  On CUDA(=HIP) tensors it calls the hand-written kernel in
``_C/libdpa_hip.so`` (required: raises if missing); on CPU tensors it runs the plain-torch
reference of the same math, which the numerics tests compare against.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import available as hip_available, check, ptr, stream_ptr

c_float = ctypes.c_float
c_ll = ctypes.c_longlong

AUX_LEN = 8          # fp64 aux block: {sumsq, norm, coef, 1 - EMA decay of the step, reserved ...}


def _check_x(p, g, m, v, ema, aux):
    ts = [p, g, m, v] + ([] if ema is None else [ema])
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel() for t in ts)
    assert aux is None or (aux.dtype == torch.float64 and aux.numel() >= AUX_LEN and aux.device == p.device)


def _ptr_or_null(t):
    return ctypes.c_void_p(None) if t is None else ptr(t)


def adam_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, bc1, bc2, ema=None, aux=None, ema_decay=0.0):
    """In-place Adam (L2 decay) over flat fp32 tensors ``p, g, m, v`` (one launch), with two options fused into
    the same pass: ``aux`` given -> the gradient is used as ``aux[2] * g`` (the clip coefficient ``grad_sumsq``
    left on the device; ``g`` itself is not changed); ``ema`` given -> ``ema += (1 - ema_decay) * (p_new - ema)``
    on the just-updated parameter."""
    if not p.is_cuda:
        from ..optim import adam_reference
        return adam_reference(p, g, m, v, lr, beta1, beta2, eps, weight_decay, bc1, bc2,
                              coef=None if aux is None else aux[2], ema=ema, ema_decay=ema_decay)
    _check_x(p, g, m, v, ema, aux)
    if p.numel() == 0:                       # (an empty tensor has no device pointer to hand over)
        return
    L = _lib.lib()
    err = L.dpa_adam_flat(ptr(p), ptr(g), ptr(m), ptr(v), _ptr_or_null(ema), c_ll(p.numel()), c_float(lr),
                          c_float(beta1), c_float(beta2), c_float(eps), c_float(weight_decay), c_float(bc1),
                          c_float(bc2), ctypes.c_double(ema_decay), _ptr_or_null(aux), ctypes.c_int(aux is not None),
                          ctypes.c_void_p(stream_ptr(p.device)))
    check(err, "adam_flat")


def ema_decay_at(decay: float, step: int) -> float:
    """EMA decay of optimizer step ``step`` (1-based): ``min(decay, (1 + step) / (10 + step))``."""
    return min(float(decay), (1.0 + step) / (10.0 + step))


def adam_step_dev(p, g, m, v, state, *, beta1, beta2, eps, weight_decay, aux=None, ema=None, clip=False,
                  ema_decay=0.0):
    """Adam whose step count, lr and bias corrections live in ``state`` (fp64 device tensor
    ``[step, lr, 1/bc1, 1/sqrt(bc2)]``); the step increments ``state[0]`` itself, so one captured
    launch sequence is valid for every replay of a HIP graph.  The options of ``adam_step``: ``clip`` scales the
    gradient by ``aux[2]``; ``ema_decay`` is the ceiling D, the step's decay ``min(D, (1 + t) / (10 + t))`` is
    computed on the device from the step count (``aux[3]``).  Either option needs ``aux``."""
    assert state.dtype == torch.float64 and state.numel() >= 4 and state.device == p.device
    assert aux is not None or (not clip and ema is None)
    if not p.is_cuda:
        from ..optim import adam_reference
        t = float(state[0]) + 1.0
        state[0] = t
        d = ema_decay_at(ema_decay, t)
        if aux is not None:
            aux[3] = 1.0 - d
        return adam_reference(p, g, m, v, float(state[1]), beta1, beta2, eps, weight_decay, 1 - beta1 ** t,
                              1 - beta2 ** t, coef=aux[2] if clip else None, ema=ema, ema_decay=d)
    _check_x(p, g, m, v, ema, aux)
    if p.numel() == 0:
        return
    L = _lib.lib()
    err = L.dpa_adam_flat_dev(ptr(p), ptr(g), ptr(m), ptr(v), _ptr_or_null(ema), c_ll(p.numel()), ptr(state),
                              _ptr_or_null(aux), ctypes.c_double(beta1), ctypes.c_double(beta2), c_float(eps),
                              c_float(weight_decay), ctypes.c_double(ema_decay), ctypes.c_int(bool(clip)),
                              ctypes.c_void_p(stream_ptr(p.device)))
    check(err, "adam_flat_dev")


def grad_sumsq_blocks(n: int) -> int:
    """Slab entries ``grad_sumsq`` needs for ``n`` elements (a function of ``n`` only)."""
    return int(_lib.lib().dpa_grad_sumsq_blocks(c_ll(n)))


def grad_sumsq(g, aux, max_norm, slab=None):
    """Global squared norm of the flat fp32 tensor ``g``, deterministic (fp64, fixed order, no atomics), into the
    fp64 block ``aux``: ``aux[0:3] = sumsq, norm, coef`` with ``coef = min(1, max_norm / (norm + 1e-6))``
    (``torch.nn.utils.clip_grad_norm_``; ``max_norm = inf`` gives 1, a non-finite sum gives NaN).  Nothing
    is read on the host.  ``slab`` is fp64 scratch of at least ``grad_sumsq_blocks(n)`` entries (allocated
    when not given; pass one when the call is captured in a graph)."""
    assert aux.dtype == torch.float64 and aux.numel() >= AUX_LEN and aux.device == g.device
    if not g.is_cuda:
        from ..optim import clip_coef_reference
        aux[0], aux[1], aux[2] = clip_coef_reference(g, max_norm)
        return
    assert g.dtype == torch.float32 and g.is_contiguous() and aux.is_contiguous()
    if g.numel() == 0:                       # (an empty tensor has no device pointer to hand over)
        aux[:3] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
        return
    L = _lib.lib()
    if slab is None:
        slab = torch.empty(max(1, grad_sumsq_blocks(g.numel())), dtype=torch.float64, device=g.device)
    assert slab.dtype == torch.float64 and slab.is_contiguous() and slab.device == g.device
    err = L.dpa_grad_sumsq(ptr(g), c_ll(g.numel()), ptr(slab), c_ll(slab.numel()), ptr(aux),
                           ctypes.c_double(max_norm), ctypes.c_void_p(stream_ptr(g.device)))
    check(err, "grad_sumsq")


__all__ = ["adam_step", "adam_step_dev", "grad_sumsq", "grad_sumsq_blocks",
           "ema_decay_at", "AUX_LEN", "hip_available"]
