#!/usr/bin/env python3
"""Record the bits of the default Adam step: tests/golden/adam_plain_bits.npz.

Three steps of ``ops.adam_step`` (host state) and of ``ops.adam_step_dev`` (device state) on n = 1027 elements
(one full block of float4s and a tail of 3), the same gradient every step.  The fixture holds the inputs
(``p0, g, m0, v0``) and ``p, m, v`` after step 3 of each form (``host_*``, ``dev_*``), all float32, so a test needs
no random generator to reproduce them.  ``tests/test_optim_ext_gpu.py`` holds every mode of the kernel to these
bits.

Only call forms that every tree has are used (``adam_step(p, g, m, v, lr=, beta1=, beta2=, eps=, weight_decay=,
bc1=, bc2=)`` and ``adam_step_dev(p, g, m, v, state, beta1=, beta2=, eps=, weight_decay=)``), so the same script
re-records on any later tree -- which is only right after a deliberate change of the update's arithmetic.  If
the file named by ``--out`` exists, its inputs are kept unless ``--fresh`` is given.  Needs a GPU.
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N = 1027
STEPS = 3
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
WD = 1e-2            # large enough that wd * p reaches the low bits of g + wd * p: a changed contraction shows
ZERO_G = (0, 5, 300, 1023, 1025)        # float4 body and tail
ZERO_V = (5, 77, 1023, 1026)


def make_inputs(seed=0):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    a = {"p0": rng.standard_normal(N).astype(f32),
         "g": (rng.standard_normal(N) * 10.0 ** rng.uniform(-4.0, 2.0, N)).astype(f32),   # magnitudes 1e-4 .. 1e2
         "m0": (np.abs(rng.standard_normal(N)) * 0.1).astype(f32),
         "v0": (np.abs(rng.standard_normal(N)) * 0.1).astype(f32)}
    a["g"][list(ZERO_G)] = 0.0
    a["v0"][list(ZERO_V)] = 0.0
    return a


def run(inputs, dev_state):
    """``p, m, v`` (cuda tensors) after STEPS steps."""
    from distributedpytorch_amd import ops
    p, g, m, v = (torch.from_numpy(inputs[k].copy()).cuda() for k in ("p0", "g", "m0", "v0"))
    state = torch.tensor([0.0, LR, 0.0, 0.0], dtype=torch.float64, device="cuda") if dev_state else None
    kw = dict(beta1=B1, beta2=B2, eps=EPS, weight_decay=WD)
    for k in range(1, STEPS + 1):
        if dev_state:
            ops.adam_step_dev(p, g, m, v, state, **kw)
        else:
            ops.adam_step(p, g, m, v, lr=LR, bc1=1 - B1 ** k, bc2=1 - B2 ** k, **kw)
    torch.cuda.synchronize()
    if dev_state:
        assert float(state[0]) == STEPS
    return p, m, v


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "adam_plain_bits.npz"))
    ap.add_argument("--fresh", action="store_true", help="draw new inputs even if the output file exists")
    a = ap.parse_args()
    if Path(a.out).exists() and not a.fresh:
        with np.load(a.out) as z:
            inputs = {k: z[k] for k in ("p0", "g", "m0", "v0")}
    else:
        inputs = make_inputs()
    out = dict(inputs)
    for form, dev_state in (("host", False), ("dev", True)):
        for name, t in zip("pmv", run(inputs, dev_state)):
            out[f"{form}_{name}"] = t.cpu().numpy()
    assert all(x.dtype == np.float32 and x.shape == (N,) and np.isfinite(x).all() for x in out.values())
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez(a.out, **out)
    print(f"wrote {a.out}: {sorted(out)}")


if __name__ == "__main__":
    main()
