"""The inverse of the ray bender as plain torch on the CPU: the reference the kernel of csrc/nrnerf_bend_inverse.h is tested against.

``x <- x - omega (bend(x) - c)`` on ``oracle.nrnerf_oracle.bend_points``, in the dtype of the points (float64 or float32), with the kernel's
stopping rule: evaluate; ``r = max_c |bend(x)_c - c_c|``; a point with ``r <= tol`` is finished; after ``max_iters`` evaluations everything
is; otherwise update and evaluate again.  No update follows a point's last evaluation, so ``residual`` is the residual OF ``points``, and
``iterations`` counts the evaluations made (1 .. max_iters).  A NaN residual is never ``<= tol``.  Not a test module."""
from __future__ import annotations

import os

import numpy as np
import torch

from oracle import nrnerf_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def unbend_reference(canonical, latents, bender, *, knobs=None, initial=None, tol=1e-6, relaxation=1.0, max_iters=64):
    """``canonical [M, 3]``, ``latents [M, L]`` or ``[1, L]``, ``bender``: the oracle's state dict.  The arithmetic runs in ``canonical.dtype``
    (weights are cast by the oracle).  Returns ``{"points", "residual", "iterations", "converged"}``."""
    dt = canonical.dtype
    c = canonical.detach().cpu()
    M = c.shape[0]
    lat = latents.detach().cpu().to(dt).expand(M, -1)
    bd = {k: v.detach().cpu() for k, v in bender.items()}
    x = c.clone() if initial is None else initial.detach().cpu().to(dt).clone()
    tol_t = torch.tensor(float(np.float32(tol)), dtype=dt)         # the kernel compares against the float32 tolerance
    omega = torch.tensor(float(np.float32(relaxation)), dtype=dt)
    done = torch.zeros(M, dtype=torch.bool)
    res = torch.zeros(M, dtype=dt)
    its = torch.zeros(M, dtype=torch.int32)
    with torch.no_grad():
        for k in range(1, int(max_iters) + 1):
            act = ~done
            if not bool(act.any()):
                break
            idx = act.nonzero().reshape(-1)
            bent = O.bend_points(x[idx], lat[idx], bd, knobs)[0]
            d = bent - c[idx]
            r = d.abs().max(-1).values                             # (torch's max propagates NaN)
            res[idx], its[idx] = r, k
            fin = r <= tol_t                                       # NaN: False
            done[idx] = fin
            if k < max_iters:
                go = idx[~fin]
                x[go] = x[go] - omega * d[~fin]
    return {"points": x, "residual": res, "iterations": its, "converged": res <= tol_t}


def fitted(name):
    """``(checkpoint, bender state dict, half the far bound)`` of a fitted checkpoint under tests/golden; the bounds are the example sequence's."""
    from nonrigid_nerf_amd.checkpoint import load_checkpoint
    ck = load_checkpoint(os.path.join(GOLDEN, name + ".tar"), N_samples=64, N_importance=128)
    z = np.load(os.path.join(GOLDEN, "example_sequence_96x72.npz"))
    bender = {k: v.detach().clone() for k, v in ck.ray_bender.state_dict().items()}
    return ck, bender, 0.5 * float(z["bds"].max())


def cube_points(n, half, seed=0, dtype=torch.float64):
    """``n`` seeded uniform points in the cube ``[-half, half]^3`` (drawn in float64, then cast: the same points in every dtype)."""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1) * half).to(torch.float32).to(dtype)
