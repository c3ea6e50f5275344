"""The adjoint of the grid lookup as plain torch on the CPU: the reference ``nrnerf_grid_lookup_backward`` and ``field.render_baked_train`` are
tested against.

The rule of include/nrnerf.h ("the adjoint of the lookup") in the dtype asked for -- float64 as THE reference, float32 to measure what the
rule costs in the kernel's own number format (the tests' tolerances are 10 x that error): ``lookup`` is ``volume_reference.lookup_reference``
operation for operation (the same values, exactly) with the grid and the points left attached, so torch's autograd states the adjoint: the
cell index is an integer (no gradient), ``f = g - i`` has slope 1 in ``g``, ``g = (p - min) * scale`` has slope ``scale``; an empty sample (outside
the box, or NaN) is cut off by ``torch.where`` and has no gradient; on a cell face the cell is the one ``floor`` and the clamp pick -- the upper
cell, the last one on the top face -- and the derivative is that cell's.  ``render`` is ``warp_reference.render_reference`` in the same way.
Not a test module."""
from __future__ import annotations

import numpy as np
import torch

from oracle import nrnerf_oracle as O


def lookup(grid, min_point, max_point, pts):
    """``grid [Gz, Gy, Gx, 4]``, ``pts [..., 3]``, both already in the dtype of the computation (and attached where a gradient is wanted)
    -> values ``[..., 4]``."""
    dtype = grid.dtype
    gz, gy, gx = grid.shape[:3]
    lo = torch.as_tensor(np.asarray(min_point, dtype=np.float32)).to(dtype)
    hi = torch.as_tensor(np.asarray(max_point, dtype=np.float32)).to(dtype)
    top = torch.tensor([gx - 1, gy - 1, gz - 1], dtype=dtype)
    g = (pts - lo) * (top / (hi - lo))
    inside = ((g >= 0) & (g <= top)).all(-1)                        # (NaN: False)
    gs = torch.where(inside[..., None], g, torch.zeros_like(g))
    i = torch.minimum(torch.floor(gs.detach()), top - 1).to(torch.int64)
    f = gs - i.to(dtype)
    flat = grid.reshape(-1, 4)

    def corner(dx, dy, dz):
        return flat[((i[..., 2] + dz) * gy + (i[..., 1] + dy)) * gx + (i[..., 0] + dx)]

    def lerp(a, b, t):
        t = t[..., None]
        return t * b + (a - t * a)

    x00, x10 = lerp(corner(0, 0, 0), corner(1, 0, 0), f[..., 0]), lerp(corner(0, 1, 0), corner(1, 1, 0), f[..., 0])
    x01, x11 = lerp(corner(0, 0, 1), corner(1, 0, 1), f[..., 0]), lerp(corner(0, 1, 1), corner(1, 1, 1), f[..., 0])
    out = lerp(lerp(x00, x10, f[..., 1]), lerp(x01, x11, f[..., 1]), f[..., 2])
    return torch.where(inside[..., None], out, torch.zeros_like(out))


def lookup_backward(grid, min_point, max_point, pts, g_value, dtype=torch.float64):
    """``(values, d_grid [Gz, Gy, Gx, 4], d_points [..., 3])`` of ``sum(g_value * lookup)`` in ``dtype``; ``grid`` in any float dtype (widened
    first), ``pts [..., 3]``."""
    gr = grid.detach().cpu().to(dtype).requires_grad_(True)
    p = pts.detach().cpu().to(dtype).requires_grad_(True)
    v = lookup(gr, min_point, max_point, p)
    d_grid, d_pts = torch.autograd.grad((v * g_value.detach().cpu().to(dtype)).sum(), (gr, p))
    return v.detach(), d_grid, d_pts


def render(vol, min_point, max_point, warp, warp_min, warp_max, rays, z_vals, *, white_bkgd=False, rigidity_cutoff=None,
           test_time_scaling=None, removal_threshold=None):
    """``warp_reference.render_reference`` with the grids left attached (``vol`` and ``warp`` already in the dtype of the computation; ``warp``
    None: straight rays): ``rgb_map, disp_map, acc_map, weights`` and ``mask`` (the rigidity before the cutoff, detached)."""
    dtype = vol.dtype
    r, z = rays.detach().cpu().to(dtype), z_vals.detach().cpu().to(dtype)
    pts = r[:, None, 0:3] + r[:, None, 3:6] * z[..., None]
    mask = None
    if warp is not None:
        um = lookup(warp, warp_min, warp_max, pts)
        u, m = um[..., :3], um[..., 3]
        mask = m.detach().clone()
        if rigidity_cutoff is not None:
            m = torch.where(m.detach() <= float(np.float32(rigidity_cutoff)), torch.zeros_like(m), m)
        off = m[..., None] * u
        if test_time_scaling is not None:
            off = off * float(np.float32(test_time_scaling))
        pts = pts + off
    raw = lookup(vol, min_point, max_point, pts)
    if removal_threshold is not None:
        kill = m.detach() >= float(np.float32(removal_threshold))
        raw = torch.cat([raw[..., :3], torch.where(kill, raw[..., 3] * 0.0, raw[..., 3])[..., None]], -1)
    rgb_map, disp_map, acc_map, _, weights, _ = O.composite(raw, z, r[:, 3:6], white_bkgd)
    return dict(rgb_map=rgb_map, disp_map=disp_map, acc_map=acc_map, weights=weights, mask=mask)
