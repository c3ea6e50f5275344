"""The adjoint of the spherical-harmonic colour sum as plain torch on the CPU: the reference ``nrnerf_sh_lookup_backward`` and
``field.sh_lookup`` / ``render_sh_train`` / ``refine_sh_bake`` are tested against.

The rule of include/nrnerf.h ("the adjoint of the colour sum") in the dtype asked for -- float64 as THE reference, float32 to measure what the
rule costs in the kernel's own number format (the tests' tolerances are 10 x that error): ``lookup_channels``, ``basis`` and ``directions`` are
``tests/sh_reference.py``'s operation for operation (the same values, exactly) with the coefficients, the points and the directions left attached,
so torch's autograd states the adjoint: the basis functions are polynomials in an unconstrained ``d``; the cell index is an integer (no
gradient); an empty sample (outside the box, or NaN) is cut off by ``torch.where`` and has no gradient; on a cell face the derivative is the
one of the cell ``floor`` and the clamp pick; under DIFFERENCES ``d_i = e_i / (|e_i| + 1e-6)`` with ``d_0 = d_1`` carries the gradient of the
directions back to the points.  ``render`` is ``sh_reference.render_reference`` in the same way.  Not a test module."""
from __future__ import annotations

import numpy as np
import torch

from tests import grid_grad_reference as G
from tests.sh_reference import C0, C1, C2, C20, C22, EPS


def lookup_channels(grid, min_point, max_point, pts):
    """``sh_reference.lookup_channels`` with ``grid [Gz, Gy, Gx, C]`` and ``pts [..., 3]`` already in the dtype of the computation and left
    attached -> ``[..., C]``."""
    dtype = grid.dtype
    gz, gy, gx, ch = grid.shape
    lo = torch.as_tensor(np.asarray(min_point, dtype=np.float32)).to(dtype)
    hi = torch.as_tensor(np.asarray(max_point, dtype=np.float32)).to(dtype)
    top = torch.tensor([gx - 1, gy - 1, gz - 1], dtype=dtype)
    g = (pts - lo) * (top / (hi - lo))
    inside = ((g >= 0) & (g <= top)).all(-1)                        # (NaN: False)
    gs = torch.where(inside[..., None], g, torch.zeros_like(g))
    i = torch.minimum(torch.floor(gs.detach()), top - 1).to(torch.int64)
    f = gs - i.to(dtype)
    flat = grid.reshape(-1, ch)

    def corner(dx, dy, dz):
        return flat[((i[..., 2] + dz) * gy + (i[..., 1] + dy)) * gx + (i[..., 0] + dx)]

    def lerp(a, b, t):
        t = t[..., None]
        return t * b + (a - t * a)

    x00, x10 = lerp(corner(0, 0, 0), corner(1, 0, 0), f[..., 0]), lerp(corner(0, 1, 0), corner(1, 1, 0), f[..., 0])
    x01, x11 = lerp(corner(0, 0, 1), corner(1, 0, 1), f[..., 0]), lerp(corner(0, 1, 1), corner(1, 1, 1), f[..., 0])
    out = lerp(lerp(x00, x10, f[..., 1]), lerp(x01, x11, f[..., 1]), f[..., 2])
    return torch.where(inside[..., None], out, torch.zeros_like(out))


def basis(d, degree):
    """``sh_reference.basis`` with ``d [..., 3]`` left attached: ``[..., K]``."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = [torch.full_like(x, C0)]
    if degree >= 1:
        out += [C1 * -y, C1 * z, C1 * -x]
    if degree >= 2:
        xx, yy, zz = x * x, y * y, z * z
        out += [C2 * (x * y), -C2 * (y * z), C20 * ((2.0 * zz - xx) - yy), -C2 * (x * z), C22 * (xx - yy)]
    return torch.stack(out, -1)


def directions(p4, rays, ray_directions):
    """``sh_reference.directions`` with ``p4 [N, S, >= 3]`` (already in the dtype of the computation) left attached: ``[N, S, 3]``."""
    if ray_directions:
        e = rays.detach().cpu().to(p4.dtype)[:, None, 3:6]
        return (e / torch.sqrt((e * e).sum(-1, keepdim=True))).expand(-1, p4.shape[1], -1)
    e = p4[:, 1:, :3] - p4[:, :-1, :3]
    d = e / (torch.sqrt((e * e).sum(-1, keepdim=True)) + EPS)
    return torch.cat([d[:, :1], d], 1)


def colour_sum(sh, degree, min_point, max_point, pts, d):
    """``s [N, S, 3]``: ``s_c = sum over k = 1 .. K - 1, ascending, of Y_k(d) v_{k,c}(pts)``."""
    v = lookup_channels(sh, min_point, max_point, pts)
    Y = basis(d, degree)
    s = torch.zeros(pts.shape[:-1] + (3,), dtype=sh.dtype)
    cols = [s[..., c] for c in range(3)]
    for k in range(1, (degree + 1) ** 2):
        for c in range(3):
            cols[c] = cols[c] + Y[..., k] * v[..., 3 * (k - 1) + c]
    return torch.stack(cols, -1)


def lookup_backward(sh, degree, min_point, max_point, points, g, *, rays=None, ray_directions=False, dtype=torch.float64):
    """``(d_sh [Gz, Gy, Gx, 12 L], d_points [N, S, 3], d_dirs [N, S, 3])`` of ``sum <g, s>`` in ``dtype``: ``sh`` in any float dtype (widened first),
    ``points [N, S, >= 3]``, ``g [N, S, >= 3]`` (channels 0 .. 2).  ``d_dirs`` is the gradient with respect to the directions as free variables
    (``d_0`` one of them), ``d_points`` the position part plus, under DIFFERENCES, the chain from the directions back to the points."""
    coeff = sh.detach().cpu().to(dtype).requires_grad_(True)
    p = points.detach().cpu().to(dtype)[..., :3].clone().requires_grad_(True)
    d_of_p = directions(p, rays, ray_directions)
    d = d_of_p.detach().clone().requires_grad_(True)
    cot = g.detach().cpu().to(dtype)[..., :3]
    loss = (colour_sum(coeff, degree, min_point, max_point, p, d) * cot).sum()
    d_sh, d_pos, d_dirs = torch.autograd.grad(loss, (coeff, p, d))
    if ray_directions:
        return d_sh, d_pos, d_dirs
    (chain,) = torch.autograd.grad((d_of_p * d_dirs).sum(), p)
    return d_sh, d_pos + chain, d_dirs


def render(vol, sh, degree, min_point, max_point, warp, warp_min, warp_max, rays, z_vals, *, white_bkgd=False, rigidity_cutoff=None,
           test_time_scaling=None, removal_threshold=None):
    """``sh_reference.render_reference`` with the grids left attached (``vol``, ``sh`` and ``warp`` already in the dtype of the computation;
    ``warp`` None: straight rays and the RAY rule, else DIFFERENCES): ``rgb_map, disp_map, acc_map, weights, raw`` and ``mask`` (the rigidity
    before the cutoff, detached)."""
    from oracle import nrnerf_oracle as O
    dtype = vol.dtype
    r, z = rays.detach().cpu().to(dtype), z_vals.detach().cpu().to(dtype)
    pts = r[:, None, 0:3] + r[:, None, 3:6] * z[..., None]
    mask = None
    if warp is not None:
        um = G.lookup(warp, warp_min, warp_max, pts)
        u, m = um[..., :3], um[..., 3]
        mask = m.detach().clone()
        if rigidity_cutoff is not None:
            m = torch.where(m.detach() <= float(np.float32(rigidity_cutoff)), torch.zeros_like(m), m)
        off = m[..., None] * u
        if test_time_scaling is not None:
            off = off * float(np.float32(test_time_scaling))
        pts = pts + off
    d = directions(pts, rays, warp is None)
    base = G.lookup(vol, min_point, max_point, pts)
    v = lookup_channels(sh, min_point, max_point, pts)
    Y = basis(d, degree)
    cols = [base[..., c] for c in range(3)]
    for k in range(1, (degree + 1) ** 2):
        for c in range(3):
            cols[c] = cols[c] + Y[..., k] * v[..., 3 * (k - 1) + c]
    sigma = base[..., 3]
    if removal_threshold is not None:
        kill = m.detach() >= float(np.float32(removal_threshold))
        sigma = torch.where(kill, sigma * 0.0, sigma)
    raw = torch.stack(cols + [sigma], -1)
    rgb_map, disp_map, acc_map, _, weights, _ = O.composite(raw, z, r[:, 3:6], white_bkgd)
    return dict(rgb_map=rgb_map, disp_map=disp_map, acc_map=acc_map, weights=weights, raw=raw, mask=mask)
