"""View-dependent bakes as plain torch on the CPU: the reference the kernels of csrc/nrnerf_sh_volume.hip and ``field.bake(sh_degree=...)`` are
tested against.

The value rule of include/nrnerf.h ("view-dependent bakes") in the dtype asked for -- float64 as THE reference, float32 to measure what the
rule costs in the kernel's own number format (the tests' tolerances are 10 x that error): the bent points ``(b, m)`` of a ray's samples (a
warp by ``warp_reference.bend_reference``, ready-made ``points4``, or the straight samples with ``m = 0``); the direction of a sample, by
DIFFERENCES ``d_i = (b_i - b_{i-1}) / (|b_i - b_{i-1}| + 1e-6)``, ``d_0 = d_1`` (run_nerf_helpers.py:339-351) or the RAY's own ``d / |d|``; the
colour logit ``raw_c + sum_k Y_k(d) v_{k,c}`` over ``k = 1 .. K - 1`` ascending, ``raw`` by ``volume_reference.lookup_reference`` and ``v`` by the
same interpolation of the ``sh`` array (``lookup_channels``); the removal knob on ``m``; the oracle's compositing; the surface reduction.
And the projection ``bake`` makes: the 26-point Lebedev rule.  Not a test module."""
from __future__ import annotations

import numpy as np
import torch

from oracle import nrnerf_oracle as O
from tests import volume_reference as V
from tests import warp_reference as W

C0, C1, C2, C20, C22 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
EPS = float(np.float32(1e-6))          # the record's 1e-6 is a float32


def lebedev_26():
    """``(directions [26, 3], weights [26])`` float64: 6 axis directions (1/21), 12 edge directions (4/105), 8 corner directions (9/280), the
    weights summing to 1.  Written out on its own here: the order must be ``field.SH_DIRECTIONS``' (asserted by the tests)."""
    rows = []
    for c in range(3):
        for s in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]
            v[c] = s
            rows.append(v)
    for skip in (2, 0, 1):
        for s0 in (1.0, -1.0):
            for s1 in (1.0, -1.0):
                v = [0.0, 0.0, 0.0]
                v[(skip + 1) % 3], v[(skip + 2) % 3] = s0, s1
                rows.append(v)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                rows.append([sx, sy, sz])
    d = torch.tensor(rows, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    w = torch.tensor([1.0 / 21.0] * 6 + [4.0 / 105.0] * 12 + [9.0 / 280.0] * 8, dtype=torch.float64)
    return d, w


def basis(dirs, degree, dtype=torch.float64):
    """``Y_0 .. Y_{K-1}`` at ``dirs [..., 3]`` in ``dtype``: ``[..., K]``, ``K = (degree + 1)^2``."""
    d = dirs.detach().cpu().to(dtype)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = [torch.full_like(x, C0)]
    if degree >= 1:
        out += [C1 * -y, C1 * z, C1 * -x]
    if degree >= 2:
        xx, yy, zz = x * x, y * y, z * z
        out += [C2 * (x * y), -C2 * (y * z), C20 * ((2.0 * zz - xx) - yy), -C2 * (x * z), C22 * (xx - yy)]
    return torch.stack(out, -1)


def project(f, degree):
    """The coefficients of ``f [26, ...]`` (its values at the 26 directions) under the rule, float64: ``[K, ...]``, ``c_k = 4 pi sum_d w_d Y_k(d)
    f(d)``."""
    d, w = lebedev_26()
    Y = basis(d, degree)                                                    # [26, K]
    f = f.detach().cpu().double()
    return 4.0 * np.pi * torch.einsum("d,dk,d...->k...", w, Y, f)


def bake_reference(f, degree):
    """What ``bake(sh_degree=degree)`` keeps of the colour logits ``f [26, ..., 3]`` at the 26 directions, float64: ``(mean [..., 3], sh [...,
    12 * degree])`` -- channel ``3 (k - 1) + c``; degree 1: three zero channels; degree 0: ``sh`` is None."""
    _, w = lebedev_26()
    f = f.detach().cpu().double()
    mean = torch.einsum("d,d...->...", w, f)
    if degree == 0:
        return mean, None
    c = project(f, degree)[1:]                                              # [K - 1, ..., 3]
    sh = torch.zeros(tuple(f.shape[1:-1]) + (12 * degree,), dtype=torch.float64)
    sh[..., :3 * c.shape[0]] = torch.movedim(c, 0, -2).reshape(tuple(f.shape[1:-1]) + (3 * c.shape[0],))
    return mean, sh


def lookup_channels(grid, min_point, max_point, pts, dtype=torch.float64):
    """``volume_reference.lookup_reference`` for any number of channels: ``grid [Gz, Gy, Gx, C]``, ``pts [..., 3]`` -> ``[..., C]``."""
    v = grid.detach().cpu().to(dtype)
    gz, gy, gx, ch = v.shape
    lo = torch.as_tensor(np.asarray(min_point, dtype=np.float32)).to(dtype)
    hi = torch.as_tensor(np.asarray(max_point, dtype=np.float32)).to(dtype)
    top = torch.tensor([gx - 1, gy - 1, gz - 1], dtype=dtype)
    p = pts.detach().cpu().to(dtype)
    g = (p - lo) * (top / (hi - lo))
    inside = ((g >= 0) & (g <= top)).all(-1)
    gs = torch.where(inside[..., None], g, torch.zeros_like(g))
    i = torch.minimum(torch.floor(gs), top - 1).to(torch.int64)
    f = gs - i.to(dtype)
    flat = v.reshape(-1, ch)

    def corner(dx, dy, dz):
        return flat[((i[..., 2] + dz) * gy + (i[..., 1] + dy)) * gx + (i[..., 0] + dx)]

    def lerp(a, b, t):
        t = t[..., None]
        return t * b + (a - t * a)

    x00, x10 = lerp(corner(0, 0, 0), corner(1, 0, 0), f[..., 0]), lerp(corner(0, 1, 0), corner(1, 1, 0), f[..., 0])
    x01, x11 = lerp(corner(0, 0, 1), corner(1, 0, 1), f[..., 0]), lerp(corner(0, 1, 1), corner(1, 1, 1), f[..., 0])
    out = lerp(lerp(x00, x10, f[..., 1]), lerp(x01, x11, f[..., 1]), f[..., 2])
    return torch.where(inside[..., None], out, torch.zeros_like(out))


def directions(p4, rays, ray_directions, dtype=torch.float64):
    """The direction of every sample: ``[N, S, 3]``."""
    if ray_directions:
        e = rays.detach().cpu().to(dtype)[:, None, 3:6]
        return (e / torch.sqrt((e * e).sum(-1, keepdim=True))).expand(-1, p4.shape[1], -1)
    e = p4[:, 1:, :3] - p4[:, :-1, :3]
    d = e / (torch.sqrt((e * e).sum(-1, keepdim=True)) + EPS)
    return torch.cat([d[:, :1], d], 1)


def render_reference(vol, sh, degree, min_point, max_point, rays, z_vals, *, warp=None, warp_min=None, warp_max=None, points4=None,
                     ray_directions=None, white_bkgd=False, rigidity_cutoff=None, test_time_scaling=None, removal_threshold=None,
                     dtype=torch.float64):
    """What nrnerf_sh_volume_render computes, in ``dtype``: ``rgb_map, disp_map, acc_map, raw, weights, alpha, median_index, median_gap,
    surface_pts, surface_rigidity, points4, dirs``.  ``ray_directions=None``: differences whenever a warp or ``points4`` is given."""
    r, z = rays.detach().cpu().to(dtype), z_vals.detach().cpu().to(dtype)
    pts = W.sample_points(rays, z_vals, dtype)
    if warp is not None:
        p4 = W.bend_reference(warp, warp_min, warp_max, pts, rigidity_cutoff=rigidity_cutoff, test_time_scaling=test_time_scaling, dtype=dtype)
    elif points4 is not None:
        p4 = points4.detach().cpu().to(dtype)
    else:
        p4 = torch.cat([pts, torch.zeros_like(pts[..., :1])], -1)
    if ray_directions is None:
        ray_directions = warp is None and points4 is None
    d = directions(p4, rays, ray_directions, dtype)
    raw = V.lookup_reference(vol, min_point, max_point, p4[..., :3], dtype).clone()
    v = lookup_channels(sh, min_point, max_point, p4[..., :3], dtype)
    Y = basis(d, degree, dtype)
    for k in range(1, (degree + 1) ** 2):
        for c in range(3):
            raw[..., c] = raw[..., c] + Y[..., k] * v[..., 3 * (k - 1) + c]
    if removal_threshold is not None:
        kill = p4[..., 3] >= float(np.float32(removal_threshold))
        raw[..., 3] = torch.where(kill, raw[..., 3] * 0.0, raw[..., 3])
    out = composite_reference(raw, z, r, p4, white_bkgd, dtype)
    out["points4"], out["dirs"] = p4, d
    return out


def composite_reference(raw, z, r, p4, white_bkgd, dtype):
    """``volume_reference.render_reference`` behind its lookup (``warp_reference._render_one_sample`` for S = 1): the oracle's compositing and
    the surface reduction over ``p4``."""
    n = r.shape[0]
    if raw.shape[1] == 1:
        dists = torch.full_like(z, 1e10) * torch.norm(r[:, None, 3:6], dim=-1)
        alpha = 1.0 - torch.exp(-torch.relu(raw[..., 3]) * dists)
        weights = alpha * (torch.ones_like(alpha))
        rgb_map = torch.sum(weights[..., None] * torch.sigmoid(raw[..., :3]), -2)
        depth_map, acc_map = torch.sum(weights * z, -1), torch.sum(weights, -1)
        disp_map = 1.0 / torch.max(1e-10 * torch.ones_like(depth_map), depth_map / acc_map)
        if white_bkgd:
            rgb_map = rgb_map + (1.0 - acc_map[..., None])
        return dict(rgb_map=rgb_map, disp_map=disp_map, acc_map=acc_map, raw=raw, weights=weights, alpha=alpha,
                    median_index=torch.zeros(n, dtype=torch.int64), median_gap=torch.full((n,), float("inf"), dtype=dtype),
                    surface_pts=p4[:, 0, :3], surface_rigidity=p4[:, 0, 3])
    rgb_map, disp_map, acc_map, alpha, weights, _ = O.composite(raw, z, r[:, 3:6], white_bkgd)
    cum = torch.cumsum(weights, -1)
    dist = (cum - 0.5).abs()
    idx = torch.argmin(dist, -1)
    rival = torch.where(cum == torch.gather(cum, 1, idx[:, None]), torch.full_like(dist, float("inf")), dist)
    out = dict(rgb_map=rgb_map, disp_map=disp_map, acc_map=acc_map, raw=raw, weights=weights, alpha=alpha, median_index=idx,
               median_gap=rival.min(-1).values - torch.gather(dist, 1, idx[:, None])[:, 0])
    pick = idx[:, None, None]
    out["surface_pts"] = torch.gather(p4[..., :3], 1, pick.expand(-1, 1, 3))[:, 0]
    out["surface_rigidity"] = torch.gather(p4[..., 3], 1, pick[..., 0])[:, 0]
    return out


def smooth_sh(gx, gy, gz, degree, seed=0, amplitude=1.5):
    """A seeded smooth random coefficient array ``[Gz, Gy, Gx, 12 * degree]`` float32 (degree 1: the last three channels zero): a plane wave
    or two per channel, a unit or so in size -- next to ``volume_reference.smooth_volume``'s colour logits of a few units."""
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = torch.meshgrid(torch.linspace(0, 1, gz, dtype=torch.float64), torch.linspace(0, 1, gy, dtype=torch.float64),
                                torch.linspace(0, 1, gx, dtype=torch.float64), indexing="ij")
    ch = 12 * degree
    used = 3 * ((degree + 1) ** 2 - 1)
    sh = torch.zeros(gz, gy, gx, ch, dtype=torch.float64)
    for c in range(used):
        for _ in range(2):
            k = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1) * 6.0
            ph, amp = torch.rand(1, generator=g, dtype=torch.float64) * 6.28, torch.rand(1, generator=g, dtype=torch.float64) * amplitude
            sh[..., c] += amp * torch.sin(k[0] * xx + k[1] * yy + k[2] * zz + ph)
    return sh.to(torch.float32)
