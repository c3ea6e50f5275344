"""Baked warps as plain torch on the CPU: the reference the kernels of csrc/nrnerf_warp.hip are tested against.

The value rule of include/nrnerf.h ("baked warps") in the dtype asked for -- float64 as THE reference, float32 to measure what the rule costs
in the kernel's own number format (the tests' tolerances are 10 x that error): ``p = o + d z``; ``(u, m)`` = the warp grid at ``p`` by the
interpolation rule of the volume (``volume_reference.lookup_reference``: outside the warp's box, or NaN, gives ``u = 0, m = 0``); ``m = 0``
where ``m <= cutoff``; ``off = m u``, times ``scaling``; ``bent = p + off``; then ``volume_reference.render_reference`` on ``points4 = (bent,
m)``: the canonical lookup, the removal knob on ``m``, the oracle's compositing, the surface reduction.  Not a test module."""
from __future__ import annotations

import numpy as np
import torch

from oracle import nrnerf_oracle as O
from tests import volume_reference as V

# the box of the warp in the accuracy series: the canonical volume's box (every sample that can meet the volume is bent by the grid)
SERIES_WARP_BOX = V.SERIES_BOX
SERIES_WARPS = (8, 16, 32, 64)
SERIES_VOLUME = 96


def bend_reference(warp, warp_min, warp_max, pts, *, rigidity_cutoff=None, test_time_scaling=None, dtype=torch.float64):
    """``pts [..., 3]`` -> ``points4 [..., 4]`` = (bent xyz, rigidity after the cutoff) in ``dtype``."""
    p = pts.detach().cpu().to(dtype)
    um = V.lookup_reference(warp, warp_min, warp_max, p, dtype)
    u, m = um[..., :3], um[..., 3]
    if rigidity_cutoff is not None:
        m = torch.where(m <= float(np.float32(rigidity_cutoff)), torch.zeros_like(m), m)          # rnh:563-564
    off = m[..., None] * u                                                                         # rnh:567
    if test_time_scaling is not None:
        off = off * float(np.float32(test_time_scaling))                                           # rnh:568-569
    return torch.cat([p + off, m[..., None]], -1)


def sample_points(rays, z_vals, dtype=torch.float64):
    """``o + d z`` in ``dtype``: ``[N, S, 3]``."""
    r, z = rays.detach().cpu().to(dtype), z_vals.detach().cpu().to(dtype)
    return r[:, None, 0:3] + r[:, None, 3:6] * z[..., None]


def render_reference(vol, min_point, max_point, warp, warp_min, warp_max, rays, z_vals, *, white_bkgd=False, rigidity_cutoff=None,
                     test_time_scaling=None, removal_threshold=None, dtype=torch.float64):
    """What nrnerf_warped_volume_render computes, in ``dtype``: ``volume_reference.render_reference``'s outputs on the bent samples, plus
    ``points4`` and the straight sample points ``points``."""
    pts = sample_points(rays, z_vals, dtype)
    p4 = bend_reference(warp, warp_min, warp_max, pts, rigidity_cutoff=rigidity_cutoff, test_time_scaling=test_time_scaling, dtype=dtype)
    if p4.shape[1] == 1:
        out = _render_one_sample(vol, min_point, max_point, rays, z_vals, p4, white_bkgd, removal_threshold, dtype)
    else:
        out = V.render_reference(vol, min_point, max_point, rays, z_vals, p4, white_bkgd=white_bkgd, removal_threshold=removal_threshold, dtype=dtype)
    out["points4"], out["points"] = p4, pts
    return out


def _render_one_sample(vol, min_point, max_point, rays, z_vals, p4, white_bkgd, removal_threshold, dtype):
    """``volume_reference.render_reference`` for S = 1, which raw2outputs' slicing (train.py:743-746, the oracle's too) does not take: the one
    sample is the last one, its distance 1e10 |d|, its transmittance 1."""
    r, z = rays.detach().cpu().to(dtype), z_vals.detach().cpu().to(dtype)
    raw = V.lookup_reference(vol, min_point, max_point, p4[..., :3], dtype)
    if removal_threshold is not None:
        kill = p4[..., 3] >= float(np.float32(removal_threshold))
        raw = raw.clone()
        raw[..., 3] = torch.where(kill, raw[..., 3] * 0.0, raw[..., 3])
    dists = torch.full_like(z, 1e10) * torch.norm(r[:, None, 3:6], dim=-1)
    alpha = 1.0 - torch.exp(-torch.relu(raw[..., 3]) * dists)
    weights = alpha * (torch.ones_like(alpha))
    rgb_map = torch.sum(weights[..., None] * torch.sigmoid(raw[..., :3]), -2)
    depth_map, acc_map = torch.sum(weights * z, -1), torch.sum(weights, -1)
    disp_map = 1.0 / torch.max(1e-10 * torch.ones_like(depth_map), depth_map / acc_map)
    if white_bkgd:
        rgb_map = rgb_map + (1.0 - acc_map[..., None])
    n = r.shape[0]
    return dict(rgb_map=rgb_map, disp_map=disp_map, acc_map=acc_map, raw=raw, weights=weights, alpha=alpha,
                median_index=torch.zeros(n, dtype=torch.int64), median_gap=torch.full((n,), float("inf"), dtype=dtype),
                surface_pts=p4[:, 0, :3], surface_rigidity=p4[:, 0, 3])


def smooth_warp(gx, gy, gz, seed=0, amplitude=0.15):
    """A seeded smooth random warp ``[Gz, Gy, Gx, 4]`` float32: offsets of up to ``amplitude`` per axis (a few plane waves each) and a rigidity
    mask that sweeps the whole of 0 .. 1."""
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = torch.meshgrid(torch.linspace(0, 1, gz, dtype=torch.float64), torch.linspace(0, 1, gy, dtype=torch.float64),
                                torch.linspace(0, 1, gx, dtype=torch.float64), indexing="ij")
    w = torch.zeros(gz, gy, gx, 4, dtype=torch.float64)
    for c in range(4):
        for _ in range(2):
            k = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1) * 5.0
            ph = torch.rand(1, generator=g, dtype=torch.float64) * 6.28
            w[..., c] += 0.5 * torch.sin(k[0] * xx + k[1] * yy + k[2] * zz + ph)
    w[..., :3] *= amplitude
    w[..., 3] = 0.5 + 0.5 * w[..., 3]
    return w.to(torch.float32)


def grid_vertices(min_point, max_point, resolution, dtype=torch.float64):
    """The vertices of nrnerf_grid_points' grid in ``dtype``: ``[Gz, Gy, Gx, 3]``."""
    gx, gy, gz = (resolution,) * 3 if isinstance(resolution, int) else resolution
    lo, hi = np.asarray(min_point, dtype=np.float32).astype(np.float64), np.asarray(max_point, dtype=np.float32).astype(np.float64)
    axes = [torch.as_tensor(lo[c] + np.arange(n) * ((hi[c] - lo[c]) / (n - 1))).to(dtype) for c, n in enumerate((gx, gy, gz))]
    zz, yy, xx = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return torch.stack([xx, yy, zz], -1)


def bake_warp_reference(scene, code, resolution, min_point=SERIES_WARP_BOX[0], max_point=SERIES_WARP_BOX[1], dtype=torch.float64):
    """The oracle's bender (no knobs) at the vertices of the grid: ``[Gz, Gy, Gx, 4]`` = (unmasked offsets, rigidity mask) in ``dtype``."""
    v = grid_vertices(min_point, max_point, resolution, dtype)
    flat = v.reshape(-1, 3)
    with torch.no_grad():
        _, det = O.bend_points(flat, code.to(dtype).reshape(1, -1).expand(flat.shape[0], -1), scene.bender)
    return torch.cat([det["unmasked_offsets"], det["rigidity_mask"]], -1).reshape(tuple(v.shape[:3]) + (4,))
