"""Baked volumes as plain torch on the CPU: the reference the kernels of csrc/nrnerf_volume.hip are tested against.

The sampling rule of include/nrnerf.h ("baked volumes") in the dtype asked for -- float64 as THE reference, float32 to measure what the
rule costs in the kernel's own number format (the tests' tolerances are 10 x that error, as tests/test_unbend.py does): the grid is
vertex-centred, ``g_c = (p_c - min_c) * ((G_c - 1) / (max_c - min_c))``; a sample with any ``g_c`` NaN, ``< 0`` or ``> G_c - 1`` is EMPTY, raw =
0; else ``i_c = min(floor(g_c), G_c - 2)``, ``f_c = g_c - i_c`` and the eight corners are interpolated along x, then y, then z with
``lerp(a, b, f) = f b + (a - f a)``, which returns ``a`` at ``f = 0`` and ``b`` at ``f = 1`` exactly.  Compositing is the oracle's
(``oracle.nrnerf_oracle.composite``); the surface reduction is ``surface_from_details``' rule.  Not a test module."""
from __future__ import annotations

import os

import numpy as np
import torch

from oracle import nrnerf_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

# the box of the resolution series (the bent samples of frame 3 of the example sequence stay inside it)
SERIES_BOX = ((-0.8, -0.9, -1.4), (1.25, 0.8, 0.0))
SERIES_FRAME, SERIES_WIDTH, SERIES_SAMPLES = 3, 48, 192


def lookup_reference(vol, min_point, max_point, pts, dtype=torch.float64):
    """``vol [Gz, Gy, Gx, 4]`` (any float dtype: widened first), ``pts [..., 3]`` -> logits ``[..., 4]`` in ``dtype``."""
    v = vol.detach().cpu().to(dtype)
    gz, gy, gx = v.shape[:3]
    lo = torch.as_tensor(np.asarray(min_point, dtype=np.float32)).to(dtype)
    hi = torch.as_tensor(np.asarray(max_point, dtype=np.float32)).to(dtype)
    top = torch.tensor([gx - 1, gy - 1, gz - 1], dtype=dtype)
    p = pts.detach().cpu().to(dtype)
    g = (p - lo) * (top / (hi - lo))
    inside = ((g >= 0) & (g <= top)).all(-1)                        # (NaN: False)
    gs = torch.where(inside[..., None], g, torch.zeros_like(g))
    i = torch.minimum(torch.floor(gs), top - 1).to(torch.int64)
    f = gs - i.to(dtype)
    flat = v.reshape(-1, 4)

    def corner(dx, dy, dz):
        return flat[((i[..., 2] + dz) * gy + (i[..., 1] + dy)) * gx + (i[..., 0] + dx)]

    def lerp(a, b, t):
        t = t[..., None]
        return t * b + (a - t * a)

    x00, x10 = lerp(corner(0, 0, 0), corner(1, 0, 0), f[..., 0]), lerp(corner(0, 1, 0), corner(1, 1, 0), f[..., 0])
    x01, x11 = lerp(corner(0, 0, 1), corner(1, 0, 1), f[..., 0]), lerp(corner(0, 1, 1), corner(1, 1, 1), f[..., 0])
    out = lerp(lerp(x00, x10, f[..., 1]), lerp(x01, x11, f[..., 1]), f[..., 2])
    return torch.where(inside[..., None], out, torch.zeros_like(out))


def coarse_depths(rays, n_samples, lindisp=False, dtype=torch.float64):
    """The coarse spacing between the rays' near and far (train.py:847-853) in ``dtype``: ``[N, S]``."""
    r = rays.detach().cpu().to(dtype)
    near, far = r[:, 6:7], r[:, 7:8]
    t = torch.linspace(0.0, 1.0, steps=n_samples, dtype=torch.float32).to(dtype)
    if lindisp:
        return 1.0 / (1.0 / near * (1.0 - t) + 1.0 / far * t)
    return near * (1.0 - t) + far * t


def render_reference(vol, min_point, max_point, rays, z_vals, points4=None, *, white_bkgd=False, removal_threshold=None, dtype=torch.float64):
    """What nrnerf_volume_render computes, in ``dtype``: the samples are ``points4[..., :3]`` or ``o + d z``.  Returns ``rgb_map, disp_map,
    acc_map, raw, weights, alpha, median_index`` and ``median_gap`` (how far the runner-up of the median sample is behind the winner)."""
    r = rays.detach().cpu().to(dtype)
    z = z_vals.detach().cpu().to(dtype)
    if points4 is not None:
        p4 = points4.detach().cpu().to(dtype)
        pts = p4[..., :3]
    else:
        pts = r[:, None, 0:3] + r[:, None, 3:6] * z[..., None]
    raw = lookup_reference(vol, min_point, max_point, pts, dtype)
    if removal_threshold is not None:
        kill = p4[..., 3] >= float(np.float32(removal_threshold))
        raw = raw.clone()
        raw[..., 3] = torch.where(kill, raw[..., 3] * 0.0, raw[..., 3])
    rgb_map, disp_map, acc_map, alpha, weights, _ = O.composite(raw, z, r[:, 3:6], white_bkgd)
    cum = torch.cumsum(weights, -1)
    dist = (cum - 0.5).abs()
    idx = torch.argmin(dist, -1)
    # how far the runner-up is behind: over the samples whose accumulated weight DIFFERS from the winner's (a plateau of zero weights repeats
    # the winner's value exactly and resolves to its first sample in every implementation)
    rival = torch.where(cum == torch.gather(cum, 1, idx[:, None]), torch.full_like(dist, float("inf")), dist)
    out = dict(rgb_map=rgb_map, disp_map=disp_map, acc_map=acc_map, raw=raw, weights=weights, alpha=alpha, median_index=idx,
               median_gap=rival.min(-1).values - torch.gather(dist, 1, idx[:, None])[:, 0])
    if points4 is not None:
        idx = out["median_index"][:, None, None]
        out["surface_pts"] = torch.gather(p4[..., :3], 1, idx.expand(-1, 1, 3))[:, 0]
        out["surface_rigidity"] = torch.gather(p4[..., 3], 1, idx[..., 0])[:, 0]
    return out


def smooth_volume(gx, gy, gz, seed=0):
    """A seeded smooth random volume ``[Gz, Gy, Gx, 4]`` float32: a few random plane waves per channel, colour logits of a few units; the
    sigma logits have shorter waves, a larger swing and a positive mean, so that rays through the box meet empty and opaque stretches."""
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = torch.meshgrid(torch.linspace(0, 1, gz, dtype=torch.float64), torch.linspace(0, 1, gy, dtype=torch.float64),
                                torch.linspace(0, 1, gx, dtype=torch.float64), indexing="ij")
    vol = torch.zeros(gz, gy, gx, 4, dtype=torch.float64)
    for c in range(4):
        for _ in range(3):
            k = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1) * (14.0 if c == 3 else 6.0)
            ph, amp = torch.rand(1, generator=g, dtype=torch.float64) * 6.28, torch.rand(1, generator=g, dtype=torch.float64) * 3.0
            vol[..., c] += amp * torch.sin(k[0] * xx + k[1] * yy + k[2] * zz + ph)
    vol[..., 3] = 3.0 * vol[..., 3] + 2.0
    return vol.to(torch.float32)


def interior_points(shape, min_point, max_point, seed=0, margin=1e-3, outside_share=0.25):
    """Seeded points ``shape + (3,)`` float32 around the box: most inside, ``outside_share`` of them pushed out along one axis; every
    coordinate at least ``margin`` of the extent away from both faces of its axis (the empty / non-empty rule is discontinuous there)."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.as_tensor(np.asarray(min_point, dtype=np.float64))
    ext = torch.as_tensor(np.asarray(max_point, dtype=np.float64)) - lo
    n = int(np.prod(shape))
    u = margin + torch.rand(n, 3, generator=g, dtype=torch.float64) * (1 - 2 * margin)           # inside, off the faces
    out = torch.rand(n, generator=g, dtype=torch.float64) < outside_share
    axis = torch.randint(0, 3, (n,), generator=g)
    side = torch.rand(n, generator=g, dtype=torch.float64) < 0.5
    far = margin + torch.rand(n, generator=g, dtype=torch.float64) * 0.3                         # how far beyond the face
    pushed = torch.where(side, 1 + far, -far)
    u[out, axis[out]] = pushed[out]
    return (lo + u * ext).to(torch.float32).reshape(tuple(shape) + (3,))


def psnr(a, b):
    """PSNR of two images with values in 0 .. 1 (free_viewpoint_rendering.py:821-828), in float64."""
    mse = float(((a.detach().cpu().double() - b.detach().cpu().double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * float(np.log10(mse))


def series_setup():
    """The resolution series' fixed half: ``fitted_latest``, frame 3 of the example sequence at width 48 (48 x 36 rays), 192 samples of the
    coarse spacing.  Returns ``(checkpoint, scene, rays float32 [N, 8], code [1, L])``."""
    from nonrigid_nerf_amd.checkpoint import load_checkpoint
    from nonrigid_nerf_amd.synthetic import Scene, SceneConfig
    ck = load_checkpoint(os.path.join(GOLDEN, "fitted_latest.tar"), N_samples=64, N_importance=128)
    z = np.load(os.path.join(GOLDEN, "example_sequence_96x72.npz"))
    near, far = float(z["bds"].min()) * 0.9, float(z["bds"].max())
    cfg = SceneConfig(near=near, far=far)
    sd = lambda m: {k: v.detach().clone() for k, v in m.state_dict().items()}
    scene = Scene(cfg, sd(ck.ray_bender), sd(ck.network_fn), sd(ck.network_fine))
    s = SERIES_WIDTH / float(z["hwf"][1])
    h = int(round(float(z["hwf"][0]) * s))
    intrin = dict(height=h, width=SERIES_WIDTH, focal_x=float(z["hwf"][2]) * s, focal_y=float(z["hwf"][2]) * s, center_x=SERIES_WIDTH / 2,
                  center_y=h / 2)
    ro, rd = O.get_rays(torch.from_numpy(z["poses"][SERIES_FRAME]).float(), intrin)
    rays = O.pack_rays(ro.reshape(-1, 3), rd.reshape(-1, 3), near, far, False).float()
    return ck, scene, rays, ck.latents[SERIES_FRAME].detach().reshape(1, -1).float()


def bake_reference(scene, resolution, min_point=SERIES_BOX[0], max_point=SERIES_BOX[1], dtype=torch.float64, chunk=1 << 16):
    """The canonical bake of ``scene``'s fine network in ``dtype``: logits ``[Gz, Gy, Gx, 4]`` at the vertices of nrnerf_grid_points' grid."""
    gx, gy, gz = (resolution,) * 3 if isinstance(resolution, int) else resolution
    lo, hi = np.asarray(min_point, dtype=np.float32).astype(np.float64), np.asarray(max_point, dtype=np.float32).astype(np.float64)
    axes = [torch.as_tensor(lo[c] + np.arange(n) * ((hi[c] - lo[c]) / (n - 1))).to(dtype) for c, n in enumerate((gx, gy, gz))]
    zz, yy, xx = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    pts = torch.stack([xx, yy, zz], -1).reshape(-1, 1, 3)
    net = scene.fine if scene.fine is not None else scene.coarse
    rows = []
    with torch.no_grad():
        for s in range(0, pts.shape[0], chunk):
            p = pts[s:s + chunk]
            rows.append(O.query_network(p, None, torch.zeros(p.shape[0], 0, dtype=dtype), net, None, scene.cfg)[..., :4])
    return torch.cat(rows, 0).reshape(gz, gy, gx, 4)
