"""Occupancy masks (include/nrnerf.h, "occupancy masks") stated in numpy / float64: the mask rule, and the baked renders'
references (tests/volume_reference.py, warp_reference.py, sh_reference.py -- imported, not edited) with a mask applied: a sample whose cell
lies in an empty block is an empty sample (raw = 0, v = 0)."""
import numpy as np
import torch

from tests import sh_reference as SH
from tests import volume_reference as V
from tests import warp_reference as W


def blocks(g, block):
    """Blocks per axis of ``g`` vertices (``g - 1`` cells)."""
    return -(-(g - 1) // block)


def mask_reference(vol, block, threshold=0.0):
    """``vol [Gz, Gy, Gx, 4]`` (any float dtype: widened to float32 first, as the kernel widens half) -> the boolean block grid
    ``[nbz, nby, nbx]``: a block is occupied iff some vertex of ``b * block .. min(b * block + block, g - 1)`` per axis has a sigma logit that is
    not ``<= threshold`` (NaN: occupied) or any channel that is not finite."""
    v = np.asarray(vol.detach().cpu().to(torch.float32) if torch.is_tensor(vol) else vol, dtype=np.float32)
    gz, gy, gx = v.shape[:3]
    thr = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        vertex = ~(v[..., 3] <= thr) | ~np.isfinite(v).all(-1)
    nbz, nby, nbx = blocks(gz, block), blocks(gy, block), blocks(gx, block)
    occ = np.zeros((nbz, nby, nbx), dtype=bool)
    for bz in range(nbz):
        for by in range(nby):
            for bx in range(nbx):
                occ[bz, by, bx] = vertex[bz * block:min(bz * block + block, gz - 1) + 1, by * block:min(by * block + block, gy - 1) + 1,
                                         bx * block:min(bx * block + block, gx - 1) + 1].any()
    return occ


def pack_bits(occ):
    """The block grid -> the int32 words: bit ``(bz * nby + by) * nbx + bx``, word ``index >> 5``, bit ``index & 31``, unused high bits zero."""
    flat = occ.reshape(-1).astype(np.uint64)
    words = np.zeros((flat.size + 31) // 32, dtype=np.uint64)
    idx = np.arange(flat.size)
    np.add.at(words, idx >> 5, flat << (idx & 31).astype(np.uint64))
    return words.astype(np.uint32).view(np.int32)


def unpack_bits(words, shape):
    w = np.asarray(words).view(np.uint32)
    idx = np.arange(int(np.prod(shape)))
    return ((w[idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool).reshape(shape)


def sample_state(occ, block, g, min_point, max_point, pts, dtype=torch.float64):
    """Per point of ``pts [..., 3]``: ``(inside the box, in an occupied block)`` by THE VALUE AT A POINT's cell in ``dtype`` (the cell rule of
    ``volume_reference.lookup_reference``); ``g = (gx, gy, gz)``."""
    lo = torch.as_tensor(np.asarray(min_point, dtype=np.float32)).to(dtype)
    hi = torch.as_tensor(np.asarray(max_point, dtype=np.float32)).to(dtype)
    top = torch.tensor([g[0] - 1, g[1] - 1, g[2] - 1], dtype=dtype)
    p = pts.detach().cpu().to(dtype)
    q = (p - lo) * (top / (hi - lo))
    inside = ((q >= 0) & (q <= top)).all(-1)
    gs = torch.where(inside[..., None], q, torch.zeros_like(q))
    i = torch.minimum(torch.floor(gs), top - 1).to(torch.int64)
    k = int(block).bit_length() - 1
    b = i >> k
    hit = torch.from_numpy(np.ascontiguousarray(occ))[b[..., 2], b[..., 1], b[..., 0]]
    return inside, hit


def render_reference(vol, sh, degree, min_point, max_point, rays, z_vals, *, occ, block, warp=None, warp_min=None, warp_max=None, points4=None,
                     ray_directions=None, white_bkgd=False, rigidity_cutoff=None, test_time_scaling=None, removal_threshold=None,
                     dtype=torch.float64):
    """What nrnerf_culled_volume_render computes, in ``dtype``: ``sh_reference.render_reference`` (``degree`` 0 with ``sh=None``: the volume /
    warp references' rule) where a sample in an empty block of ``occ`` is an empty sample.  Adds ``inside`` and ``occupied`` ``[N, S]``: whether
    the sample's bent point is in the box, and whether its block is occupied."""
    r, z = rays.detach().cpu().to(dtype), z_vals.detach().cpu().to(dtype)
    pts = W.sample_points(rays, z_vals, dtype)
    if warp is not None:
        p4 = W.bend_reference(warp, warp_min, warp_max, pts, rigidity_cutoff=rigidity_cutoff, test_time_scaling=test_time_scaling, dtype=dtype)
    elif points4 is not None:
        p4 = points4.detach().cpu().to(dtype)
    else:
        p4 = torch.cat([pts, torch.zeros_like(pts[..., :1])], -1)
    gz, gy, gx = vol.shape[:3]
    inside, hit = sample_state(occ, block, (gx, gy, gz), min_point, max_point, p4[..., :3], dtype)
    raw = V.lookup_reference(vol, min_point, max_point, p4[..., :3], dtype).clone()
    raw = torch.where(hit[..., None], raw, torch.zeros_like(raw))
    d = None
    if degree:
        if ray_directions is None:
            ray_directions = warp is None and points4 is None
        d = SH.directions(p4, rays, ray_directions, dtype)            # (from the bent points, masked or not)
        v = SH.lookup_channels(sh, min_point, max_point, p4[..., :3], dtype)
        v = torch.where(hit[..., None], v, torch.zeros_like(v))
        Y = SH.basis(d, degree, dtype)
        for k in range(1, (degree + 1) ** 2):
            for c in range(3):
                raw[..., c] = raw[..., c] + Y[..., k] * v[..., 3 * (k - 1) + c]
    if removal_threshold is not None:
        kill = p4[..., 3] >= float(np.float32(removal_threshold))
        raw[..., 3] = torch.where(kill, raw[..., 3] * 0.0, raw[..., 3])
    out = SH.composite_reference(raw, z, r, p4, white_bkgd, dtype)
    out["points4"], out["dirs"], out["inside"], out["occupied"] = p4, d, inside, hit
    return out


def blob_volume(gx, gy, gz, seed=0, centre=(0.5, 0.5, 0.5), radius=0.3, shell=0.08):
    """A seeded volume ``[Gz, Gy, Gx, 4]`` float32 for the exactness tests: sigma logits positive inside a blob (an ellipsoid of ``radius`` of
    the box around ``centre``, in box coordinates), negative outside it, and of MIXED sign in a shell of width ``shell`` between: cells there
    have corners of both signs, and interpolate to either.  Colour logits: smooth waves of a few units, everywhere (an empty cell's colours
    are not zero: skipping it must not show)."""
    g = torch.Generator().manual_seed(seed)
    zz, yy, xx = torch.meshgrid(torch.linspace(0, 1, gz, dtype=torch.float64), torch.linspace(0, 1, gy, dtype=torch.float64),
                                torch.linspace(0, 1, gx, dtype=torch.float64), indexing="ij")
    vol = torch.zeros(gz, gy, gx, 4, dtype=torch.float64)
    for c in range(3):
        for _ in range(3):
            k = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1) * 6.0
            ph, amp = torch.rand(1, generator=g, dtype=torch.float64) * 6.28, torch.rand(1, generator=g, dtype=torch.float64) * 3.0
            vol[..., c] += amp * torch.sin(k[0] * xx + k[1] * yy + k[2] * zz + ph)
    rr = torch.sqrt((xx - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (zz - centre[2]) ** 2)
    noise = torch.rand(gz, gy, gx, generator=g, dtype=torch.float64)
    sigma = torch.where(rr < radius, 1.0 + 6.0 * noise, -(0.5 + 4.0 * noise))
    mixed = (rr - radius).abs() < 0.5 * shell
    sigma = torch.where(mixed, (noise - 0.5) * 6.0, sigma)
    vol[..., 3] = sigma
    return vol.to(torch.float32)
