"""A numpy float64 restatement of the iso-surface definitions (nonrigid_nerf_amd/csrc/nrnerf_isosurface.h), and the
mesh properties the tests state.  Not code under test: written from the header's TEXT -- the permutations, the owner / slot rule and the
sixteen cases as printed there -- vectorised over the cells that the surface crosses.
"""
from __future__ import annotations

import itertools

import numpy as np

# six tetrahedra, one per permutation of the axes in lexicographic order; local corners 0, e_p1, e_p1 + e_p2, 7; odd permutations are
# negatively oriented
PERMUTATIONS = list(itertools.permutations(range(3)))
TETRAHEDRA = [(0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7) for p in PERMUTATIONS]
ODD = [sum(p[i] > p[j] for i in range(3) for j in range(i + 1, 3)) % 2 == 1 for p in PERMUTATIONS]

# THE SIXTEEN CASES of a positively oriented tetrahedron, as the header prints them: mask m (bit k = local corner k inside) -> triangles,
# each vertex the tetrahedron edge "ij" of local corners i, j
_E = lambda s: tuple(tuple(int(ch) for ch in v) for v in s.split())
CASES = {
    0: [], 15: [],
    1: [_E("01 02 03")], 14: [_E("01 03 02")],
    2: [_E("01 13 12")], 13: [_E("01 12 13")],
    3: [_E("02 03 13"), _E("02 13 12")], 12: [_E("02 13 03"), _E("02 12 13")],
    4: [_E("02 12 23")], 11: [_E("02 23 12")],
    5: [_E("01 12 23"), _E("01 23 03")], 10: [_E("01 23 12"), _E("01 03 23")],
    6: [_E("01 13 23"), _E("01 23 02")], 9: [_E("01 23 13"), _E("01 02 23")],
    7: [_E("03 13 23")], 8: [_E("03 23 13")],
}


def grid_steps(lo, hi, g):
    """(lo, step) per axis in float64 from the float32 box, as grid_points_kernel computes them."""
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64)
    hi = np.asarray(hi, dtype=np.float32).astype(np.float64)
    return lo, np.array([(hi[c] - lo[c]) / (g[c] - 1) if g[c] > 1 else 0.0 for c in range(3)])


def _gradient(v64, steps):
    """grad value on the grid [gz, gy, gx, 3] (x, y, z): central differences, one-sided at the box faces, an axis with step 0 contributes 0."""
    out = np.zeros(v64.shape + (3,))
    for c, axis in enumerate((2, 1, 0)):
        if steps[c] == 0.0 or v64.shape[axis] < 2:
            continue
        f = np.moveaxis(v64, axis, 0)
        d = np.empty_like(f)
        d[1:-1] = (f[2:] - f[:-2]) / (2.0 * steps[c])
        d[0] = (f[1] - f[0]) / steps[c]
        d[-1] = (f[-1] - f[-2]) / steps[c]
        out[..., c] = np.moveaxis(d, 0, axis)
    return out


def marching_tetrahedra(value, level, lo, hi, normals=True):
    """``value`` float32 [gz, gy, gx] -> {"vertices": float64 [V, 3] (before the one rounding to fp32), "faces": int64 [F, 3],
    "normals": float64 [V, 3]} in the stated orders."""
    value = np.asarray(value, dtype=np.float32)
    gz, gy, gx = value.shape
    g = (gx, gy, gz)
    empty = {"vertices": np.zeros((0, 3)), "faces": np.zeros((0, 3), dtype=np.int64), "normals": np.zeros((0, 3))}
    if min(g) < 2:
        return empty
    level = np.float64(np.float32(level))
    v64 = value.astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = value >= np.float32(level)                       # NaN: outside
    lo64, steps = grid_steps(lo, hi, g)

    # active owned edges: [gz, gy, gx, 7]; slot s joins the vertex with the one at + (dx, dy, dz), d = s + 1 = dx + 2 dy + 4 dz
    active = np.zeros((gz, gy, gx, 7), dtype=bool)
    for s in range(7):
        dx, dy, dz = (s + 1) & 1, ((s + 1) >> 1) & 1, ((s + 1) >> 2) & 1
        a = inside[:gz - dz, :gy - dy, :gx - dx]
        b = inside[dz:, dy:, dx:]
        active[:gz - dz, :gy - dy, :gx - dx, s] = a != b
    vertex_id = (np.cumsum(active.reshape(-1)) - 1).reshape(active.shape)           # ascending (owner linear index, slot)
    iz, iy, ix, slot = np.nonzero(active)
    d = slot + 1
    dirs = np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], -1)
    fa, fb = v64[iz, iy, ix], v64[iz + dirs[:, 2], iy + dirs[:, 1], ix + dirs[:, 0]]
    with np.errstate(all="ignore"):
        t = (level - fa) / (fb - fa)
    t = np.where(np.isfinite(t), np.clip(t, 0.0, 1.0), 0.5)
    index = np.stack([ix, iy, iz], -1).astype(np.float64)
    out = {"vertices": lo64 + (index + t[:, None] * dirs) * steps}
    if normals:
        grad = _gradient(v64, steps)
        with np.errstate(all="ignore"):
            ga, gb = grad[iz, iy, ix], grad[iz + dirs[:, 2], iy + dirs[:, 1], ix + dirs[:, 0]]
            gv = ga + t[:, None] * (gb - ga)
            length = np.sqrt((gv * gv).sum(-1))
            ok = np.isfinite(length) & (length > 0.0)
            out["normals"] = np.where(ok[:, None], -gv / np.where(ok, length, 1.0)[:, None], 0.0)

    # the cells the surface crosses, ascending by linear index of their minimum corner
    corner = [inside[(c >> 2) & 1:gz - 1 + ((c >> 2) & 1), (c >> 1) & 1:gy - 1 + ((c >> 1) & 1), (c & 1):gx - 1 + (c & 1)] for c in range(8)]
    mixed = np.zeros_like(corner[0])
    for c in range(1, 8):
        mixed |= corner[c] != corner[0]
    cz, cy, cx = np.nonzero(mixed)
    bits = [corner[c][cz, cy, cx] for c in range(8)]
    faces = np.full((cz.size, 6, 2, 3), -1, dtype=np.int64)
    for ti, tet in enumerate(TETRAHEDRA):
        m = sum(bits[tet[k]].astype(np.int64) << k for k in range(4))
        for case, triangles in CASES.items():
            sel = np.nonzero(m == case)[0]
            if sel.size == 0:
                continue
            for k, tri in enumerate(triangles):
                if ODD[ti]:
                    tri = (tri[0], tri[2], tri[1])
                for j, (li, lj) in enumerate(tri):
                    a, b = tet[li], tet[lj]
                    assert a & b == a and a != b
                    s = (b & ~a) - 1
                    faces[sel, ti, k, j] = vertex_id[cz[sel] + ((a >> 2) & 1), cy[sel] + ((a >> 1) & 1), cx[sel] + (a & 1), s]
    faces = faces.reshape(-1, 3)
    out["faces"] = faces[faces[:, 0] >= 0]                        # ascending (cell, tetrahedron, triangle)
    return out


# ---- properties ------------------------------------------------------------------------------------------------------------------------------
def directed_edge_counts(faces):
    """(edges [E, 2], counts [E]) of the DIRECTED edges (v0 v1), (v1 v2), (v2 v0) of every triangle."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    if e.size == 0:
        return e, np.zeros(0, dtype=np.int64)
    span = int(e.max()) + 1
    code, counts = np.unique(e[:, 0] * span + e[:, 1], return_counts=True)
    return np.stack([code // span, code % span], -1), counts


def unmatched_edges(faces):
    """(number of directed edges that occur more than once, the directed edges [U, 2] whose reverse does not occur)."""
    e, n = directed_edge_counts(faces)
    if e.size == 0:
        return 0, e
    span = int(e.max()) + 1
    code, rev = e[:, 0] * span + e[:, 1], e[:, 1] * span + e[:, 0]
    return int((n > 1).sum()), e[~np.isin(rev, code)]


def euler_characteristic(n_vertices, faces):
    e, _ = directed_edge_counts(faces)
    span = int(e.max()) + 1 if e.size else 1
    undirected = np.unique(e.min(1) * span + e.max(1)).size if e.size else 0
    return int(n_vertices) - undirected + int(np.asarray(faces).reshape(-1, 3).shape[0])


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def triangle_normals(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def on_box_face(vertices, edges, lo, hi, atol=1e-6):
    """per edge: both ends lie in one face of the box."""
    v = np.asarray(vertices, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    a, b = v[edges[:, 0]], v[edges[:, 1]]
    at_lo = (np.abs(a - lo) <= atol) & (np.abs(b - lo) <= atol)
    at_hi = (np.abs(a - hi) <= atol) & (np.abs(b - hi) <= atol)
    return (at_lo | at_hi).any(-1)


# ---- the three fields of the tests --------------------------------------------------------------------------------------------------------------
def sphere_field(n=25, centre=12.0, radius_sq=100.0):
    """100 - |p - (12, 12, 12)|^2 on the integer points of a 25^3 grid: exact in fp32.  -> (value, level, lo, hi)"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    v = radius_sq - ((x - centre) ** 2 + (y - centre) ** 2 + (z - centre) ** 2)
    return v.astype(np.float32), -0.5, (0.0, 0.0, 0.0), (n - 1.0,) * 3


def plane_field():
    """x + 2 y + 4 z on a 9 x 7 x 6 integer grid, level 10.5."""
    z, y, x = np.meshgrid(np.arange(6.0), np.arange(7.0), np.arange(9.0), indexing="ij")
    return (x + 2 * y + 4 * z).astype(np.float32), 10.5, (0.0, 0.0, 0.0), (8.0, 6.0, 5.0)


def random_field(g=(8, 7, 6), seed=0, lo=(-1.25, 0.3, -2.0), hi=(0.75, 1.9, 3.5)):
    """standard normal values on a gx x gy x gz grid over a box that is not the index box, level 0.1."""
    v = np.random.default_rng(seed).standard_normal((g[2], g[1], g[0])).astype(np.float32)
    return v, 0.1, lo, hi


SPHERE_VOLUME_BOUNDS = (4.0 / 3.0 * np.pi * 99.75 ** 1.5, 4.0 / 3.0 * np.pi * 100.5 ** 1.5)
