"""GPU tier of the iso-surface extraction: ``field.isosurface`` (nrnerf_isosurface_count / _emit), ``field.extract_mesh``.

1. the three fields of tests/test_isosurface_host.py through the kernels: faces EQUAL to the numpy restatement (tests/mesh_reference.py),
   vertices within one fp32 ulp, normals at the suite's fp32 tolerance; the sphere's properties on the device result itself;
2. shapes at which indexing and the scans can go wrong; 3. NaN; 4. capacities below the totals, and the same bytes twice;
5. ``extract_mesh`` on the synthetic scene.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import _lib, field as F
from nonrigid_nerf_amd import render as R
from nonrigid_nerf_amd.synthetic import Scene, SceneConfig, build_modules, make_scene
from tests import mesh_reference as M
from tests.helpers import TOL, compare_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def on_device(value):
    return torch.from_numpy(np.ascontiguousarray(value)).to(DEV)


def vertex_bound(ref, lo, hi):
    """One fp32 ulp of each coordinate's magnitude (the same double formula, rounded once: half an ulp, and the other half for a product the
    device contracts into an FMA), plus the float64 noise of that formula at the box's scale for a coordinate that happens to land near 0."""
    scale = float(np.abs(np.asarray(lo, np.float64)).max() + np.abs(np.asarray(hi, np.float64)).max())
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -50 * scale


def check_against_restatement(value, level, lo, hi, label):
    got = F.isosurface(on_device(value), level, lo, hi)
    ref = M.marching_tetrahedra(value, level, lo, hi)
    v, f, n = got["vertices"].cpu().numpy(), got["faces"].cpu().numpy(), got["normals"].cpu().numpy()
    assert v.dtype == np.float32 and f.dtype == np.int32 and n.dtype == np.float32
    assert v.shape == ref["vertices"].shape and f.shape == ref["faces"].shape and n.shape == v.shape, (v.shape, f.shape, ref["faces"].shape)
    assert np.array_equal(f, ref["faces"])
    err = np.abs(v.astype(np.float64) - ref["vertices"])
    bound = vertex_bound(ref["vertices"], lo, hi)
    worst = float((err / np.maximum(2.0 ** -23 * np.abs(ref["vertices"]), 1e-300)).max()) if err.size else 0.0
    print(f"[{label}] {v.shape[0]} vertices, {f.shape[0]} triangles; worst vertex error {worst:.3f} ulp")
    assert (err <= bound).all(), float((err - bound).max())
    fails = compare_dict({"normals": got["normals"]}, {"normals": torch.from_numpy(ref["normals"])})
    assert not fails, "\n".join(fails)
    return got, ref


# ---- 1. the three fields ----------------------------------------------------------------------------------------------------------------------------
def test_sphere_on_the_device():
    value, level, lo, hi = M.sphere_field()
    got, _ = check_against_restatement(value, level, lo, hi, "sphere 25^3")
    v, f = got["vertices"].cpu().numpy().astype(np.float64), got["faces"].cpu().numpy()
    assert v.shape == (5666, 3) and f.shape == (11328, 3)
    assert int(M.directed_edge_counts(f)[1].max()) == 1 and M.unmatched_edges(f)[1].shape[0] == 0
    assert M.euler_characteristic(v.shape[0], f) == 2
    assert float(np.linalg.norm(M.triangle_normals(v, f), axis=1).min()) > 0.0
    vol = M.signed_volume(v, f)
    print(f"[sphere 25^3, device] enclosed volume {vol:.2f} (bounds {M.SPHERE_VOLUME_BOUNDS[0]:.2f} .. {M.SPHERE_VOLUME_BOUNDS[1]:.2f})")
    assert M.SPHERE_VOLUME_BOUNDS[0] <= vol <= M.SPHERE_VOLUME_BOUNDS[1]


def test_plane_on_the_device():
    value, level, lo, hi = M.plane_field()
    got, _ = check_against_restatement(value, level, lo, hi, "plane 9x7x6")
    v, f = got["vertices"].cpu().numpy().astype(np.float64), got["faces"].cpu().numpy()
    assert v.shape == (217, 3) and f.shape == (368, 3)
    assert float(np.abs(v @ np.array([1.0, 2.0, 4.0]) - 10.5).max()) <= 2 * 2.0 ** -23 * float(np.abs(v).max())
    assert float((M.triangle_normals(v, f) @ np.array([1.0, 2.0, 4.0])).max()) < 0.0


def test_random_field_on_the_device():
    value, level, lo, hi = M.random_field()
    got, _ = check_against_restatement(value, level, lo, hi, "random 8x7x6")
    v, f = got["vertices"].cpu().numpy().astype(np.float64), got["faces"].cpu().numpy()
    duplicated, open_edges = M.unmatched_edges(f)
    assert duplicated == 0 and bool(M.on_box_face(v, open_edges, lo, hi).all())


# ---- 2. shapes ------------------------------------------------------------------------------------------------------------------------------------
# (70, 3, 2): an x-row that is no multiple of the wave or the block; (3, 2, 300): rows much shorter than a wave; (37, 5, 3): odd everything
@pytest.mark.parametrize("g", [(2, 2, 2), (37, 5, 3), (70, 3, 2), (3, 2, 300)], ids=lambda g: "x".join(map(str, g)))
def test_small_and_ragged_grids(g):
    value, level, lo, hi = M.random_field(g, seed=sum(g))
    check_against_restatement(value, level, lo, hi, "random " + "x".join(map(str, g)))


@pytest.mark.parametrize("g", [(1, 4, 4), (4, 1, 4), (4, 4, 1)], ids=lambda g: "x".join(map(str, g)))
def test_a_grid_without_cells_is_an_empty_mesh(g):
    value, level, lo, hi = M.random_field(g)
    got = F.isosurface(on_device(value), level, lo, hi)
    assert tuple(got["vertices"].shape) == (0, 3) and tuple(got["faces"].shape) == (0, 3) and tuple(got["normals"].shape) == (0, 3)


def _sphere(g, radius):
    gx, gy, gz = g
    z, y, x = np.meshgrid(np.arange(gz, dtype=np.float64), np.arange(gy, dtype=np.float64), np.arange(gx, dtype=np.float64), indexing="ij")
    c = [(n - 1) // 2 for n in g]
    v = radius ** 2 - ((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    return v.astype(np.float32), -0.5, (0.0, 0.0, 0.0), (gx - 1.0, gy - 1.0, gz - 1.0)


# (45, 41, 43): 310 blocks of 256 vertices -- more than one wave of block sums in the scan workgroup; (102, 102, 101): 4105 blocks, more than
# the ISO_SCAN_CHUNK = 4096 block sums the scan workgroup takes at once (the carry into a second chunk).  There is no further level below 2^30.
@pytest.mark.parametrize("g,radius", [((45, 41, 43), 17.0), ((102, 102, 101), 40.0)], ids=["45x41x43", "102x102x101"])
def test_more_blocks_than_the_scan_takes_at_once(g, radius):
    assert (g[0] * g[1] * g[2] + _lib.ISO_BLOCK - 1) // _lib.ISO_BLOCK > (64 if g[0] == 45 else _lib.ISO_SCAN_CHUNK)
    value, level, lo, hi = _sphere(g, radius)
    got = F.isosurface(on_device(value), level, lo, hi)
    ref = M.marching_tetrahedra(value, level, lo, hi, normals=False)
    v, f = got["vertices"].cpu().numpy().astype(np.float64), got["faces"].cpu().numpy()
    assert v.shape == ref["vertices"].shape and f.shape == ref["faces"].shape
    assert int(f.min()) == 0 and int(f.max()) == v.shape[0] - 1
    assert int(M.directed_edge_counts(f)[1].max()) == 1 and M.unmatched_edges(f)[1].shape[0] == 0
    assert M.euler_characteristic(v.shape[0], f) == 2
    vol = M.signed_volume(v, f)
    assert 4.0 / 3.0 * np.pi * (radius ** 2 - 0.25) ** 1.5 <= vol <= 4.0 / 3.0 * np.pi * (radius ** 2 + 0.5) ** 1.5      # as the 25^3 sphere's


def test_all_outside_and_all_inside_are_empty():
    value, _, lo, hi = M.random_field((37, 5, 3))
    for level in (100.0, -100.0):
        got = F.isosurface(on_device(value), level, lo, hi)
        assert tuple(got["vertices"].shape) == (0, 3) and tuple(got["faces"].shape) == (0, 3)


# ---- 3. NaN -----------------------------------------------------------------------------------------------------------------------------------------
def test_nan_is_outside_and_the_mesh_stays_finite():
    value, level, lo, hi = M.random_field((8, 7, 6))
    value[1, 2, 3] = value[0, 0, 0] = value[5, 6, 7] = value[2, 3, 3] = np.nan
    value[4, 4, 4] = np.inf
    got, _ = check_against_restatement(value, level, lo, hi, "random 8x7x6 with NaN")
    assert bool(torch.isfinite(got["vertices"]).all()) and bool(torch.isfinite(got["normals"]).all())


# ---- 4. capacities and determinism ----------------------------------------------------------------------------------------------------------------------
def _raw_calls(value, level, lo, hi, short_by, guard=4096):
    """count + emit through the C ABI with capacities `short_by` below the totals and a guard region behind every output."""
    vol = on_device(value)
    gz, gy, gx = vol.shape
    lib = _lib.load()
    a = _lib.IsosurfaceArgs()
    a.struct_size = C.sizeof(_lib.IsosurfaceArgs)
    a.value, a.gx, a.gy, a.gz, a.level = vol.data_ptr(), gx, gy, gz, level
    a.min_point[:], a.max_point[:] = lo, hi
    need = lib.nrnerf_isosurface_workspace_bytes(gx, gy, gz)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    totals = torch.empty(2, dtype=torch.int64, device=DEV)
    a.workspace, a.workspace_bytes, a.totals = ws.data_ptr(), need, totals.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.nrnerf_isosurface_count(C.byref(a), stream) == _lib.OK
    n_v, n_t = totals.tolist()
    verts = torch.full(((n_v + guard) * 3,), -7.0, dtype=torch.float32, device=DEV)
    norms = torch.full(((n_v + guard) * 3,), -7.0, dtype=torch.float32, device=DEV)
    faces = torch.full(((n_t + guard) * 3,), -7, dtype=torch.int32, device=DEV)
    a.vertices, a.normals, a.faces = verts.data_ptr(), norms.data_ptr(), faces.data_ptr()
    a.n_vertices, a.n_triangles = n_v - short_by, n_t - short_by
    status = lib.nrnerf_isosurface_emit(C.byref(a), stream)
    torch.cuda.synchronize()
    return status, n_v, n_t, verts, norms, faces


def test_capacities_below_the_totals_write_the_prefix_and_nothing_else():
    value, level, lo, hi = M.random_field((37, 5, 3), seed=45)
    status, n_v, n_t, verts, norms, faces = _raw_calls(value, level, lo, hi, short_by=0)
    assert status == _lib.OK and n_v > 1 and n_t > 1
    s_status, s_v, s_t, s_verts, s_norms, s_faces = _raw_calls(value, level, lo, hi, short_by=1)
    assert s_status == _lib.OK and (s_v, s_t) == (n_v, n_t)         # pinned: OK, with the prefix of both arrays written
    for full, short, n in ((verts, s_verts, n_v), (norms, s_norms, n_v), (faces, s_faces, n_t)):
        assert torch.equal(short[:(n - 1) * 3], full[:(n - 1) * 3])
        assert bool((short[(n - 1) * 3:] == -7).all())              # the last element and the guard region behind it: untouched
        assert bool((full[n * 3:] == -7).all())


def test_two_runs_give_identical_bytes():
    value, level, lo, hi = _sphere((45, 41, 43), 17.0)
    vol = on_device(value)
    a, b = F.isosurface(vol, level, lo, hi), F.isosurface(vol, level, lo, hi)
    for k in ("vertices", "faces", "normals"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


# ---- 5. extract_mesh on the synthetic scene ---------------------------------------------------------------------------------------------------------
LO, HI, RES = (-0.8, -0.7, -0.9), (0.9, 0.6, 0.8), (24, 20, 17)
_built = {}


def modules(cfg_kw, seed=3):
    """(cfg, scene, coarse network) of a configuration, built once per module (the handle cache keys on the network object)."""
    key = (tuple(sorted(cfg_kw.items())), seed)
    if key not in _built:
        cfg = SceneConfig(**cfg_kw)
        scene = make_scene(cfg, seed)
        rb, coarse, _ = build_modules(scene, device=DEV)
        for m in (rb, coarse):
            if m is not None:
                m.requires_grad_(False)
        _built[key] = (cfg, scene, coarse)
    return _built[key]


def code_of(cfg):
    return (torch.randn(cfg.latent_size, generator=torch.Generator().manual_seed(9)) * 0.5).to(DEV)


def level_between(sigma):
    lo, hi = float(sigma.min()), float(sigma.max())
    assert hi > lo
    return lo + 0.25 * (hi - lo)


def same_mesh(a, b, keys=("vertices", "faces", "normals")):
    return all(torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("family", ["default", "no_bender"])
def test_extract_mesh_is_sample_grid_isosurface_and_query_points(family):
    cfg, scene, net = modules({"default": dict(N_importance=0), "no_bender": dict(N_importance=0, ray_bending=False)}[family])
    kw, code = {"network_fn": net, "network_fine": None}, code_of(cfg)
    grid = F.sample_grid(kw, code, LO, HI, RES, precision="f32")
    level = level_between(grid["sigma"])
    mesh = F.extract_mesh(kw, code, level, LO, HI, RES, precision="f32")
    assert same_mesh(mesh, F.isosurface(grid["sigma"], level, LO, HI))
    n_v = int(mesh["vertices"].shape[0])
    assert n_v > 0 and int(mesh["faces"].shape[0]) > 0
    raw, det = R.query_points(mesh["vertices"], net, code.reshape(1, -1), detailed_output=True, precision="f32")
    assert mesh["rgb"].dtype == torch.uint8 and torch.equal(mesh["rgb"], F.field_from_raw(raw)[1])
    if cfg.ray_bending:
        assert mesh["rigidity"].dtype == torch.float32 and torch.equal(mesh["rigidity"], det["rigidity_mask"].reshape(n_v))
    else:
        assert "rigidity" not in mesh
    bare = F.extract_mesh(kw, code, level, LO, HI, RES, precision="f32", colors=False, rigidity=False)
    assert set(bare) == {"vertices", "faces", "normals"} and same_mesh(bare, mesh)
    # closed away from the box
    duplicated, open_edges = M.unmatched_edges(mesh["faces"].cpu().numpy())
    assert duplicated == 0 and bool(M.on_box_face(mesh["vertices"].cpu().numpy(), open_edges, LO, HI).all())


def test_extract_mesh_without_bending_is_the_bender_free_models_mesh():
    cfg, scene, net = modules(dict(N_importance=0))
    plain_scene = Scene(SceneConfig(N_importance=0, ray_bending=False), None, scene.coarse, None)
    _, plain, _ = build_modules(plain_scene, device=DEV)
    plain.requires_grad_(False)
    level = level_between(F.sample_grid({"network_fn": plain}, None, LO, HI, RES, precision="f32")["sigma"])
    got = F.extract_mesh({"network_fn": net}, None, level, LO, HI, RES, with_bending=False, precision="f32")
    want = F.extract_mesh({"network_fn": plain}, None, level, LO, HI, RES, precision="f32")
    assert set(got) == set(want) == {"vertices", "faces", "normals", "rgb"}
    assert int(got["vertices"].shape[0]) > 0 and same_mesh(got, want, ("vertices", "faces", "normals", "rgb"))
    bent = F.extract_mesh({"network_fn": net}, code_of(cfg), level, LO, HI, RES, precision="f32", colors=False, rigidity=False)
    assert bent["vertices"].shape != got["vertices"].shape or not torch.equal(bent["vertices"], got["vertices"])


@pytest.mark.parametrize("bender", [False, True], ids=["no_bender", "bender"])
def test_a_view_dependent_head_is_seen_along_minus_the_normal(bender):
    cfg, scene, net = modules(dict(N_importance=0, use_viewdirs=True, ray_bending=bender))
    kw, code = {"network_fn": net, "network_fine": None}, code_of(cfg)
    level = level_between(F.sample_grid(kw, code, LO, HI, RES, precision="f32")["sigma"])
    mesh = F.extract_mesh(kw, code, level, LO, HI, RES, precision="f32")
    v, n = mesh["vertices"], mesh["normals"]
    n_v = int(v.shape[0])
    assert n_v > 0
    lat = code.reshape(1, -1).expand(n_v, -1)
    if bender:
        h = F.vertex_probe_step(LO, HI, RES)
        step = [(HI[c] - LO[c]) / (RES[c] - 1) for c in range(3)]
        assert abs(h - sum(s * s for s in step) ** 0.5) <= 1e-6 * h            # one cell diagonal
        raw, det = R.query_points(torch.stack([v + h * n, v], 1), net, lat, None, detailed_output=True, precision="f32")
        assert torch.equal(mesh["rgb"], F.field_from_raw(raw[:, 1].contiguous())[1])
        assert torch.equal(mesh["rigidity"], det["rigidity_mask"][:, 1].reshape(n_v))
    else:
        raw = R.query_points(v.reshape(n_v, 1, 3), net, None, -n, precision="f32")
        assert torch.equal(mesh["rgb"], F.field_from_raw(raw[:, 0].contiguous())[1])
        other = R.query_points(v.reshape(n_v, 1, 3), net, None, n, precision="f32")          # the direction matters
        assert not torch.equal(raw[..., :3], other[..., :3])


@pytest.mark.parametrize("case", ["exact_jacobian", "odd_bender"])
def test_what_no_point_query_takes_gives_its_geometry_alone(case):
    """The cases of tests/test_query.py::test_what_the_library_cannot_take_is_handed_over: attributes raise Unsupported, the geometry comes
    from the renderer's kernels (density_along_rows).  That route, on a model sample_grid DOES take, gives sample_grid's density up to the
    rounding of its sample positions: checked first, at the fp32 tolerance of `raw` on the density's scale."""
    cfg_kw = {"exact_jacobian": dict(N_importance=0, use_viewdirs=True, approx_nonrigid_viewdirs=False), "odd_bender": dict(N_importance=0, bend_hidden=96)}[case]
    cfg, scene, net = modules(cfg_kw)
    kw, code = {"network_fn": net, "network_fine": None}, code_of(cfg)
    with pytest.raises(R.Unsupported):
        F.extract_mesh(kw, code, 1.0, LO, HI, RES, precision="f32")
    with pytest.raises(R.Unsupported):
        F.extract_mesh(kw, code, 1.0, LO, HI, RES, precision="f32", colors=False)            # rigidity is still asked for
    sigma = F.density_along_rows(kw, code, LO, HI, RES, precision="f32")
    assert tuple(sigma.shape) == (17, 20, 24)
    level = level_between(sigma)
    mesh = F.extract_mesh(kw, code, level, LO, HI, RES, precision="f32", colors=False, rigidity=False)
    assert set(mesh) == {"vertices", "faces", "normals"} and int(mesh["vertices"].shape[0]) > 0
    assert same_mesh(mesh, F.isosurface(sigma, level, LO, HI))


def test_density_along_rows_is_sample_grids_density():
    cfg, scene, net = modules(dict(N_importance=0))
    kw, code = {"network_fn": net, "network_fine": None}, code_of(cfg)
    want = F.sample_grid(kw, code, LO, HI, RES, precision="f32")["sigma"]
    got = F.density_along_rows(kw, code, LO, HI, RES, precision="f32")
    # the sample positions differ by a rounding in x (o + d * t in fp32 against the grid's double formula): the tolerance of `raw` -- 1e-4 of the
    # tensor's scale -- plus the density's slope over that rounding, which the same bound covers on this scene (printed)
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"[density along rows] max |sigma - sample_grid's| = {err:.3e} (scale {scale:.3e})")
    assert err <= TOL["raw"]["scale_atol"] * scale


def test_extract_mesh_in_bf16_is_closed_and_carries_its_attributes():
    cfg, scene, net = modules(dict(N_importance=0))
    kw, code = {"network_fn": net, "network_fine": None}, code_of(cfg)
    level = level_between(F.sample_grid(kw, code, LO, HI, RES, precision="bf16")["sigma"])
    mesh = F.extract_mesh(kw, code, level, LO, HI, RES, precision="bf16")
    n_v, n_t = int(mesh["vertices"].shape[0]), int(mesh["faces"].shape[0])
    assert n_v > 0 and n_t > 0
    assert tuple(mesh["normals"].shape) == (n_v, 3) and tuple(mesh["rgb"].shape) == (n_v, 3) and tuple(mesh["rigidity"].shape) == (n_v,)
    assert mesh["rgb"].dtype == torch.uint8 and mesh["faces"].dtype == torch.int32
    duplicated, open_edges = M.unmatched_edges(mesh["faces"].cpu().numpy())
    assert duplicated == 0 and bool(M.on_box_face(mesh["vertices"].cpu().numpy(), open_edges, LO, HI).all())
