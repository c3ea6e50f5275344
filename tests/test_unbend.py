"""The inverse of the ray bender on the device: nrnerf_bender_inverse / field.unbend_points / animate_mesh / track_points.

The solver and the point-source fp32 bender of nrnerf_query do the same arithmetic, so the central check is exact: the fp32 query at the
returned point answers a bent point whose distance from the canonical point IS the returned residual, bit for bit.  Accuracy is measured
against the float64 reference solver of tests/unbend_reference.py, with bars taken from the reference's own float32 solve."""
import ctypes as C
import os

import pytest
import torch

from nonrigid_nerf_amd import _lib, field as F
from nonrigid_nerf_amd import render as R
from tests.test_query import _scattered_points, modules, set_knobs
from tests.test_unbend_host import reference_solve
from tests.unbend_reference import cube_points, fitted, unbend_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-6
TOL32 = float(torch.tensor(TOL, dtype=torch.float32))
FAMILIES = {"default": dict(N_importance=0), "deep_bender": dict(N_importance=0, bend_depth=7)}


def codes(n, cfg, seed=9):
    return (torch.randn(n, cfg.latent_size, generator=torch.Generator().manual_seed(seed)) * 0.5).to(DEV)


def bend(points, net, lat):
    """The fp32 point-source bender at ``points``: nrnerf_query's input_pts."""
    return R.query_points(points, net, lat, detailed_output=True, precision="f32")[1]["input_pts"]


def residual_of(points, canonical, net, lat):
    return (bend(points, net, lat) - canonical).abs().max(-1).values


def check_solution(sol, canonical, net, lat, tol=TOL, max_iters=64):
    tol32 = float(torch.tensor(tol, dtype=torch.float32))
    got = residual_of(sol["points"], canonical, net, lat)
    assert torch.equal(got, sol["residual"]), float((got - sol["residual"]).abs().max())
    assert torch.equal(sol["converged"], sol["residual"] <= tol32)
    assert int(sol["iterations"].min()) >= 1 and int(sol["iterations"].max()) <= max_iters
    assert sol["iterations"].dtype == torch.int32 and sol["converged"].dtype == torch.bool


# ---- 1. round trip, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{}, dict(rigidity_test_time_cutoff=0.3, test_time_scaling=0.5)], ids=["plain", "cutoff+scaling"])
@pytest.mark.parametrize("shape", [(37, 33), (3, 5), (1, 1)], ids=["37x33", "3x5", "1x1"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_query_at_the_solution_has_exactly_the_returned_residual(family, shape, knobs):
    cfg, scene, rb, coarse = modules(FAMILIES[family])
    c = _scattered_points(shape[0] * shape[1], seed=7).reshape(*shape, 3)
    lat = codes(shape[0], cfg)
    set_knobs(rb, coarse, knobs)
    try:
        sol = F.unbend_points(coarse, c, lat)
        assert tuple(sol["points"].shape) == (*shape, 3) and tuple(sol["residual"].shape) == shape
        check_solution(sol, c, coarse, lat)
        print(f"[{family} {shape} {knobs}] converged {float(sol['converged'].float().mean()):.3f}, evaluations max {int(sol['iterations'].max())}, "
              f"residual max {float(sol['residual'].max()):.2e}")
        # a few evaluations with a damped step: the residual is still that of the stored point (taken after the last update's evaluation)
        few = F.unbend_points(coarse, c, lat, max_iters=3, relaxation=0.5, tol=0.0)
        check_solution(few, c, coarse, lat, tol=0.0, max_iters=3)
    finally:
        set_knobs(rb, coarse, {})


# ---- 2. against float64, synthetic -------------------------------------------------------------------------------------------------------------
def test_synthetic_solution_against_the_float64_reference():
    cfg, scene, rb, coarse = modules(FAMILIES["default"])
    set_knobs(rb, coarse, {})
    pts = _scattered_points(1008)
    code = codes(1, cfg)
    kw = dict(tol=0.0, max_iters=48)
    ref64 = unbend_reference(pts.cpu().double(), code.cpu(), scene.bender, **kw)
    ref32 = unbend_reference(pts.cpu(), code.cpu(), scene.bender, **kw)
    sol = F.unbend_points(coarse, pts, code, **kw)
    own = float((ref32["points"].double() - ref64["points"]).abs().max())
    got = float((sol["points"].cpu().double() - ref64["points"]).abs().max())
    print(f"[synthetic, tol 0, 48 evaluations] |kernel - float64| max {got:.3e}; reference float32 vs float64 {own:.3e}; "
          f"float64 residual max {float(ref64['residual'].max()):.2e}, kernel residual max {float(sol['residual'].max()):.2e}")
    assert float(ref64["residual"].max()) < 1e-9, "the float64 reference did not converge: the comparison has no meaning"
    assert got <= 10 * own
    check_solution(sol, pts, coarse, code, tol=0.0, max_iters=48)


# ---- 3. against float64, fitted ----------------------------------------------------------------------------------------------------------------
_fitted = {}


def fitted_case(name):
    if name not in _fitted:
        ck, bender, half = fitted(name)
        for m in (ck.ray_bender, ck.network_fn, ck.network_fine):
            if m is not None:
                m.requires_grad_(False)
        _fitted[name] = (ck, cube_points(2000, half, seed=0, dtype=torch.float32).to(DEV), ck.latents[3].reshape(1, -1).to(DEV))
    return _fitted[name]


@pytest.mark.parametrize("name", ["fitted_latest", "fitted_config4"])
def test_fitted_solution_against_the_float64_reference(name):
    ck, pts, code = fitted_case(name)
    sol = F.unbend_points(ck.network_fn, pts, code)
    ref64, ref32 = reference_solve(name), reference_solve(name, dtype=torch.float32)
    conv = sol["converged"].cpu()
    share = float(conv.float().mean())
    both = conv & ref64["converged"]
    bar_set = both & ref32["converged"]
    own = float((ref32["points"].double() - ref64["points"])[bar_set].abs().max())
    got = float((sol["points"].cpu().double() - ref64["points"])[both].abs().max())
    print(f"[{name}] kernel converged {100 * share:.2f} %, compared on {100 * float(both.float().mean()):.2f} %: |kernel - float64| max {got:.3e}; "
          f"reference float32 vs float64 {own:.3e}; evaluations mean {float(sol['iterations'].float().mean()):.2f} max {int(sol['iterations'].max())}")
    assert share >= 0.995
    assert float(both.float().mean()) >= 0.99
    assert got <= 10 * own
    assert bool((sol["iterations"][~sol["converged"]] == 64).all())


# ---- 4. relaxation -----------------------------------------------------------------------------------------------------------------------------
def test_relaxation_converges_where_the_plain_iteration_oscillates():
    ck, pts, code = fitted_case("fitted_latest")
    bender = R._bender_of(ck.network_fn)
    bender.test_time_scaling = 2.0
    try:
        damped = F.unbend_points(ck.network_fn, pts, code, relaxation=0.7)
        plain = F.unbend_points(ck.network_fn, pts, code, relaxation=1.0)
    finally:
        bender.test_time_scaling = None
    n_damped, n_plain = int(damped["converged"].sum()), int(plain["converged"].sum())
    print(f"[fitted_latest, test_time_scaling 2] converged: omega 0.7 {n_damped} / 2000, omega 1 {n_plain} / 2000")
    assert n_damped >= 0.995 * 2000
    assert n_plain < n_damped
    lost = ~plain["converged"]
    assert bool((plain["iterations"][lost] == 64).all()) and bool((plain["residual"][lost] > TOL32).all())


# ---- 5. indexing invariances, bit for bit per point ------------------------------------------------------------------------------------------------
def test_a_points_solution_does_not_depend_on_where_it_sits():
    cfg, scene, rb, coarse = modules(FAMILIES["default"], 3)
    set_knobs(rb, coarse, {})
    pts = _scattered_points(1008)
    code = codes(1, cfg)
    rows = lambda n: code.expand(n, -1).contiguous()          # per-row latents (stride = latent size)
    KEYS = ("points", "residual", "iterations")

    def flat(sol):
        return {k: sol[k].reshape(1008, -1) for k in KEYS}

    def same(a, b, index=None):
        return all(torch.equal(a[k], b[k] if index is None else b[k][index]) for k in KEYS)

    solve = lambda p, lat, **kw: flat(F.unbend_points(coarse, p, lat, **kw))
    base = solve(pts.reshape(1, 1008, 3), rows(1))
    print(f"[1008 scattered points] evaluations min {int(base['iterations'].min())} max {int(base['iterations'].max())}")
    assert same(solve(pts.reshape(63, 16, 3), rows(63)), base)
    assert same(solve(pts.reshape(144, 7, 3), rows(144)), base)
    assert same(solve(pts, code), base)                       # flat: rows of 64, the last one padded
    perm = torch.randperm(1008, generator=torch.Generator().manual_seed(2)).to(DEV)
    assert same(solve(pts[perm].reshape(63, 16, 3), rows(63)), base, perm)
    # one code for the call (latent_stride 0) against per-row latents
    assert same(solve(pts.reshape(63, 16, 3), code.expand(63, -1)), base)
    # point_stride 4 against 3
    model = R.get_model(coarse, None, precision="f32", device=DEV)
    p4 = torch.cat([pts, torch.full((1008, 1), 7.0, device=DEV)], -1).reshape(63, 16, 4)
    x, res, its = model.bender_inverse(p4, rows(63))
    assert same(flat({"points": x, "residual": res, "iterations": its}), base)
    # fixed against dynamic shares; the same call twice; the canonical point as an explicit first guess
    assert same(solve(pts.reshape(63, 16, 3), rows(63), flags=_lib.RENDER_FIXED_SHARES), base)
    assert same(solve(pts.reshape(1, 1008, 3), rows(1)), base)
    assert same(solve(pts.reshape(63, 16, 3), rows(63), initial=pts.reshape(63, 16, 3)), base)


# ---- 6. every wave loops -----------------------------------------------------------------------------------------------------------------------
def test_more_blocks_than_the_grid_has_waves():
    """[4100, 40]: 8200 blocks of 32 points against 4 workgroups x 4 waves x 256 CUs, the second block of every row ragged."""
    cfg, scene, rb, coarse = modules(FAMILIES["default"])
    set_knobs(rb, coarse, {})
    pts = _scattered_points(4100 * 40, seed=6).reshape(4100, 40, 3)
    lat = codes(4100, cfg, seed=4)
    a = F.unbend_points(coarse, pts, lat)
    b = F.unbend_points(coarse, pts, lat)
    fixed = F.unbend_points(coarse, pts, lat, flags=_lib.RENDER_FIXED_SHARES)
    for k in ("points", "residual", "iterations"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], fixed[k]), k
    sub = {k: v[::16].contiguous() for k, v in a.items()}
    check_solution(sub, pts[::16].contiguous(), coarse, lat[::16].contiguous())
    print(f"[4100 x 40] converged {float(a['converged'].float().mean()):.4f}, evaluations mean {float(a['iterations'].float().mean()):.2f}")


# ---- 7. warm start -----------------------------------------------------------------------------------------------------------------------------
def test_a_solution_as_first_guess_is_confirmed_in_one_evaluation():
    cfg, scene, rb, coarse = modules(FAMILIES["default"])
    set_knobs(rb, coarse, {})
    pts = _scattered_points(37 * 33, seed=8).reshape(37, 33, 3)
    lat = codes(37, cfg)
    first = F.unbend_points(coarse, pts, lat)
    again = F.unbend_points(coarse, pts, lat, initial=first["points"])
    done = first["converged"]
    assert bool(done.any())
    assert bool((again["iterations"][done] == 1).all())
    assert torch.equal(again["points"][done], first["points"][done]) and torch.equal(again["residual"][done], first["residual"][done])
    one = F.unbend_points(coarse, pts, lat, initial=first["points"], max_iters=1)
    assert torch.equal(one["points"], first["points"]) and torch.equal(one["residual"], first["residual"])
    assert bool((one["iterations"] == 1).all())
    start = F.unbend_points(coarse, pts, lat, max_iters=1)               # no guess, one evaluation: the canonical point and ITS residual
    assert torch.equal(start["points"], pts) and torch.equal(start["residual"], residual_of(pts, pts, coarse, lat))


# ---- 8. hand-overs and edges -------------------------------------------------------------------------------------------------------------------
def test_what_the_inverse_does_not_take():
    cfg, scene, rb, coarse = modules(FAMILIES["default"])
    pts = _scattered_points(15).reshape(3, 5, 3)
    lat = codes(3, cfg)
    with pytest.raises(_lib.NrnerfError) as e:
        R.get_model(coarse, None, precision="bf16", device=DEV).bender_inverse(pts, lat)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    cfg_o, _, _, odd = modules(dict(N_importance=0, bend_hidden=96))
    with pytest.raises(R.Unsupported):
        F.unbend_points(odd, pts, codes(3, cfg_o))
    with pytest.raises(R.Unsupported), torch.enable_grad():
        F.unbend_points(coarse, pts.clone().requires_grad_(True), lat)
    with pytest.raises(ValueError):
        F.unbend_points(coarse, pts.reshape(15, 3), lat)                 # flat points take one code
    for bad in (dict(tol=-1.0), dict(relaxation=0.0), dict(relaxation=1.5), dict(max_iters=0), dict(max_iters=1025)):
        with pytest.raises(_lib.NrnerfError) as e:
            F.unbend_points(coarse, pts, lat, **bad)
        assert e.value.status == _lib.ERR_INVALID, bad


def test_identity_without_a_bender_and_an_empty_call():
    cfg_n, _, _, plain = modules(dict(N_importance=0, ray_bending=False))
    pts = _scattered_points(15).reshape(3, 5, 3)
    sol = F.unbend_points(plain, pts, None)
    assert torch.equal(sol["points"], pts) and bool(sol["converged"].all()) and int(sol["iterations"].abs().max()) == 0
    assert float(sol["residual"].abs().max()) == 0.0
    cfg, scene, rb, coarse = modules(FAMILIES["default"])
    model = R.get_model(coarse, None, precision="f32", device=DEV)
    x, res, its = model.bender_inverse(torch.empty((0, 5, 3), device=DEV), torch.empty((0, cfg.latent_size), device=DEV))
    assert tuple(x.shape) == (0, 5, 3) and tuple(res.shape) == (0, 5) and tuple(its.shape) == (0, 5)
    empty = F.unbend_points(coarse, torch.empty((0, 3), device=DEV), codes(1, cfg))
    assert tuple(empty["points"].shape) == (0, 3) and tuple(empty["converged"].shape) == (0,)


def test_status_of_pointers_and_workspace_on_the_device():
    cfg, scene, rb, coarse = modules(FAMILIES["default"])
    model = R.get_model(coarse, None, precision="f32", device=DEV)
    lib = model.lib
    need = lib.nrnerf_bender_inverse_workspace_bytes(model.handle)
    assert need == 256
    assert lib.nrnerf_bender_inverse_workspace_bytes(R.get_model(coarse, None, precision="bf16", device=DEV).handle) == 0
    pts = _scattered_points(15).reshape(3, 5, 3).contiguous()
    lat = codes(3, cfg).contiguous()
    out = torch.empty((3, 5, 3), device=DEV)
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) // 256 * 256
    host = torch.zeros(3 * 5 * 3)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def status(**kw):
        a = _lib.BenderInverseArgs()
        a.struct_size = C.sizeof(_lib.BenderInverseArgs)
        a.n_rows, a.n_samples, a.point_stride, a.latent_stride = 3, 5, 3, cfg.latent_size
        a.tolerance, a.relaxation, a.max_iters = 1e-6, 1.0, 4
        a.canonical, a.latents, a.observed, a.workspace, a.workspace_bytes = pts.data_ptr(), lat.data_ptr(), out.data_ptr(), base, need
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.nrnerf_bender_inverse(model.handle, C.byref(a), stream)

    assert status() == _lib.OK
    assert status(canonical=host.data_ptr()) == _lib.ERR_INVALID
    assert status(initial=host.data_ptr()) == _lib.ERR_INVALID
    assert status(observed=host.data_ptr()) == _lib.ERR_INVALID
    assert status(residual=host.data_ptr()) == _lib.ERR_INVALID
    assert status(workspace_bytes=need - 1) == _lib.ERR_WORKSPACE
    assert status(workspace=base + 64) == _lib.ERR_WORKSPACE
    assert status(workspace=None) == _lib.ERR_WORKSPACE
    assert status(workspace=base, workspace_bytes=need, flags=_lib.RENDER_FIXED_SHARES) == _lib.OK
    torch.cuda.synchronize()


def test_a_nan_point_runs_to_max_iters_and_leaves_its_neighbours_alone():
    cfg, scene, rb, coarse = modules(FAMILIES["default"])
    set_knobs(rb, coarse, {})
    pts = _scattered_points(40).reshape(1, 40, 3)
    lat = codes(1, cfg)
    clean = F.unbend_points(coarse, pts, lat, max_iters=16)
    dirty = pts.clone()
    dirty[0, 5, 1] = float("nan")
    sol = F.unbend_points(coarse, dirty, lat, max_iters=16)
    assert int(sol["iterations"][0, 5]) == 16 and not bool(sol["converged"][0, 5]) and bool(torch.isnan(sol["residual"][0, 5]))
    keep = torch.ones(40, dtype=torch.bool, device=DEV)
    keep[5] = False
    for k in ("points", "residual", "iterations", "converged"):
        assert torch.equal(sol[k][0, keep], clean[k][0, keep]), k


# ---- 9. mesh and tracks ------------------------------------------------------------------------------------------------------------------------
def test_a_canonical_mesh_is_carried_into_every_frame(tmp_path):
    cfg, scene, rb, coarse = modules(FAMILIES["default"], 3)
    set_knobs(rb, coarse, {})
    kw = {"network_fn": coarse}
    LO, HI = (-0.8, -0.7, -0.9), (0.9, 0.6, 0.8)
    sigma = F.sample_grid(kw, None, LO, HI, 24, with_bending=False, precision="f32")["sigma"]
    level = float(sigma.min()) + 0.25 * (float(sigma.max()) - float(sigma.min()))
    mesh = F.extract_mesh(kw, None, level, LO, HI, 24, with_bending=False, precision="f32")
    n_v, n_f = int(mesh["vertices"].shape[0]), int(mesh["faces"].shape[0])
    assert n_v > 0 and n_f > 0
    lats = codes(3, cfg, seed=12)
    frames = F.animate_mesh(mesh, kw, lats)
    cold = F.animate_mesh(mesh, kw, lats, warm_start=False)
    assert len(frames) == 3
    for t, frame in enumerate(frames):
        assert frame["faces"] is mesh["faces"] and frame["rgb"] is mesh["rgb"]               # shared, not copied
        assert ("rigidity" in frame) == ("rigidity" in mesh)
        assert tuple(frame["vertices"].shape) == (n_v, 3) and tuple(frame["normals"].shape) == (n_v, 3)
        back = bend(frame["vertices"], coarse, lats[t:t + 1])
        assert torch.equal((back - mesh["vertices"]).abs().max(-1).values, frame["residual"])
        assert torch.equal(frame["converged"], frame["residual"] <= TOL32)
        both = frame["converged"] & cold[t]["converged"]
        assert float((frame["vertices"] - cold[t]["vertices"])[both].abs().max()) <= 10 * TOL
        # (a sum over a vertex's triangles in the device's order: unit vectors equal up to the rounding of a handful of additions)
        assert float((frame["normals"] - F.vertex_normals(frame["vertices"], mesh["faces"])).abs().max()) <= 1e-5
        print(f"[frame {t}] {n_v} vertices, converged {float(frame['converged'].float().mean()):.4f} (cold start {float(cold[t]['converged'].float().mean()):.4f})")
    assert not torch.equal(frames[0]["vertices"], frames[1]["vertices"])
    path = tmp_path / "frame.ply"
    F.write_ply(str(path), frames[2])
    head = path.read_bytes().split(b"end_header\n")[0].decode("ascii")
    assert f"element vertex {n_v}\n" in head and f"element face {n_f}\n" in head and "property uchar red" in head and "property float nx" in head


def test_points_are_tracked_from_one_time_step_to_another():
    cfg, scene, rb, coarse = modules(FAMILIES["default"], 3)
    set_knobs(rb, coarse, {})
    p = _scattered_points(300, seed=13)
    l_a, l_b = codes(1, cfg, seed=14), codes(1, cfg, seed=15)
    got = F.track_points({"network_fn": coarse}, p, l_a, [l_a[0], l_b[0]])
    canonical = got["canonical"]
    assert torch.equal(canonical, bend(p, coarse, l_a))
    at_a, at_b = got["tracks"]
    # back in the source frame: the solver starts at the canonical point and lands on a point that bends to it; where the map is
    # injective that is p itself, within the residual and the map's conditioning -- checked as a point that bends back within the residual
    assert torch.equal((bend(at_a["points"], coarse, l_a) - canonical).abs().max(-1).values, at_a["residual"])
    assert torch.equal((bend(at_b["points"], coarse, l_b) - canonical).abs().max(-1).values, at_b["residual"])
    ok = at_a["converged"]
    assert float(ok.float().mean()) >= 0.99
    # |x - p| <= |bend(x) - bend(p)| / (1 - L) with L the offset field's Lipschitz constant; the synthetic bender's is far below 1/2
    assert float((at_a["points"] - p)[ok].abs().max()) <= 2 * 3 ** 0.5 * TOL + 4 * 2.0 ** -24
    assert not torch.equal(at_a["points"], at_b["points"])
