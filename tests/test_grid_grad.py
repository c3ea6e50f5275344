"""GPU tier of the adjoint of the grid lookup: ``nrnerf_grid_lookup_backward`` by itself, and ``field.grid_lookup`` / ``render_baked_train`` /
``refine_bake`` on top of it.

1. d_grid and d_points against float64 autograd (tests/grid_grad_reference.py); 2. points on vertices and on the top face: weights of exactly
0 and 1, the one-sided derivative; 3. every atomic add colliding; 4. either output alone; 5. ``render_baked_train``'s forward IS
``render_baked``'s; 6. its gradients against float64 autograd through the reference render; 7. ``refine_bake`` against the same steps on the CPU.

Tolerances: 10 x the maximum error of the SAME reference evaluated in float32 on the same inputs, computed here and printed.  d_grid is summed
with atomic adds: its bits are not asserted between runs, d_points' are."""
import ctypes as C

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd import field as F
from nonrigid_nerf_amd import render as R
from tests import grid_grad_reference as G
from tests import volume_reference as V
from tests import warp_reference as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO, HI = (-0.5, 0.25, 1.0), (1.5, 1.0, 4.0)                 # the volume's box (tests/test_warp.py)
WLO, WHI = (-0.1, 0.4, 0.5), (1.1, 1.3, 3.2)                # the warp's: partly overlapping
GRIDS = [(2, 2, 2), (5, 4, 3), (17, 9, 33)]                 # (Gx, Gy, Gz)
VOLUME = (17, 9, 33)
DTYPES = {"f32": torch.float32, "f16": torch.float16}
NAN = float("nan")

_cache = {}


def smooth(g, dtype=torch.float32, kind="v"):
    """A seeded grid ``[Gz, Gy, Gx, 4]`` on the CPU in its storage dtype; built once."""
    key = (kind, g, dtype)
    if key not in _cache:
        _cache[key] = (V.smooth_volume(*g, seed=sum(g)) if kind == "v" else W.smooth_warp(*g, seed=sum(g))).to(dtype)
    return _cache[key]


def cotangent(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def lookup_backward(grid, lo, hi, pts, cot, *, d_grid=True, d_points=True, into=None, pass_grid=True):
    """``nrnerf_grid_lookup_backward`` called directly: ``grid`` on the CPU in its storage dtype, ``pts [M, stride]``, ``cot [M, 4]`` ->
    ``(d_grid or None, d_points or None)`` on the CPU; ``into``: the initial contents of d_grid (zeros)."""
    gd, pd, cd = grid.to(DEV).contiguous(), pts.to(DEV).contiguous(), cot.to(DEV).contiguous()
    M = int(pts.shape[0])
    dg = (torch.zeros(grid.shape, dtype=torch.float32) if into is None else into.clone()).to(DEV) if d_grid else None
    dp = torch.full((M, 3), 7.0, dtype=torch.float32, device=DEV) if d_points else None
    a = _lib.GridLookupBackwardArgs()
    a.struct_size = C.sizeof(a)
    a.grid, a.grid_dtype = (gd.data_ptr() if pass_grid else None), {torch.float32: _lib.VOLUME_F32, torch.float16: _lib.VOLUME_F16}[grid.dtype]
    a.g[:] = (grid.shape[2], grid.shape[1], grid.shape[0])
    a.min_point[:], a.max_point[:] = lo, hi
    a.n_points, a.points, a.point_stride, a.g_value = M, pd.data_ptr(), int(pts.shape[1]), cd.data_ptr()
    a.d_grid, a.d_points = (dg.data_ptr() if d_grid else None), (dp.data_ptr() if d_points else None)
    _lib.check(_lib.load().nrnerf_grid_lookup_backward(C.byref(a), C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)),
               "nrnerf_grid_lookup_backward")
    torch.cuda.synchronize()
    return (dg.cpu() if d_grid else None), (dp.cpu() if d_points else None)


def bar(ref64, ref32, what):
    """10 x the float32 reference's own maximum error."""
    err = float((ref32.double() - ref64).abs().max())
    print(f"  {what}: float32 reference max error {err:.3e} -> bar {10 * err:.3e}")
    return 10 * err


def worst(got, ref64, what):
    w = float((got.double() - ref64).abs().max())
    print(f"  {what}: kernel max error {w:.3e}")
    return w


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def bits_same(a, b):
    """Bit for bit, except that any NaN equals any NaN (disp_map of a ray that hits nothing is 0 / 0)."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def inside_box(pts, lo=LO, hi=HI):
    p = pts[:, :3]
    return ((p >= torch.tensor(lo)) & (p <= torch.tensor(hi))).all(-1)


# ---- 1. against float64 --------------------------------------------------------------------------------------------------------------------------
POINT_SEED = {1: 2, 37 * 33: 1}          # (at seed 2 the one point lies inside the box)


def case_points(m, stride):
    """``m`` points of ``volume_reference.interior_points`` and one NaN point behind them, ``[m + 1, stride]``."""
    pts = torch.cat([V.interior_points((m,), LO, HI, seed=POINT_SEED[m]), torch.tensor([[0.5, NAN, 2.0]])], 0)
    if stride == 4:
        pts = torch.cat([pts, torch.full((m + 1, 1), 3.0)], -1)           # (the fourth column is not read)
    return pts


@pytest.mark.parametrize("m", [1, 37 * 33], ids=["M1", "M1221"])
@pytest.mark.parametrize("stride", [3, 4], ids=["stride3", "stride4"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("g", GRIDS, ids=["2x2x2", "5x4x3", "17x9x33"])
def test_both_gradients_match_float64_autograd(g, dtype, stride, m):
    grid = smooth(g, DTYPES[dtype])
    pts = case_points(m, stride)
    cot = cotangent((m + 1, 4), 100 + m)
    d_grid, d_pts = lookup_backward(grid, LO, HI, pts, cot)
    _, g64, p64 = G.lookup_backward(grid, LO, HI, pts[:, :3], cot)
    _, g32, p32 = G.lookup_backward(grid, LO, HI, pts[:, :3], cot, torch.float32)
    empty = ~inside_box(pts)
    print(f"[{g} {dtype} stride {stride} M {m} + 1] {int(empty.sum())} empty points")
    assert bool(empty[-1]) and int((~empty).sum()) >= 1
    assert worst(d_grid, g64, "d_grid") <= bar(g64, g32, "d_grid")
    assert worst(d_pts, p64, "d_points") <= bar(p64, p32, "d_points")
    # outside the box, or NaN: exact zeros, and nothing is added to the grid
    assert torch.equal(d_pts[empty], torch.zeros_like(d_pts[empty])) and not bool(p64[empty].any())
    before = cotangent(tuple(grid.shape), 9)
    after, zeros = lookup_backward(grid, LO, HI, pts[empty], cot[empty], into=before)
    assert bits_equal(after, before) and torch.equal(zeros, torch.zeros_like(zeros))


# ---- 2. vertices and the top face ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_vertices_and_the_top_face_have_weights_of_exactly_zero_and_one(dtype):
    g = (5, 4, 3)
    grid = smooth(g, DTYPES[dtype])
    lo, hi = (0.0, 0.0, 0.0), (g[0] - 1.0, g[1] - 1.0, g[2] - 1.0)                    # unit spacing: a vertex IS its index, the scale is 1
    verts = W.grid_vertices(lo, hi, g, torch.float32).reshape(-1, 3)                  # every vertex once, the top faces included
    cot = cotangent((verts.shape[0], 4), 21)
    d_grid, d_pts = lookup_backward(grid, lo, hi, verts, cot)
    assert bits_equal(d_grid.reshape(-1, 4), cot)                                     # each cotangent on its own vertex, bit for bit
    # the one-sided derivative: the difference to the NEXT vertex (the upper cell), on a top face from the previous one (the last cell)
    for dt in (torch.float64, torch.float32):
        w = grid.to(dt)
        want = []
        for axis, dim in ((0, 2), (1, 1), (2, 0)):
            fwd = w.narrow(dim, 1, w.shape[dim] - 1) - w.narrow(dim, 0, w.shape[dim] - 1)
            diff = torch.cat([fwd, fwd.narrow(dim, fwd.shape[dim] - 1, 1)], dim)
            want.append((cot.to(dt).reshape(w.shape) * diff).sum(-1).reshape(-1))
        if dt == torch.float64:
            want64 = torch.stack(want, -1)
        else:
            want32 = torch.stack(want, -1)
    assert worst(d_pts, want64, "d_points on vertices") <= bar(want64, want32, "d_points on vertices")
    # on the top face of x, off the vertices in y and z: the x-weights are exactly 0 and 1 -- nothing reaches the vertices below the face
    n = 64
    gen = torch.Generator().manual_seed(22)
    face = torch.cat([torch.full((n, 1), hi[0]), torch.rand(n, 1, generator=gen) * hi[1], torch.rand(n, 1, generator=gen) * hi[2]], -1)
    cot = cotangent((n, 4), 23)
    d_grid, d_pts = lookup_backward(grid, lo, hi, face, cot)
    _, g64, p64 = G.lookup_backward(grid, lo, hi, face, cot)
    _, g32, p32 = G.lookup_backward(grid, lo, hi, face, cot, torch.float32)
    assert not bool(d_grid[:, :, :-1].any()) and bool(d_grid[:, :, -1].any())
    assert worst(d_grid, g64, "d_grid on the face") <= bar(g64, g32, "d_grid on the face")
    assert worst(d_pts, p64, "d_points on the face") <= bar(p64, p32, "d_points on the face")


# ---- 3. collisions -------------------------------------------------------------------------------------------------------------------------------
def test_every_atomic_colliding_stays_within_the_bar():
    """The 2 x 2 x 2 grid is ONE cell: all 4096 points add into the same eight vertices."""
    g, m = (2, 2, 2), 4096
    grid = smooth(g)
    pts = V.interior_points((m,), LO, HI, seed=31, outside_share=0.0)
    cot = cotangent((m, 4), 32)
    assert bool(inside_box(pts).all())
    _, g64, p64 = G.lookup_backward(grid, LO, HI, pts, cot)
    _, g32, p32 = G.lookup_backward(grid, LO, HI, pts, cot, torch.float32)
    tol = bar(g64, g32, "d_grid")
    first, p_first = lookup_backward(grid, LO, HI, pts, cot)
    second, p_second = lookup_backward(grid, LO, HI, pts, cot)
    assert worst(first, g64, "d_grid, first run") <= tol and worst(second, g64, "d_grid, second run") <= tol
    print(f"  the two runs differ by at most {float((first - second).abs().max()):.3e}")
    assert float((first - second).abs().max()) <= tol
    assert worst(p_first, p64, "d_points") <= bar(p64, p32, "d_points") and bits_equal(p_first, p_second)


# ---- 4. either output alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_either_output_alone_is_the_joint_calls(dtype):
    g, m = (17, 9, 33), 37 * 33
    grid = smooth(g, DTYPES[dtype])
    pts, cot = case_points(m, 3), cotangent((m + 1, 4), 41)
    both_g, both_p = lookup_backward(grid, LO, HI, pts, cot)
    again_g, again_p = lookup_backward(grid, LO, HI, pts, cot)
    only_g, none_p = lookup_backward(grid, LO, HI, pts, cot, d_points=False)
    blind_g, _ = lookup_backward(grid, LO, HI, pts, cot, d_points=False, pass_grid=False)          # (d_grid alone does not read the grid)
    none_g, only_p = lookup_backward(grid, LO, HI, pts, cot, d_grid=False)
    assert none_p is None and none_g is None
    assert bits_equal(only_p, both_p) and bits_equal(again_p, both_p)
    _, g64, _ = G.lookup_backward(grid, LO, HI, pts, cot)
    _, g32, _ = G.lookup_backward(grid, LO, HI, pts, cot, torch.float32)
    tol = bar(g64, g32, "d_grid")
    for name, other in (("alone", only_g), ("alone, no grid given", blind_g), ("joint, again", again_g)):
        print(f"  d_grid {name} differs from the joint call's by at most {float((other - both_g).abs().max()):.3e}")
        assert float((other - both_g).abs().max()) <= tol and worst(other, g64, f"d_grid {name}") <= tol


def test_grid_lookup_has_the_bits_of_the_lookup_kernel_and_both_gradients():
    """``field.grid_lookup``: forward = ``volume_render(composite=False)``, backward = the entry point; a half grid gets a half gradient."""
    g, n, s = (5, 4, 3), 7, 9
    pts = V.interior_points((n, s), LO, HI, seed=51)
    cot = cotangent((n, s, 4), 52)
    for dtype in (torch.float32, torch.float16):
        grid = smooth(g, dtype)
        gd = grid.to(DEV).requires_grad_(True)
        pd = pts.to(DEV).requires_grad_(True)
        val = F.grid_lookup(gd, LO, HI, pd)
        p4 = torch.cat([pts, torch.zeros(n, s, 1)], -1).to(DEV)
        rays = torch.zeros(n, 8, device=DEV)
        want = F.volume_render({"raw": grid.to(DEV), "min_point": LO, "max_point": HI}, rays, N_samples=s, points4=p4, composite=False)["raw"]
        assert bits_equal(val.detach(), want)
        d_g, d_p = torch.autograd.grad((val * cot.to(DEV)).sum(), (gd, pd))
        assert d_g.dtype == dtype and d_g.shape == gd.shape and d_p.shape == pd.shape
        raw_g, raw_p = lookup_backward(grid, LO, HI, pts.reshape(-1, 3), cot.reshape(-1, 4))
        assert bits_equal(d_p.cpu().reshape(-1, 3), raw_p)
        _, g64, _ = G.lookup_backward(grid, LO, HI, pts, cot)
        _, g32, _ = G.lookup_backward(grid, LO, HI, pts, cot, torch.float32)
        tol = bar(g64, g32, "d_grid") + (float(g64.abs().max()) * 2.0 ** -11 if dtype == torch.float16 else 0.0)      # (+ the one cast to half)
        assert worst(d_g.cpu(), g64, "d_grid") <= tol


# ---- 5. the forward of render_baked_train --------------------------------------------------------------------------------------------------------
def crossing_rays(n, seed, near=0.5, far=5.0):
    """``n`` rays that cross the box LO .. HI along +z from in front of it, with different direction lengths (tests/test_warp.py's)."""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.5, 0.6, 0.0]) + 0.05 * torch.randn(n, 3, generator=g)
    d = (torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(n, 3, generator=g)) * (0.5 + torch.rand(n, 1, generator=g))
    return torch.cat([o, d, torch.full((n, 1), near), torch.full((n, 1), far)], -1)


def sorted_depths(n, s, seed):
    return torch.sort(0.5 + 4.5 * torch.rand(n, s, generator=torch.Generator().manual_seed(seed)), -1).values


KNOBS = dict(rigidity_cutoff=0.4, test_time_scaling=1.5, removal_threshold=0.6)
FORWARD_CASES = [(2, "f32", "f32", {}), (33, "f32", "f32", {}), (65, "f32", "f32", {}), (33, "f16", "f32", {}), (33, "f32", "f16", {}),
                 (33, "f16", "f16", {}), (65, "f32", "f32", KNOBS)]
MAPS = ("rgb_map", "disp_map", "acc_map", "weights")


@pytest.mark.parametrize("S,vdtype,wdtype,knobs", FORWARD_CASES, ids=[f"S{c[0]}-{c[1]}-{c[2]}{'-knobs' if c[3] else ''}" for c in FORWARD_CASES])
def test_the_forward_of_render_baked_train_is_render_baked(S, vdtype, wdtype, knobs):
    vol = {"raw": smooth(VOLUME, DTYPES[vdtype]).to(DEV), "min_point": LO, "max_point": HI}
    wrp = {"warp": smooth((9, 17, 6), DTYPES[wdtype], "w").to(DEV), "min_point": WLO, "max_point": WHI}
    rays = crossing_rays(37, 5).to(DEV)
    for z, white in ((None, True), (sorted_depths(37, S, S).to(DEV), False)):
        want = F.warped_volume_render(vol, wrp, rays, N_samples=S, z_vals=z, white_bkgd=white, weights=True, return_points=True, **knobs)
        trained = dict(vol, raw=vol["raw"].clone().requires_grad_(True)), dict(wrp, warp=wrp["warp"].clone().requires_grad_(True))
        got = F.render_baked_train(*trained, rays, N_samples=S, z_vals=z, white_bkgd=white, **knobs)
        torch.cuda.synchronize()
        assert set(got) == set(MAPS)
        if S >= 33:
            assert float(want["acc_map"].max()) > 0.5
        if knobs:
            m = want["points4"][..., 3]
            assert bool((m == 0).any()) and bool((m >= knobs["removal_threshold"]).any()) and bool(((m > 0) & (m < knobs["removal_threshold"])).any())
        for k in MAPS:
            assert got[k].requires_grad and bits_same(got[k].detach(), want[k]), (k, z is None)
        with pytest.raises(R.Unsupported):
            F.render_baked(*trained, rays, N_samples=S, z_vals=z)
    straight = F.render_baked_train(vol, None, rays, N_samples=S)
    want = F.volume_render(vol, rays, N_samples=S, weights=True)
    for k in MAPS:
        assert bits_same(straight[k], want[k]), k


# ---- 6. the gradients of render_baked_train ------------------------------------------------------------------------------------------------------
def clear_of(values, target, margin=1e-4):
    """A threshold near ``target`` that no entry of ``values`` comes within ``2 * margin`` of: the middle of the widest gap among the sixty-odd
    sorted values around it."""
    v = torch.sort(values.reshape(-1).double()).values
    at = int(torch.searchsorted(v, torch.tensor(float(target), dtype=torch.float64)))
    w = v[max(0, at - 32):at + 32]
    gaps = w[1:] - w[:-1]
    k = int(torch.argmax(gaps))
    thr = float(np.float32(0.5 * float(w[k] + w[k + 1])))
    assert float((values.double() - thr).abs().min()) > 2 * margin, "no clear threshold here"
    return thr


GRADIENT_CASES = [((2, 2, 2), (37, 33), False), ((9, 17, 6), (37, 33), False), ((2, 2, 2), (3, 5), False), ((9, 17, 6), (3, 5), False),
                  ((9, 17, 6), (37, 33), True)]


@pytest.mark.parametrize("wg,shape,knobs_on", GRADIENT_CASES,
                         ids=[f"warp{'x'.join(map(str, c[0]))}-{c[1][0]}x{c[1][1]}{'-knobs' if c[2] else ''}" for c in GRADIENT_CASES])
def test_the_gradients_of_render_baked_train_match_float64_autograd(wg, shape, knobs_on):
    n, s = shape
    vcpu, wcpu = smooth(VOLUME), smooth(wg, kind="w")
    rays, z = crossing_rays(n, 61 + n), sorted_depths(n, s, 62 + n)
    c_rgb, c_acc, c_w = cotangent((n, 3), 63), cotangent((n,), 64), cotangent((n, s), 65)
    knobs = {}
    if knobs_on:
        # the cutoff and the removal threshold are decisions: thresholds that no sample's rigidity comes within 1e-4 of, in float64 and float32
        mask64 = G.render(vcpu.double(), LO, HI, wcpu.double(), WLO, WHI, rays, z)["mask"]
        mask32 = G.render(vcpu, LO, HI, wcpu, WLO, WHI, rays, z)["mask"]
        both = torch.cat([mask64.reshape(-1), mask32.double().reshape(-1)])
        knobs = dict(rigidity_cutoff=clear_of(both, 0.4), test_time_scaling=1.5, removal_threshold=clear_of(both, 0.6))
        for thr in (knobs["rigidity_cutoff"], knobs["removal_threshold"]):
            assert float((both - thr).abs().min()) > 1e-4                                           # no sample is excluded
        assert bool((mask64 <= knobs["rigidity_cutoff"]).any()) and bool((mask64 >= knobs["removal_threshold"]).any())

    def reference(dtype):
        v, w = vcpu.detach().to(dtype).clone().requires_grad_(True), wcpu.detach().to(dtype).clone().requires_grad_(True)
        out = G.render(v, LO, HI, w, WLO, WHI, rays, z, white_bkgd=True, **knobs)
        loss = (c_rgb.to(dtype) * out["rgb_map"]).sum() + (c_acc.to(dtype) * out["acc_map"]).sum() + (c_w.to(dtype) * out["weights"]).sum()
        return torch.autograd.grad(loss, (v, w))

    v64, w64 = reference(torch.float64)
    v32, w32 = reference(torch.float32)
    vol = {"raw": vcpu.detach().to(DEV).requires_grad_(True), "min_point": LO, "max_point": HI}
    wrp = {"warp": wcpu.detach().to(DEV).requires_grad_(True), "min_point": WLO, "max_point": WHI}
    out = F.render_baked_train(vol, wrp, rays.to(DEV), N_samples=s, z_vals=z.to(DEV), white_bkgd=True, **knobs)
    loss = (c_rgb.to(DEV) * out["rgb_map"]).sum() + (c_acc.to(DEV) * out["acc_map"]).sum() + (c_w.to(DEV) * out["weights"]).sum()
    d_vol, d_warp = torch.autograd.grad(loss, (vol["raw"], wrp["warp"]))
    torch.cuda.synchronize()
    print(f"[warp {wg}, {n} x {s}, knobs {knobs}] |d volume| up to {float(v64.abs().max()):.3e}, |d warp| up to {float(w64.abs().max()):.3e}")
    assert float(v64.abs().max()) > 0 and float(w64.abs().max()) > 0
    assert worst(d_vol.cpu(), v64, "d volume") <= bar(v64, v32, "d volume")
    assert worst(d_warp.cpu(), w64, "d warp") <= bar(w64, w32, "d warp")
    # one of the two alone: the same gradient (the volume's within the bar -- its sums are atomic; the warp's has the volume's d_points behind it)
    alone = F.render_baked_train(dict(vol, raw=vol["raw"].detach()), wrp, rays.to(DEV), N_samples=s, z_vals=z.to(DEV), white_bkgd=True, **knobs)
    loss = (c_rgb.to(DEV) * alone["rgb_map"]).sum() + (c_acc.to(DEV) * alone["acc_map"]).sum() + (c_w.to(DEV) * alone["weights"]).sum()
    assert worst(torch.autograd.grad(loss, wrp["warp"])[0].cpu(), w64, "d warp alone") <= bar(w64, w32, "d warp")


# ---- 7. refine_bake ------------------------------------------------------------------------------------------------------------------------------
def test_refine_bake_takes_the_steps_of_the_cpu_reference():
    """Ten steps of plain gradient descent on the 17 x 9 x 33 volume, 37 rays of 33 samples through a fixed warp, the targets the render of
    ANOTHER volume: the refined volume against the same ten steps in float64 on the CPU, the bar from the same ten steps in float32."""
    n, s, steps, lr = 37, 33, 10, 20.0
    vcpu, wcpu = smooth(VOLUME), smooth((5, 4, 3), kind="w")
    rays = crossing_rays(n, 71)
    z = V.coarse_depths(rays, s, dtype=torch.float32)
    target = W.render_reference(V.smooth_volume(*VOLUME, seed=5), LO, HI, wcpu, WLO, WHI, rays, z.double())["rgb_map"].float()

    def cpu_steps(dtype):
        v, losses = vcpu.detach().to(dtype).clone().requires_grad_(True), []
        for _ in range(steps):
            out = G.render(v, LO, HI, wcpu.to(dtype), WLO, WHI, rays, z.to(dtype) if dtype == torch.float32 else V.coarse_depths(rays, s))
            loss = ((out["rgb_map"] - target.to(dtype)) ** 2).mean()
            (grad,) = torch.autograd.grad(loss, v)
            v = (v.detach() - lr * grad).requires_grad_(True)
            losses.append(float(loss.detach()))
        return v.detach(), losses

    v64, loss64 = cpu_steps(torch.float64)
    v32, loss32 = cpu_steps(torch.float32)
    vol = {"raw": vcpu.to(DEV), "min_point": LO, "max_point": HI}
    wrp = {"warp": wcpu.to(DEV), "min_point": WLO, "max_point": WHI}
    new_vol, new_warps, history = F.refine_bake(vol, wrp, [(rays.to(DEV), target.to(DEV), 0)], steps=steps, lr=lr, optimizer="sgd", N_samples=s)
    torch.cuda.synchronize()
    print(f"  loss {history[0]:.5e} -> {history[-1]:.5e} on the device, {loss64[0]:.5e} -> {loss64[-1]:.5e} in float64; "
          f"the volume moved by up to {float((v64 - vcpu.double()).abs().max()):.3e}")
    assert len(history) == steps and history[-1] < history[0] and loss64[-1] < loss64[0]
    assert bits_equal(vol["raw"].cpu(), vcpu) and bits_equal(new_warps["warp"].cpu(), wcpu)           # the inputs are not modified, the warp not refined
    assert float((v64 - vcpu.double()).abs().max()) > 1e-3
    assert worst(new_vol["raw"].cpu(), v64, "refined volume") <= bar(v64, v32, "refined volume")


def test_refine_bake_refines_a_stack_of_warps_with_adam_on_ray_batches():
    """Volume and warps together, one warp per frame, Adam on batches of 16 of the 37 rays, half records in and out: the loss falls, both
    grids move, the records keep their dtype and the inputs their bits; the same seed takes the same batches."""
    n, s = 37, 33
    vcpu = smooth(VOLUME, torch.float16)
    wcpu = torch.stack([smooth((5, 4, 3), torch.float16, "w"), smooth((9, 17, 6), kind="w")[:3, :4, :5].contiguous().half()], 0)
    vol = {"raw": vcpu.to(DEV), "min_point": LO, "max_point": HI}
    wrp = {"warp": wcpu.to(DEV), "min_point": WLO, "max_point": WHI}
    frames = []
    for index, seed in ((0, 81), (1, 82)):
        rays = crossing_rays(n, seed)
        z = V.coarse_depths(rays, s)
        target = W.render_reference(V.smooth_volume(*VOLUME, seed=5), LO, HI, wcpu[index], WLO, WHI, rays, z)["rgb_map"].float()
        frames.append((rays.to(DEV), target.to(DEV), index))
    kw = dict(steps=12, lr=2e-2, batch_rays=16, params=("volume", "warp"), N_samples=s)
    new_vol, new_warps, history = F.refine_bake(vol, wrp, frames, seed=3, **kw)
    again_vol, again_warps, again = F.refine_bake(vol, wrp, frames, seed=3, **kw)
    torch.cuda.synchronize()
    print(f"  loss per step: {' '.join(f'{v:.4f}' for v in history)}")
    assert len(history) == 12 and min(history[-2:]) < min(history[:2])                    # (frames alternate: compare like with like)
    assert new_vol["raw"].dtype == torch.float16 and new_warps["warp"].dtype == torch.float16 and new_warps["warp"].shape == wcpu.shape
    assert torch.equal(vol["raw"].cpu(), vcpu) and torch.equal(wrp["warp"].cpu(), wcpu)
    assert not torch.equal(new_vol["raw"].cpu(), vcpu)
    assert not torch.equal(new_warps["warp"][0].cpu(), wcpu[0]) and not torch.equal(new_warps["warp"][1].cpu(), wcpu[1])
    # the same batches: the histories agree to the rounding of the reordered atomic sums
    assert max(abs(a - b) for a, b in zip(history, again)) <= 1e-4 * max(history)
    with pytest.raises(ValueError):
        F.refine_bake(vol, None, frames, steps=1, lr=1e-2, params=("warp",), N_samples=s)
