"""GPU tier of the adjoint of the spherical-harmonic colour sum: ``nrnerf_sh_lookup_backward`` by itself, and ``field.sh_lookup`` /
``render_sh_train`` / ``refine_sh_bake`` on top of it.

1. d_sh, d_points and d_dirs against float64 autograd (tests/sh_grad_reference.py); 2. empty samples; 3. points on vertices and on the top face:
weights of exactly 0 and 1, the one-sided derivative; 4. every atomic add colliding; 5. each output alone; 6. coincident points; 7. the forwards
ARE ``sh_volume_render``'s / ``render_baked``'s; 8. the gradients of ``render_sh_train`` against float64 autograd through the reference render;
9. ``refine_sh_bake`` against the same steps on the CPU; 10. refusals.

Tolerances: 10 x the maximum error of the SAME reference evaluated in float32 on the same inputs, computed here and printed.  d_sh is summed
with atomic adds: its bits are not asserted between runs, d_points' and d_dirs' are."""
import ctypes as C

import pytest
import torch

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd import field as F
from nonrigid_nerf_amd import render as R
from tests import sh_grad_reference as SG
from tests import sh_reference as SH
from tests import volume_reference as V
from tests import warp_reference as W
from tests.test_grid_grad import clear_of
from tests.test_warp import DEV, DTYPES, HI, LO, VOLUME, WHI, WLO, bar, bits_equal, bits_same, crossing_rays, sorted_depths

pytestmark = pytest.mark.gpu
GRIDS = [(2, 2, 2), (5, 4, 3), (17, 9, 33)]                 # (Gx, Gy, Gz)
SHAPES = [(1, 2), (3, 5), (37, 33)]
DIFF, RAY = _lib.SH_DIRECTION_DIFFERENCES, _lib.SH_DIRECTION_RAY
NAN = float("nan")

_cache = {}


def coefficients(g, degree, dtype=torch.float32):
    """A seeded coefficient array ``[Gz, Gy, Gx, 12 * degree]`` on the CPU in its storage dtype (degree 1: channels 9 .. 11 zero); built once."""
    key = ("sh", g, degree, dtype)
    if key not in _cache:
        sh = SH.smooth_sh(*g, 2, seed=5 + sum(g))[..., :12 * degree].clone()
        if degree == 1:
            sh[..., 9:] = 0
        _cache[key] = sh.to(dtype)
    return _cache[key]


def raw_volume(g, dtype=torch.float32):
    key = ("raw", g, dtype)
    if key not in _cache:
        _cache[key] = V.smooth_volume(*g, seed=sum(g)).to(dtype)
    return _cache[key]


def warp_grid(g, dtype=torch.float32):
    key = ("warp", g, dtype)
    if key not in _cache:
        _cache[key] = W.smooth_warp(*g, seed=sum(g), amplitude=0.15).to(dtype)
    return _cache[key]


def cotangent(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def bent_points(n, s, seed, nan=False):
    """``(rays [n, 8], points4 [n, s, 4])`` float32: the samples of rays that cross the box LO .. HI from in front of it to behind it -- some of
    them outside -- moved by a few hundredths as a bender would; ``nan``: one sample in the middle is NaN."""
    rays = crossing_rays(n, seed)
    if s == 2:
        pts = torch.tensor([[0.5, 0.6, 0.6], [0.52, 0.63, 2.2]]).expand(n, 2, 3)           # in front of the box, inside it
    else:
        pts = W.sample_points(rays, sorted_depths(n, s, seed + 1), torch.float32)
    pts = pts + 0.02 * torch.randn(n, s, 3, generator=torch.Generator().manual_seed(seed + 2))
    if nan:
        pts[n // 2, s // 2, 1] = NAN
    return rays, torch.cat([pts, torch.zeros(n, s, 1)], -1).contiguous()


def sh_backward(sh, degree, lo, hi, p4, cot, mode, rays=None, *, d_sh=True, d_points=True, d_dirs=True, into=None, pass_sh=True):
    """``nrnerf_sh_lookup_backward`` called directly: ``sh`` on the CPU in its storage dtype, ``p4 [N, S, 4]``, ``cot [N, S, 4]`` -> ``(d_sh,
    d_points, d_dirs)`` on the CPU, None where not asked for; ``into``: the initial contents of d_sh (zeros)."""
    n, s = int(p4.shape[0]), int(p4.shape[1])
    shd, pd, cd = sh.to(DEV).contiguous(), p4.to(DEV).contiguous(), cot.to(DEV).contiguous()
    rd = None if rays is None else rays.to(DEV).contiguous()
    ds = (torch.zeros(sh.shape, dtype=torch.float32) if into is None else into.clone()).to(DEV) if d_sh else None
    dp = torch.full((n, s, 3), 7.0, dtype=torch.float32, device=DEV) if d_points else None
    dd = torch.full((n, s, 3), 7.0, dtype=torch.float32, device=DEV) if d_dirs else None
    a = _lib.ShLookupBackwardArgs()
    a.struct_size = C.sizeof(a)
    a.n_rays, a.n_samples = n, s
    if rd is not None:
        a.rays, a.ray_stride = rd.data_ptr(), int(rd.shape[1])
    a.points4, a.direction_mode = pd.data_ptr(), mode
    a.sh, a.sh_dtype, a.sh_degree = (shd.data_ptr() if pass_sh else None), {torch.float32: _lib.VOLUME_F32, torch.float16: _lib.VOLUME_F16}[sh.dtype], degree
    a.g[:] = (sh.shape[2], sh.shape[1], sh.shape[0])
    a.min_point[:], a.max_point[:] = lo, hi
    a.g_raw = cd.data_ptr()
    a.d_sh, a.d_points, a.d_dirs = (ds.data_ptr() if d_sh else None), (dp.data_ptr() if d_points else None), (dd.data_ptr() if d_dirs else None)
    _lib.check(_lib.load().nrnerf_sh_lookup_backward(C.byref(a), C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)),
               "nrnerf_sh_lookup_backward")
    torch.cuda.synchronize()
    return (ds.cpu() if d_sh else None), (dp.cpu() if d_points else None), (dd.cpu() if d_dirs else None)


def references(sh, degree, lo, hi, p4, cot, mode, rays):
    kw = dict(rays=rays, ray_directions=mode == RAY)
    return SG.lookup_backward(sh, degree, lo, hi, p4, cot, **kw), SG.lookup_backward(sh, degree, lo, hi, p4, cot, dtype=torch.float32, **kw)


def worst(got, ref64, what):
    w = float((got.double() - ref64).abs().max())
    print(f"  {what}: kernel max error {w:.3e}")
    return w


def empty_samples(p4, lo=LO, hi=HI):
    p = p4[..., :3]
    return ~((p >= torch.tensor(lo)) & (p <= torch.tensor(hi))).all(-1)


def smallest_step(p4):
    e = p4[:, 1:, :3].double() - p4[:, :-1, :3].double()
    return float(torch.sqrt((e * e).sum(-1)).min())


def check_three(got, ref64, ref32, label=""):
    for name, k, r64, r32 in zip(("d_sh", "d_points", "d_dirs"), got, ref64, ref32):
        if k is not None:
            assert worst(k, r64, label + name) <= bar(r64, r32, label + name), name


# ---- 1. against float64 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{s}" for n, s in SHAPES])
@pytest.mark.parametrize("mode", [DIFF, RAY], ids=["differences", "ray"])
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("g", GRIDS, ids=["2x2x2", "5x4x3", "17x9x33"])
def test_all_three_gradients_match_float64_autograd(g, degree, storage, mode, shape):
    n, s = shape
    sh = coefficients(g, degree, DTYPES[storage])
    rays, p4 = bent_points(n, s, 3 + n, nan=mode == RAY and n * s > 2)      # (a NaN position under DIFFERENCES poisons its neighbour's direction)
    cot = cotangent((n, s, 4), 100 + n)
    empty = empty_samples(p4)
    print(f"[{g} degree {degree} {storage} mode {mode} {n} x {s}] {int(empty.sum())} of {empty.numel()} samples empty")
    assert bool(empty.any()) and bool((~empty).any())
    assert bool((p4[..., :3][empty & ~torch.isnan(p4[..., :3]).any(-1)]).numel())            # samples outside the box, not only the NaN one
    if mode == DIFF:
        assert smallest_step(p4) > 1e-3
    ref64, ref32 = references(sh, degree, LO, HI, p4, cot, mode, rays)
    got = sh_backward(sh, degree, LO, HI, p4, cot, mode, rays)
    check_three(got, ref64, ref32)
    assert torch.equal(got[2][empty], torch.zeros_like(got[2][empty])) and not bool(ref64[2][empty].any())      # d_dirs of an empty sample
    if mode == RAY:
        assert torch.equal(got[1][empty], torch.zeros_like(got[1][empty]))
    if degree == 1:
        before = cotangent(tuple(sh.shape), 9)
        after, _, _ = sh_backward(sh, degree, LO, HI, p4, cot, mode, rays, d_points=False, d_dirs=False, into=before)
        assert bits_equal(after[..., 9:].contiguous(), before[..., 9:].contiguous()) and not bits_equal(after, before)


# ---- 2. empty samples ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2])
def test_empty_samples_add_nothing(degree):
    g = (5, 4, 3)
    sh = coefficients(g, degree)
    gen = torch.Generator().manual_seed(12)
    n, s = 5, 7
    out = torch.cat([1.6 + torch.rand(n, s, 1, generator=gen), 0.25 + 0.75 * torch.rand(n, s, 1, generator=gen),
                     1.0 + 3.0 * torch.rand(n, s, 1, generator=gen), torch.zeros(n, s, 1)], -1)          # x beyond the box
    out[2, 3, 2] = NAN
    cot = cotangent((n, s, 4), 13)
    rays = crossing_rays(n, 14)
    assert bool(empty_samples(out).all())
    before = cotangent(tuple(sh.shape), 15)
    d_sh, d_pts, d_dirs = sh_backward(sh, degree, LO, HI, out, cot, RAY, rays, into=before)
    assert bits_equal(d_sh, before) and torch.equal(d_dirs, torch.zeros_like(d_dirs)) and torch.equal(d_pts, torch.zeros_like(d_pts))
    out[2, 3, 2] = 2.0
    d_sh, d_pts, d_dirs = sh_backward(sh, degree, LO, HI, out, cot, DIFF, into=before)
    assert bits_equal(d_sh, before) and torch.equal(d_dirs, torch.zeros_like(d_dirs)) and torch.equal(d_pts, torch.zeros_like(d_pts))
    # an outside sample between two inside ones: its d_points is the direction part alone
    _, p4 = bent_points(3, 5, 16)
    p4[:, 1:4, :3] = torch.tensor([[0.4, 0.5, 1.5], [2.0, 0.55, 2.0], [0.5, 0.6, 2.5]])[None] + 0.01 * torch.randn(3, 3, 3, generator=gen)
    empty = empty_samples(p4)
    assert bool(empty[:, 2].all()) and not bool(empty[:, 1].any()) and not bool(empty[:, 3].any()) and smallest_step(p4) > 1e-3
    cot = cotangent((3, 5, 4), 17)
    ref64, ref32 = references(sh, degree, LO, HI, p4, cot, DIFF, None)
    got = sh_backward(sh, degree, LO, HI, p4, cot, DIFF)
    check_three(got, ref64, ref32)
    # (the position part of the reference there is exactly zero: with the directions held fixed nothing reaches the point)
    _, pos64, _ = SG.lookup_backward(sh, degree, LO, HI, p4, cot, rays=crossing_rays(3, 1), ray_directions=True)
    assert not bool(pos64[:, 2].any()) and bool(ref64[1][:, 2].any()) and bool(got[1][:, 2].any())
    assert worst(got[1][:, 2], ref64[1][:, 2], "d_points of the outside samples") <= bar(ref64[1], ref32[1], "d_points")


# ---- 3. vertices and the top face ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("degree", [1, 2])
def test_vertices_and_the_top_face_have_weights_of_exactly_zero_and_one(degree, storage):
    g = (5, 4, 3)
    sh = coefficients(g, degree, DTYPES[storage])
    ch = 12 * degree
    used = 3 * ((degree + 1) ** 2 - 1)
    lo, hi = (0.0, 0.0, 0.0), (g[0] - 1.0, g[1] - 1.0, g[2] - 1.0)                    # unit spacing: a vertex IS its index, the scale is 1
    verts = W.grid_vertices(lo, hi, g, torch.float32).reshape(-1, 3)                  # every vertex once, the top faces included
    n = verts.shape[0]
    gen = torch.Generator().manual_seed(21)
    keep = torch.rand(n, generator=gen) < 0.5                                         # the other vertices get no point: they stay exactly zero
    keep[-1] = True                                                                   # (the corner of the three top faces)
    at = torch.nonzero(keep)[:, 0]
    p4 = torch.cat([verts[at], torch.zeros(at.numel(), 1)], -1)[:, None].contiguous()  # one sample per ray: the RAY rule
    rays = torch.cat([torch.zeros(at.numel(), 3), torch.randn(at.numel(), 3, generator=gen), torch.zeros(at.numel(), 2)], -1)
    cot = cotangent((at.numel(), 1, 4), 22)
    d_sh, d_pts, d_dirs = sh_backward(sh, degree, lo, hi, p4, cot, RAY, rays)
    d_sh = d_sh.reshape(n, ch)
    assert not bool(d_sh[~keep].any()) and not bool(d_sh[:, used:].any())             # exact zeros elsewhere
    want = {}
    for dt in (torch.float64, torch.float32):
        Y = SH.basis(SH.directions(p4, rays, True, dt), degree, dt)[:, 0, 1:]        # [n, K - 1]
        want[dt] = (Y[:, :, None] * cot.to(dt)[:, 0, None, :3]).reshape(at.numel(), used)
    assert bool(d_sh[keep][:, :used].any())
    assert worst(d_sh[keep][:, :used], want[torch.float64], "d_sh on vertices") <= bar(want[torch.float64], want[torch.float32], "d_sh on vertices")
    # the one-sided derivative: the difference to the NEXT vertex (the upper cell), on a top face from the previous one (the last cell)
    ref64, ref32 = references(sh, degree, lo, hi, p4, cot, RAY, rays)
    check_three((None, d_pts, d_dirs), ref64, ref32, "on vertices: ")
    w = sh.double()
    fwd = w[:, :, 1:] - w[:, :, :-1]
    diff = torch.cat([fwd, fwd[:, :, -1:]], 2).reshape(n, ch)[at][:, :used]
    explicit = (want[torch.float64] * diff).sum(-1)
    assert float((ref64[1][:, 0, 0] - explicit).abs().max()) <= 1e-12 * max(1.0, float(explicit.abs().max()))
    # on the top face of x, off the vertices in y and z: the x-weights are exactly 0 and 1 -- nothing reaches the vertices below the face
    m = 64
    face = torch.cat([torch.full((m, 1), hi[0]), torch.rand(m, 1, generator=gen) * hi[1], torch.rand(m, 1, generator=gen) * hi[2],
                      torch.zeros(m, 1)], -1)[:, None].contiguous()
    rays = torch.cat([torch.zeros(m, 3), torch.randn(m, 3, generator=gen), torch.zeros(m, 2)], -1)
    cot = cotangent((m, 1, 4), 23)
    got = sh_backward(sh, degree, lo, hi, face, cot, RAY, rays)
    assert not bool(got[0][:, :, :-1].any()) and bool(got[0][:, :, -1].any())
    check_three(got, *references(sh, degree, lo, hi, face, cot, RAY, rays), "on the face: ")


# ---- 4. collisions ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2])
def test_every_atomic_colliding_stays_within_the_bar(degree):
    """The 2 x 2 x 2 grid is ONE cell: all 64 x 64 samples add into the same eight vertices."""
    g, n, s = (2, 2, 2), 64, 64
    sh = coefficients(g, degree)
    pts = V.interior_points((n, s), LO, HI, seed=31, outside_share=0.0)
    p4 = torch.cat([pts, torch.zeros(n, s, 1)], -1).contiguous()
    cot = cotangent((n, s, 4), 32)
    assert not bool(empty_samples(p4).any()) and smallest_step(p4) > 1e-3
    ref64, ref32 = references(sh, degree, LO, HI, p4, cot, DIFF, None)
    first = sh_backward(sh, degree, LO, HI, p4, cot, DIFF)
    second = sh_backward(sh, degree, LO, HI, p4, cot, DIFF)
    check_three(first, ref64, ref32, "first run: ")
    check_three(second, ref64, ref32, "second run: ")
    print(f"  the two runs' d_sh differ by at most {float((first[0] - second[0]).abs().max()):.3e}")
    assert bits_equal(first[1], second[1]) and bits_equal(first[2], second[2])


# ---- 5. each output alone --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("mode", [DIFF, RAY], ids=["differences", "ray"])
def test_each_output_alone_is_the_joint_calls(mode, storage):
    g, degree, (n, s) = (17, 9, 33), 2, (37, 33)
    sh = coefficients(g, degree, DTYPES[storage])
    rays, p4 = bent_points(n, s, 41, nan=mode == RAY)
    cot = cotangent((n, s, 4), 42)
    run = lambda **kw: sh_backward(sh, degree, LO, HI, p4, cot, mode, rays if mode == RAY else None, **kw)
    both = run()
    again = run()
    assert bits_equal(again[1], both[1]) and bits_equal(again[2], both[2])                                  # two runs: the same bits
    only_sh = run(d_points=False, d_dirs=False)
    blind_sh = run(d_points=False, d_dirs=False, pass_sh=False)                                              # (d_sh alone does not read the coefficients)
    only_dirs = run(d_sh=False, d_points=False)
    assert only_sh[1] is None and only_sh[2] is None and only_dirs[0] is None and only_dirs[1] is None
    assert bits_equal(only_dirs[2], both[2])
    if mode == RAY:
        only_pts = run(d_sh=False, d_dirs=False)
        assert only_pts[0] is None and only_pts[2] is None and bits_equal(only_pts[1], both[1])
    else:
        pts_dirs = run(d_sh=False)                                                                           # (the chain's workspace is d_dirs)
        assert pts_dirs[0] is None and bits_equal(pts_dirs[1], both[1]) and bits_equal(pts_dirs[2], both[2])
    ref64, ref32 = references(sh, degree, LO, HI, p4, cot, mode, rays)
    tol = bar(ref64[0], ref32[0], "d_sh")
    for name, other in (("alone", only_sh[0]), ("alone, no coefficients given", blind_sh[0]), ("joint, again", again[0])):
        print(f"  d_sh {name} differs from the joint call's by at most {float((other - both[0]).abs().max()):.3e}")
        assert float((other - both[0]).abs().max()) <= tol and worst(other, ref64[0], f"d_sh {name}") <= tol


# ---- 6. coincident points --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2])
def test_coincident_bent_points_give_finite_gradients(degree):
    sh = coefficients((5, 4, 3), degree)
    _, p4 = bent_points(3, 5, 51)
    p4[:, 1:4, :3] = torch.tensor([[0.4, 0.5, 1.5], [0.45, 0.55, 2.0], [0.5, 0.6, 2.5]])[None]
    p4[1, 2] = p4[1, 1]                                                               # n_2 == 0 in the middle of a ray
    p4[2, 1] = p4[2, 0]                                                               # n_1 == 0: d_0 = d_1 = 0
    assert smallest_step(p4) == 0.0
    for out in sh_backward(sh, degree, LO, HI, p4, cotangent((3, 5, 4), 52), DIFF):
        assert bool(torch.isfinite(out).all()) and bool(out.any())


# ---- 7. the forwards -------------------------------------------------------------------------------------------------------------------------------
def sh_record(degree, dtype=torch.float32, zero=False):
    sh = coefficients(VOLUME, degree, dtype)
    return {"raw": raw_volume(VOLUME, dtype).to(DEV), "sh": (torch.zeros_like(sh) if zero else sh).to(DEV), "sh_degree": degree,
            "min_point": LO, "max_point": HI}


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("degree", [1, 2])
def test_the_forward_of_sh_lookup_is_the_lookup_kernels(degree, storage):
    rec = sh_record(degree, DTYPES[storage])
    rays, p4 = bent_points(37, 33, 61)
    for with_rays in (False, True):
        want = F.sh_volume_render(rec, rays.to(DEV), N_samples=33, points4=p4.to(DEV), retraw=True, ray_directions=with_rays)["raw"]
        trained = dict(rec, raw=rec["raw"].clone().requires_grad_(True), sh=rec["sh"].clone().requires_grad_(True))
        got = F.sh_lookup(trained, p4[..., :3].to(DEV).requires_grad_(True), rays.to(DEV) if with_rays else None)
        assert got.requires_grad and bits_same(got.detach(), want) and bool((want[..., :3] != 0).any())


KNOBS = dict(rigidity_cutoff=0.4, test_time_scaling=1.5, removal_threshold=0.6)
MAPS = ("rgb_map", "disp_map", "acc_map", "weights")


@pytest.mark.parametrize("shape", [(37, 33), (3, 130)], ids=["37x33", "3x130"])
@pytest.mark.parametrize("degree", [1, 2])
def test_the_forward_of_render_sh_train_is_render_baked(degree, shape):
    n, s = shape
    rec = sh_record(degree)
    wrp = {"warp": warp_grid((9, 17, 6)).to(DEV), "min_point": WLO, "max_point": WHI}
    rays = crossing_rays(n, 5).to(DEV)
    for z, white, knobs in ((None, True, {}), (sorted_depths(n, s, s).to(DEV), False, KNOBS)):
        want = F.render_baked(rec, wrp, rays, N_samples=s, z_vals=z, white_bkgd=white, **knobs)
        want["weights"] = F.sh_volume_render(rec, rays, warp=wrp, N_samples=s, z_vals=z, white_bkgd=white, weights=True, **knobs)["weights"]
        trained = dict(rec, sh=rec["sh"].clone().requires_grad_(True)), dict(wrp, warp=wrp["warp"].clone().requires_grad_(True))
        got = F.render_sh_train(*trained, rays, N_samples=s, z_vals=z, white_bkgd=white, **knobs)
        torch.cuda.synchronize()
        assert set(got) == set(MAPS) and float(want["acc_map"].max()) > 0.5
        for k in MAPS:
            assert got[k].requires_grad and bits_same(got[k].detach(), want[k]), (k, z is None)
    straight = F.render_sh_train(rec, None, rays, N_samples=s)
    want = F.sh_volume_render(rec, rays, N_samples=s, weights=True)
    for k in MAPS:
        assert bits_same(straight[k], want[k]), k


# ---- 8. the gradients of render_sh_train -----------------------------------------------------------------------------------------------------------
def map_loss(out, c_rgb, c_acc, c_w):
    return (c_rgb * out["rgb_map"]).sum() + (c_acc * out["acc_map"]).sum() + (c_w * out["weights"]).sum()


@pytest.mark.parametrize("knobs_on", [False, True], ids=["plain", "knobs"])
@pytest.mark.parametrize("degree", [1, 2])
def test_the_gradients_of_render_sh_train_match_float64_autograd(degree, knobs_on):
    n, s, wg = 37, 33, (9, 17, 6)
    vcpu, shcpu, wcpu = raw_volume(VOLUME), coefficients(VOLUME, degree), warp_grid(wg)
    rays, z = crossing_rays(n, 61 + n), sorted_depths(n, s, 62 + n)
    cots = cotangent((n, 3), 63), cotangent((n,), 64), cotangent((n, s), 65)
    knobs = {}
    if knobs_on:
        mask64 = SG.render(vcpu.double(), shcpu.double(), degree, LO, HI, wcpu.double(), WLO, WHI, rays, z)["mask"]
        mask32 = SG.render(vcpu, shcpu, degree, LO, HI, wcpu, WLO, WHI, rays, z)["mask"]
        both = torch.cat([mask64.reshape(-1), mask32.double().reshape(-1)])
        knobs = dict(rigidity_cutoff=clear_of(both, 0.4), test_time_scaling=1.5, removal_threshold=clear_of(both, 0.6))
        for thr in (knobs["rigidity_cutoff"], knobs["removal_threshold"]):
            assert float((both - thr).abs().min()) > 1e-4                                           # no sample's rigidity comes near a threshold
        assert bool((mask64 <= knobs["rigidity_cutoff"]).any()) and bool((mask64 >= knobs["removal_threshold"]).any())

    def reference(dtype, coeff):
        leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (vcpu, coeff, wcpu)]
        out = SG.render(leaves[0], leaves[1], degree, LO, HI, leaves[2], WLO, WHI, rays, z, white_bkgd=True, **knobs)
        return torch.autograd.grad(map_loss(out, *(c.to(dtype) for c in cots)), leaves)

    def device(fn, coeff, with_sh=True):
        vol = {"raw": vcpu.to(DEV).requires_grad_(True), "min_point": LO, "max_point": HI}
        if with_sh:
            vol.update(sh=coeff.to(DEV).requires_grad_(True), sh_degree=degree)
        wrp = {"warp": wcpu.to(DEV).requires_grad_(True), "min_point": WLO, "max_point": WHI}
        out = fn(vol, wrp, rays.to(DEV), N_samples=s, z_vals=z.to(DEV), white_bkgd=True, **knobs)
        leaves = [vol["raw"]] + ([vol["sh"]] if with_sh else []) + [wrp["warp"]]
        grads = torch.autograd.grad(map_loss(out, *(c.to(DEV) for c in cots)), leaves)
        torch.cuda.synchronize()
        return [t.cpu() for t in grads]

    ref64, ref32 = reference(torch.float64, shcpu), reference(torch.float32, shcpu)
    got = device(F.render_sh_train, shcpu)
    print(f"[degree {degree}, knobs {knobs}] |d raw| up to {float(ref64[0].abs().max()):.3e}, |d sh| up to {float(ref64[1].abs().max()):.3e}, "
          f"|d warp| up to {float(ref64[2].abs().max()):.3e}")
    for name, k, r64, r32 in zip(("d raw", "d sh", "d warp"), got, ref64, ref32):
        assert float(r64.abs().max()) > 0
        assert worst(k, r64, name) <= bar(r64, r32, name), name
    # all-zero coefficients: the raw and warp gradients are render_baked_train's on "raw"
    zero = torch.zeros_like(shcpu)
    z64, z32 = reference(torch.float64, zero), reference(torch.float32, zero)
    got0 = device(F.render_sh_train, zero)
    plain = device(F.render_baked_train, None, with_sh=False)
    for name, a, b, r64, r32 in (("d raw", got0[0], plain[0], z64[0], z32[0]), ("d warp", got0[2], plain[1], z64[2], z32[2])):
        diff = float((a - b).abs().max())
        print(f"  zero coefficients, {name}: differs from render_baked_train's by at most {diff:.3e}")
        assert diff <= bar(r64, r32, name + " (zero coefficients)")


# ---- 9. refine_sh_bake -----------------------------------------------------------------------------------------------------------------------------
def test_refine_sh_bake_takes_the_steps_of_the_cpu_reference():
    """Ten steps of plain gradient descent on the 17 x 9 x 33 degree-2 record, 37 rays of 33 samples through a fixed warp, the targets the
    render of ANOTHER record: the losses and the refined raw and sh against the same ten steps in float64 on the CPU, the bar from the same
    ten steps in float32."""
    n, s, steps, lr, degree = 37, 33, 10, 20.0, 2
    vcpu, shcpu, wcpu = raw_volume(VOLUME), coefficients(VOLUME, degree), warp_grid((5, 4, 3))
    rays = crossing_rays(n, 71)
    z = V.coarse_depths(rays, s, dtype=torch.float32)
    other = V.smooth_volume(*VOLUME, seed=5), SH.smooth_sh(*VOLUME, degree, seed=6)
    target = SH.render_reference(*other, degree, LO, HI, rays, z.double(), warp=wcpu, warp_min=WLO, warp_max=WHI)["rgb_map"].float()

    def cpu_steps(dtype):
        v, c, losses = vcpu.detach().to(dtype).clone().requires_grad_(True), shcpu.detach().to(dtype).clone().requires_grad_(True), []
        for _ in range(steps):
            out = SG.render(v, c, degree, LO, HI, wcpu.to(dtype), WLO, WHI, rays, z.to(dtype) if dtype == torch.float32 else V.coarse_depths(rays, s))
            loss = ((out["rgb_map"] - target.to(dtype)) ** 2).mean()
            gv, gc = torch.autograd.grad(loss, (v, c))
            v, c = (v.detach() - lr * gv).requires_grad_(True), (c.detach() - lr * gc).requires_grad_(True)
            losses.append(float(loss.detach()))
        return v.detach(), c.detach(), torch.tensor(losses, dtype=torch.float64)

    v64, c64, loss64 = cpu_steps(torch.float64)
    v32, c32, loss32 = cpu_steps(torch.float32)
    vol = {"raw": vcpu.to(DEV), "sh": shcpu.to(DEV), "sh_degree": degree, "min_point": LO, "max_point": HI}
    wrp = {"warp": wcpu.to(DEV), "min_point": WLO, "max_point": WHI}
    frames = [(rays.to(DEV), target.to(DEV), 0)]
    new_vol, new_warps, history = F.refine_sh_bake(vol, wrp, frames, steps=steps, lr=lr, optimizer="sgd", N_samples=s)
    torch.cuda.synchronize()
    print(f"  loss {history[0]:.5e} -> {history[-1]:.5e} on the device, {float(loss64[0]):.5e} -> {float(loss64[-1]):.5e} in float64; raw moved by "
          f"up to {float((v64 - vcpu.double()).abs().max()):.3e}, sh by up to {float((c64 - shcpu.double()).abs().max()):.3e}")
    assert len(history) == steps and history[-1] < history[0] and float(loss64[-1]) < float(loss64[0])
    assert bits_equal(vol["raw"].cpu(), vcpu) and bits_equal(vol["sh"].cpu(), shcpu) and bits_equal(new_warps["warp"].cpu(), wcpu)
    assert float((v64 - vcpu.double()).abs().max()) > 1e-3 and float((c64 - shcpu.double()).abs().max()) > 1e-3
    assert worst(torch.tensor(history, dtype=torch.float64), loss64, "losses") <= bar(loss64, loss32, "losses")
    assert worst(new_vol["raw"].cpu(), v64, "refined raw") <= bar(v64, v32, "refined raw")
    assert worst(new_vol["sh"].cpu(), c64, "refined sh") <= bar(c64, c32, "refined sh")
    assert new_vol["sh_degree"] == degree
    only_sh, _, _ = F.refine_sh_bake(vol, wrp, frames, steps=2, lr=lr, optimizer="sgd", params=("sh",), N_samples=s)
    assert bits_equal(only_sh["raw"].cpu(), vcpu) and not bits_equal(only_sh["sh"].cpu(), shcpu)


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    sh = coefficients((5, 4, 3), 2)
    rays, p4 = bent_points(3, 5, 81)
    cot = cotangent((3, 5, 4), 82)
    def refused(*args, **kw):
        with pytest.raises(_lib.NrnerfError) as e:
            sh_backward(*args, **kw)
        assert e.value.status == _lib.ERR_INVALID

    refused(sh, 2, LO, HI, p4, cot, DIFF, d_dirs=False)                                                 # differences: d_points without d_dirs
    refused(sh, 2, LO, HI, p4, cot, DIFF, d_sh=False, d_dirs=False)
    refused(sh, 2, LO, HI, p4, cot, RAY, rays, d_sh=False, d_points=False, d_dirs=False)                # nothing to write
    refused(sh, 0, LO, HI, p4, cot, RAY, rays)
    refused(sh, 3, LO, HI, p4, cot, RAY, rays)
    refused(sh, 2, LO, HI, p4[:, :1].contiguous(), cot[:, :1].contiguous(), DIFF)                       # differences with one sample
    refused(sh, 2, LO, HI, p4, cot, RAY, None)                                                          # the ray rule without rays
    refused(sh, 2, LO, HI, p4, cot, 2, rays)                                                            # an unknown direction mode
    rec = sh_record(2)
    plain = {k: v for k, v in rec.items() if k not in ("sh", "sh_degree")}
    wrp = {"warp": warp_grid((5, 4, 3)).to(DEV), "min_point": WLO, "max_point": WHI}
    pts = p4[..., :3].to(DEV)
    with pytest.raises(R.Unsupported):
        F.sh_lookup(plain, pts)
    with pytest.raises(R.Unsupported):
        F.render_sh_train(plain, wrp, rays.to(DEV), N_samples=5)
    with pytest.raises(R.Unsupported):
        F.refine_sh_bake(plain, wrp, [(rays.to(DEV), torch.zeros(3, 3, device=DEV), 0)], steps=1, lr=1e-2, N_samples=5)
    with pytest.raises(ValueError):
        F.sh_lookup(rec, pts[:, :1])                                                                    # differences with one sample
    with pytest.raises(ValueError):
        F.sh_lookup(rec, pts, rays[:2].to(DEV))
    with pytest.raises(ValueError):
        F.refine_sh_bake(rec, wrp, [(rays.to(DEV), torch.zeros(3, 3, device=DEV), 0)], steps=1, lr=1e-2, params=("sh", "rays"), N_samples=5)
    with pytest.raises(ValueError):
        F.refine_sh_bake(rec, None, [(rays.to(DEV), torch.zeros(3, 3, device=DEV), 0)], steps=1, lr=1e-2, params=("warp",), N_samples=5)
    with pytest.raises(ValueError):
        F.render_sh_train(rec, None, rays.to(DEV), N_samples=5, removal_threshold=0.5)
