"""GPU tier of the baked volumes: ``nrnerf_volume_render`` / ``nrnerf_bend_points`` through ``field.volume_render``, ``Model.bend_points``,
``field.bake`` and ``field.render_volume``.

1. the lookup alone against the float64 reference (tests/volume_reference.py), vertices and empty samples bit for bit;
2. the fused kernel's maps are ``nrnerf_composite_forward``'s on the kernel's own ``raw`` output, bit for bit (that entry point runs
   ``composite_kernel``, which composites with ``composite_ray`` -- csrc/nrnerf_composite.hip -- the device function the fused kernel calls);
3. every output against the float64 reference; 4. ``nrnerf_bend_points`` returns the query's bits; 5. ``bake``; 6. the resolution series of
   tests/test_volume_host.py on the device.

Tolerances: 10 x the maximum error of the SAME reference evaluated in float32 on the same inputs, computed here and printed."""
import ctypes as C

import pytest
import torch

from nonrigid_nerf_amd import _lib, field as F
from nonrigid_nerf_amd import render as R
from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_scene
from tests import volume_reference as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO, HI = (-0.5, 0.25, 1.0), (1.5, 1.0, 4.0)
VOLUMES = [(2, 2, 2), (5, 4, 3), (17, 9, 33)]           # (Gx, Gy, Gz), all different in the last one: every axis mix-up shows
POINT_SHAPES = [(37, 33), (3, 5), (1, 1)]

_volumes = {}


def volume(g, dtype=torch.float32, lo=LO, hi=HI):
    """(the volume dictionary on the device, its CPU copy in the storage dtype) of a seeded smooth volume; built once."""
    key = (g, dtype, lo, hi)
    if key not in _volumes:
        cpu = V.smooth_volume(*g, seed=sum(g)).to(dtype)
        _volumes[key] = ({"raw": cpu.to(DEV), "min_point": lo, "max_point": hi}, cpu)
    return _volumes[key]


def dummy_rays(n):
    return torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 2.0], device=DEV).repeat(n, 1)


def lookup(vol, pts):
    """``pts [N, S, 3]`` -> the kernel's logits ``[N, S, 4]`` (the stand-alone lookup kernel: no maps are asked for)."""
    p4 = torch.cat([pts, torch.zeros_like(pts[..., :1])], -1).to(DEV)
    out = F.volume_render(vol, dummy_rays(p4.shape[0]), N_samples=p4.shape[1], points4=p4, composite=False)
    torch.cuda.synchronize()
    assert set(out) == {"raw"}
    return out["raw"].cpu()


def bar(ref64, ref32, what):
    """10 x the float32 reference's own maximum error."""
    ok = torch.isfinite(ref64) & torch.isfinite(ref32.double())
    err = float((ref32.double() - ref64)[ok].abs().max()) if bool(ok.any()) else 0.0
    print(f"  {what}: float32 reference max error {err:.3e} -> bar {10 * err:.3e}")
    return 10 * err


# ---- 1. the lookup alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", POINT_SHAPES, ids=["37x33", "3x5", "1x1"])
@pytest.mark.parametrize("g", VOLUMES, ids=["2x2x2", "5x4x3", "17x9x33"])
def test_lookup_matches_the_float64_reference(g, shape, dtype):
    vol, cpu = volume(g, dtype)
    pts = V.interior_points(shape, LO, HI, seed=shape[0] + g[0])
    got = lookup(vol, pts)
    ref64, ref32 = V.lookup_reference(cpu, LO, HI, pts), V.lookup_reference(cpu, LO, HI, pts, torch.float32)
    empty = (ref64 == 0).all(-1)
    print(f"[lookup {g} {dtype} {shape}] {int(empty.sum())} of {empty.numel()} samples empty")
    assert torch.equal(got[empty], torch.zeros_like(got[empty]))                       # empty samples: exact zeros
    tol = bar(ref64, ref32, "raw")
    worst = float((got.double() - ref64).abs().max())
    print(f"  kernel max error {worst:.3e}")
    assert worst <= tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("g", VOLUMES, ids=["2x2x2", "5x4x3", "17x9x33"])
def test_lookup_at_vertices_and_outside_is_bit_exact(g, dtype):
    gx, gy, gz = g
    lo, hi = (0.0, 0.0, 0.0), (gx - 1.0, gy - 1.0, gz - 1.0)                          # unit spacing: a vertex is its index, g_c = p_c exactly
    vol, cpu = volume(g, dtype, lo, hi)
    zz, yy, xx = torch.meshgrid(torch.arange(gz), torch.arange(gy), torch.arange(gx), indexing="ij")
    verts = torch.stack([xx, yy, zz], -1).float().reshape(gz * gy, gx, 3)
    got = lookup(vol, verts)
    assert torch.equal(got.reshape(gz, gy, gx, 4), cpu.float())
    nan, inf = float("nan"), float("inf")
    outside = torch.tensor([[nan, 0.5, 0.5], [0.5, nan, 0.5], [0.5, 0.5, nan], [nan, nan, nan], [inf, 0.5, 0.5], [0.5, -inf, 0.5],
                            [-1e-3, 0.5, 0.5], [0.5, gy - 1 + 1e-3, 0.5], [0.5, 0.5, gz - 1 + 1e-3], [0.5, 0.5, 0.5]]).reshape(2, 5, 3)
    got = lookup(vol, outside).reshape(10, 4)
    assert torch.equal(got[:9], torch.zeros(9, 4))
    # the tenth point is inside: seven lerps of two roundings each on logits below 9 stay within 9 * 14 * 2^-24 = 7.5e-6
    assert float((got[9].double() - V.lookup_reference(cpu, lo, hi, outside.reshape(10, 3)[9:])[0]).abs().max()) <= 1e-5


# ---- 2. fused equals split --------------------------------------------------------------------------------------------------------------------
def crossing_rays(n, seed, near=0.5, far=5.0):
    """``n`` rays that cross the box LO .. HI along +z from in front of it, with different direction lengths."""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.5, 0.6, 0.0]) + 0.05 * torch.randn(n, 3, generator=g)
    d = (torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(n, 3, generator=g)) * (0.5 + torch.rand(n, 1, generator=g))
    return torch.cat([o, d, torch.full((n, 1), near), torch.full((n, 1), far)], -1)


def composite_forward(rays, raw, z, lindisp, white_bkgd):
    n, s = raw.shape[:2]
    out = {k: torch.empty(shape, dtype=torch.float32, device=DEV) for k, shape in (("rgb_map", (n, 3)), ("disp_map", (n,)), ("acc_map", (n,)),
                                                                                     ("weights", (n, s)), ("alpha", (n, s)))}
    a = _lib.CompositeArgs()
    a.struct_size = C.sizeof(_lib.CompositeArgs)
    a.n_rays, a.n_samples, a.rays, a.ray_stride, a.raw4 = n, s, rays.data_ptr(), rays.shape[1], raw.data_ptr()
    a.z, a.lindisp, a.white_bkgd = (None if z is None else z.data_ptr()), int(lindisp), int(white_bkgd)
    a.rgb, a.disp, a.acc, a.weights, a.alpha = (out[k].data_ptr() for k in ("rgb_map", "disp_map", "acc_map", "weights", "alpha"))
    _lib.check(_lib.load().nrnerf_composite_forward(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nrnerf_composite_forward")
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("explicit_z", [False, True], ids=["linspace", "z"])
@pytest.mark.parametrize("S", [2, 33, 64, 65, 257, 1024])
def test_fused_maps_are_the_composite_kernels_on_the_fused_raw(S, explicit_z, dtype):
    vol, _ = volume((17, 9, 33), dtype)
    rays = crossing_rays(5, S).to(DEV)
    for lindisp, white in ((False, False), (True, True), (False, True)):
        z = None
        if explicit_z:
            g = torch.Generator().manual_seed(S)
            z = torch.sort(0.5 + 4.5 * torch.rand(5, S, generator=g), -1).values.to(DEV)
        kw = dict(N_samples=S, z_vals=z, lindisp=lindisp, white_bkgd=white, retraw=True, weights=True, alpha=True)
        fused = F.volume_render(vol, rays, **kw)
        again = F.volume_render(vol, rays, **kw)
        split = composite_forward(rays, fused["raw"], z, lindisp, white)
        torch.cuda.synchronize()
        if S >= 33:
            assert float(fused["acc_map"].max()) > 0.5                                   # (something is hit; two samples may both miss the box)
        for k in ("rgb_map", "disp_map", "acc_map", "weights", "alpha"):
            same = (fused[k] == split[k]) | (torch.isnan(fused[k]) & torch.isnan(split[k]))
            assert bool(same.all()), (k, lindisp, white, float((fused[k] - split[k]).abs().max()))
        for k in fused:
            assert fused[k].view(torch.int32).equal(again[k].view(torch.int32)), k     # a repeated call: the same bits
        alone = F.volume_render(vol, rays, N_samples=S, z_vals=z, lindisp=lindisp, composite=False)      # the stand-alone lookup kernel
        assert set(alone) == {"raw"} and torch.equal(alone["raw"], fused["raw"])


# ---- 3. the maps against float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", ["points4_removal_300x65", "straight_37x33", "straight_lindisp_white_5x257"])
def test_maps_match_the_float64_reference(case, dtype):
    vol, cpu = volume((17, 9, 33), dtype)
    n, s = {"points4_removal_300x65": (300, 65), "straight_37x33": (37, 33), "straight_lindisp_white_5x257": (5, 257)}[case]
    lindisp = white = case.startswith("straight_lindisp")
    rays = crossing_rays(n, n + s)
    p4, removal = None, None
    if case.startswith("points4"):
        # wobbling sample points (what a bender returns) with a rigidity column, explicit depths
        g = torch.Generator().manual_seed(7)
        z = torch.sort(0.5 + 4.5 * torch.rand(n, s, generator=g), -1).values
        pts = rays[:, None, :3] + rays[:, None, 3:6] * z[..., None] + 0.02 * torch.randn(n, s, 3, generator=g)
        p4, removal = torch.cat([pts, torch.rand(n, s, 1, generator=g)], -1), 0.8
        zr64 = zr32 = z
    else:
        z = None
        zr64, zr32 = V.coarse_depths(rays, s, lindisp), V.coarse_depths(rays, s, lindisp, torch.float32)
    got = F.volume_render(vol, rays.to(DEV), N_samples=s, z_vals=None if z is None else z.to(DEV), points4=None if p4 is None else p4.to(DEV),
                          lindisp=lindisp, white_bkgd=white, removal_threshold=removal, retraw=True, weights=True, alpha=True, surface=p4 is not None)
    torch.cuda.synchronize()
    ref64 = V.render_reference(cpu, LO, HI, rays, zr64, p4, white_bkgd=white, removal_threshold=removal)
    ref32 = V.render_reference(cpu, LO, HI, rays, zr32, p4, white_bkgd=white, removal_threshold=removal, dtype=torch.float32)
    print(f"[{case} {dtype}] acc_map from {float(ref64['acc_map'].min()):.3f} to {float(ref64['acc_map'].max()):.3f}")
    bars = {}
    for k in ("raw", "rgb_map", "disp_map", "acc_map", "weights", "alpha"):
        bars[k] = bar(ref64[k], ref32[k], k)
        g64, r64 = got[k].cpu().double(), ref64[k]
        both = torch.isfinite(g64) & torch.isfinite(r64)
        if k != "disp_map":
            assert bool(both.all()), k
        worst = float((g64 - r64)[both].abs().max())
        print(f"  {k}: kernel max error {worst:.3e}")
        assert worst <= bars[k], k
    if p4 is not None:
        idx = got["median_index"].cpu().long()
        off = idx != ref64["median_index"]
        excused = off & (ref64["median_gap"] <= bars["acc_map"])
        ties = int((ref64["median_gap"] <= bars["acc_map"]).sum())
        print(f"  median_index: {int(off.sum())} of {n} rays differ, {int(excused.sum())} excused; {ties} rays ({100 * ties / n:.2f} %) tie within {bars['acc_map']:.3e}")
        assert bool((off == excused).all())
        assert int(excused.sum()) <= 0.01 * n
        rows = torch.arange(n)
        assert torch.equal(got["surface_pts"].cpu(), p4[rows, idx, :3]) and torch.equal(got["surface_rigidity"].cpu(), p4[rows, idx, 3])
        kill = p4[..., 3] >= removal
        assert bool((got["raw"].cpu()[..., 3][kill] == 0).all()) and bool(kill.any()) and bool((~kill).any())


# ---- 4. nrnerf_bend_points ------------------------------------------------------------------------------------------------------------------------
_built = {}


def modules(cfg_kw, seed=0):
    key = (tuple(sorted(cfg_kw.items())), seed)
    if key not in _built:
        cfg = SceneConfig(**cfg_kw)
        scene = make_scene(cfg, seed)
        rb, coarse, fine = build_modules(scene, device=DEV)
        for m in (rb, coarse, fine):
            if m is not None:
                m.requires_grad_(False)
        _built[key] = (cfg, scene, rb, coarse, fine)
    return _built[key]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("shape", POINT_SHAPES, ids=["37x33", "3x5", "1x1"])
@pytest.mark.parametrize("depth", [5, 7])
def test_bend_points_returns_the_querys_bits(depth, shape, precision):
    cfg, scene, rb, coarse, _ = modules(dict(N_importance=0, bend_depth=depth))
    n, s = shape
    g = torch.Generator().manual_seed(depth + n)
    pts = ((torch.rand(n, s, 3, generator=g) * 2 - 1) * 1.5).to(DEV)
    lat_rows = torch.randn(n, cfg.latent_size, generator=g).to(DEV)
    model = R.get_model(coarse, None, precision=precision, device=DEV)
    try:
        for knobs in ({}, dict(rigidity_test_time_cutoff=0.3, test_time_scaling=0.5)):
            rb.rigidity_test_time_cutoff, rb.test_time_scaling = knobs.get("rigidity_test_time_cutoff"), knobs.get("test_time_scaling")
            kn = R._query_knobs(coarse)
            for lat in (lat_rows, lat_rows[:1].contiguous().expand(n, -1)):                 # a code per row; one code for the call
                for flags in (0, _lib.RENDER_BENDER_32X32, _lib.RENDER_FIXED_SHARES, _lib.RENDER_BENDER_32X32 | _lib.RENDER_FIXED_SHARES):
                    bent4 = model.bend_points(pts, lat, rigidity_cutoff=kn["rigidity_cutoff"], test_time_scaling=kn["test_time_scaling"], flags=flags)
                    _, det = R.query_points(pts, coarse, lat, detailed_output=True, precision=precision, flags=flags)
                    torch.cuda.synchronize()
                    where = (knobs, lat.stride(0), flags)
                    assert torch.equal(bent4[..., :3], det["input_pts"]), where
                    assert torch.equal(bent4[..., 3:], det["rigidity_mask"]), where
                    if not knobs:
                        assert bool((bent4[..., :3] != pts).any()), where                   # (the bender does move the points; a cutoff may freeze one)
    finally:
        rb.rigidity_test_time_cutoff = rb.test_time_scaling = None


# ---- 5. bake -----------------------------------------------------------------------------------------------------------------------------------------
def test_bake_holds_the_querys_logits():
    cfg, scene, rb, coarse, fine = modules(dict(N_importance=64))
    kwargs = {"network_fn": coarse, "network_fine": fine}
    g = (5, 4, 3)
    rows = F.grid_points(LO, HI, g, device=DEV)[..., :3].contiguous()                      # [Gy * Gz, Gx, 3]
    want = R.query_points(rows, F.canonical_view(fine), None, precision="f32")
    assert want.shape[-1] == 5                                                           # (output_ch 5: the bake keeps the first four)
    for rpl in (None, 1, 7):
        b = F.bake(kwargs, None, LO, HI, g, rows_per_launch=rpl, precision="f32")
        assert b["raw"].dtype == torch.float32 and tuple(b["raw"].shape) == (3, 4, 5, 4)
        assert torch.equal(b["raw"].view(12, 5, 4), want[..., :4]), rpl
    half = F.bake(kwargs, None, LO, HI, g, dtype=torch.float16, precision="f32")
    assert half["raw"].dtype == torch.float16 and torch.equal(half["raw"], b["raw"].half())
    # the observed space of one time step
    lat = torch.randn(1, cfg.latent_size, generator=torch.Generator().manual_seed(1)).to(DEV)
    bent = F.bake(kwargs, lat, LO, HI, g, with_bending=True, precision="f32")
    want_b = R.query_points(rows, fine, lat.expand(rows.shape[0], -1), precision="f32")
    assert torch.equal(bent["raw"].view(12, 5, 4), want_b[..., :4]) and not torch.equal(bent["raw"], b["raw"])
    # the coarse network on request
    assert not torch.equal(F.bake(kwargs, None, LO, HI, g, fine=False, precision="f32")["raw"], b["raw"])


def test_bake_refuses_a_view_dependent_head():
    cfg, scene, rb, coarse, fine = modules(dict(N_importance=0, use_viewdirs=True))
    with pytest.raises(R.Unsupported):
        F.bake({"network_fn": coarse}, None, LO, HI, 4)


# ---- 6. end to end on the fitted checkpoint --------------------------------------------------------------------------------------------------------
def test_resolution_series_on_the_device():
    ck, scene, rays, code = V.series_setup()
    rays, code = rays.to(DEV), code.to(DEV)
    n = rays.shape[0]
    kwargs = {"network_fn": ck.network_fn, "network_fine": ck.network_fine}
    R.set_precision("f32")
    try:
        with torch.no_grad():
            net = R.batchify_rays(rays, {"ray_bending_latents": code.expand(n, -1)}, network_fn=ck.network_fn, network_fine=ck.network_fine,
                                  N_samples=64, N_importance=128)
    finally:
        R.set_precision("bf16")
    lo, hi = V.SERIES_BOX
    series = {}
    for res in (24, 48, 96):
        vol = F.bake(kwargs, None, lo, hi, res, precision="f32")
        out = F.render_volume(vol, rays, network=ck.network_fine, latents=code, N_samples=V.SERIES_SAMPLES, precision="f32")
        out16 = F.render_volume(dict(vol, raw=vol["raw"].half()), rays, network=ck.network_fine, latents=code, N_samples=V.SERIES_SAMPLES, precision="f32")
        torch.cuda.synchronize()
        series[res] = (V.psnr(out["rgb_map"], net["rgb_map"]), V.psnr(out16["rgb_map"], net["rgb_map"]), V.psnr(out["acc_map"], net["acc_map"]),
                       V.psnr(out16["rgb_map"], out["rgb_map"]))
        print(f"[fitted_latest frame {V.SERIES_FRAME}, {res}^3] PSNR against the 64 + 128 network render: rgb_map float32 {series[res][0]:.2f} dB, "
              f"float16 {series[res][1]:.2f} dB, acc_map {series[res][2]:.2f} dB; float16 against float32 storage {series[res][3]:.1f} dB")
    assert series[48][0] >= series[24][0] + 1.0
    assert series[96][0] >= series[48][0] + 1.0
    for res in series:
        assert abs(series[res][1] - series[res][0]) <= 0.1, res
    # test_time_scaling 0 switches the bender's offsets off: the bent samples are the straight ones, bit for bit
    rb = R._bender_of(ck.network_fine)
    try:
        rb.test_time_scaling = 0.0
        still = F.render_volume(vol, rays, network=ck.network_fine, latents=code, N_samples=V.SERIES_SAMPLES, retraw=True, precision="f32")
    finally:
        rb.test_time_scaling = None
    straight = F.render_volume(vol, rays, N_samples=V.SERIES_SAMPLES, retraw=True)
    torch.cuda.synchronize()
    assert torch.equal(still["raw"], straight["raw"])
    assert not torch.equal(still["raw"], F.render_volume(vol, rays, network=ck.network_fine, latents=code, N_samples=V.SERIES_SAMPLES, retraw=True,
                                                         precision="f32")["raw"])
    print(f"  test_time_scaling 0: raw equals the straight-ray render; PSNR of that render against the network's {V.psnr(straight['rgb_map'], net['rgb_map']):.2f} dB")


def test_render_volume_frames_and_refusals():
    vol, _ = volume((17, 9, 33))
    poses = [torch.tensor([[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, 0.6], [0.0, 0.0, 1.0, 6.0]]) for _ in range(2)]      # looking down -z at the box
    intrin = dict(height=6, width=8, focal_x=20.0, focal_y=20.0, center_x=4.0, center_y=3.0)
    rgbs, disps = F.render_volume_frames(vol, poses, intrin, 1.0, 6.0, N_samples=33)
    assert rgbs.dtype == torch.uint8 and tuple(rgbs.shape) == (2, 6, 8, 3) and tuple(disps.shape) == (2, 6, 8) and disps.dtype == torch.float32
    from nonrigid_nerf_amd.driver import generate_rays
    rays = generate_rays(poses[0], intrin, 1.0, 6.0, False, DEV)
    one = F.render_volume(vol, rays, N_samples=33)
    assert torch.equal(rgbs[0].view(-1, 3), (255 * one["rgb_map"].clamp(0, 1)).to(torch.uint8)) and torch.equal(rgbs[0], rgbs[1])
    assert int(rgbs.max()) > 0
    # straight rays with the surface outputs: the samples themselves stand in for the bent points (rigidity 0)
    surf = F.render_volume(vol, rays, N_samples=33, surface=True, retraw=True)
    assert set(surf) == {"rgb_map", "disp_map", "acc_map", "raw", "surface_pts", "surface_rigidity", "median_index"}
    assert torch.equal(surf["rgb_map"], one["rgb_map"]) and tuple(surf["raw"].shape) == (48, 33, 4)
    idx = surf["median_index"].long()
    assert int(idx.min()) >= 0 and int(idx.max()) <= 32 and not bool(surf["surface_rigidity"].any())
    z, pts = F.sample_rays(rays, 33)
    assert torch.equal(surf["surface_pts"], pts[torch.arange(48, device=DEV), idx])
    with pytest.raises(R.Unsupported):
        F.render_volume(vol, rays.clone().requires_grad_(True), N_samples=33)
    with pytest.raises(R.Unsupported):
        F.render_volume(dict(vol, raw=vol["raw"].cpu()), rays, N_samples=33)
