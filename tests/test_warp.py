"""GPU tier of the baked warps: ``nrnerf_warped_volume_render`` through ``field.warped_volume_render`` / ``render_baked`` /
``render_baked_frames``, and ``field.bake_warp`` / ``bake_warps``.

1. every output against the float64 reference (tests/warp_reference.py); 2. the fused call's second half IS ``nrnerf_volume_render``: on the
kernel's own ``points4`` that call returns the same bits; 3. the knobs; 4. samples on warp vertices are ``p + m * u`` of torch's float32, bit
for bit (no fma was contracted); 5. ``bake_warp`` holds the query's bits; 6. the accuracy series of tests/test_warp_host.py on the device;
7. frames and refusals.

Tolerances: 10 x the maximum error of the SAME reference evaluated in float32 on the same inputs, computed here and printed."""
import pytest
import torch

from nonrigid_nerf_amd import field as F
from nonrigid_nerf_amd import render as R
from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_scene
from tests import volume_reference as V
from tests import warp_reference as W
from tests.test_warp_host import SERIES_PSNR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO, HI = (-0.5, 0.25, 1.0), (1.5, 1.0, 4.0)                 # the volume's box (tests/test_volume.py)
WLO, WHI = (-0.1, 0.4, 0.5), (1.1, 1.3, 3.2)                # the warp's: partly overlapping -- samples fall outside it, others are bent out of the volume
VOLUME = (17, 9, 33)
WARPS = [(2, 2, 2), (5, 4, 3), (9, 17, 6)]                  # (Gx, Gy, Gz)
RAY_SETS = [(37, 33), (3, 5), (1, 1)]
RAY_NEAR = {(37, 33): 0.5, (3, 5): 0.5, (1, 1): 2.0}          # (one sample of the coarse spacing sits AT near: inside the volume)
RAY_SEED = {(37, 33): 1, (3, 5): 3, (1, 1): 59}             # seeds at which the float32 reference alone has no median tie and every set hits the volume
DTYPES = {"f32": torch.float32, "f16": torch.float16}
MAPS = ("rgb_map", "disp_map", "acc_map", "weights", "alpha")

_grids = {}


def volume(dtype=torch.float32, g=VOLUME, lo=LO, hi=HI):
    """(the volume dictionary on the device, its CPU copy in the storage dtype); built once."""
    key = ("v", g, dtype, lo, hi)
    if key not in _grids:
        cpu = V.smooth_volume(*g, seed=sum(g)).to(dtype)
        _grids[key] = ({"raw": cpu.to(DEV), "min_point": lo, "max_point": hi}, cpu)
    return _grids[key]


def warp(g, dtype=torch.float32, lo=WLO, hi=WHI, amplitude=0.15):
    key = ("w", g, dtype, lo, hi, amplitude)
    if key not in _grids:
        cpu = W.smooth_warp(*g, seed=sum(g), amplitude=amplitude).to(dtype)
        _grids[key] = ({"warp": cpu.to(DEV), "min_point": lo, "max_point": hi}, cpu)
    return _grids[key]


def crossing_rays(n, seed, near=0.5, far=5.0):
    """``n`` rays that cross the box LO .. HI along +z from in front of it, with different direction lengths."""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.5, 0.6, 0.0]) + 0.05 * torch.randn(n, 3, generator=g)
    d = (torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(n, 3, generator=g)) * (0.5 + torch.rand(n, 1, generator=g))
    return torch.cat([o, d, torch.full((n, 1), near), torch.full((n, 1), far)], -1)


def sorted_depths(n, s, seed):
    return torch.sort(0.5 + 4.5 * torch.rand(n, s, generator=torch.Generator().manual_seed(seed)), -1).values


def bar(ref64, ref32, what):
    """10 x the float32 reference's own maximum error."""
    ok = torch.isfinite(ref64) & torch.isfinite(ref32.double())
    err = float((ref32.double() - ref64)[ok].abs().max()) if bool(ok.any()) else 0.0
    print(f"  {what}: float32 reference max error {err:.3e} -> bar {10 * err:.3e}")
    return 10 * err


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def same(a, b):
    """Equal values, NaN equal to NaN (disp_map of a ray that hits nothing is 0 / 0)."""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def bits_same(a, b):
    """Bit for bit (+0 and -0 differ), except that any NaN equals any NaN (disp_map of a ray that hits nothing is 0 / 0)."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


ALL = dict(retraw=True, weights=True, alpha=True, surface=True, return_points=True)


# ---- 1. every output against float64 -----------------------------------------------------------------------------------------------------------
def depth_cases(shape):
    """(name, explicit depths or None, lindisp, white_bkgd): the caller's depths and the coarse spacing; lindisp + white once."""
    n, s = shape
    cases = [("z", sorted_depths(n, s, 11 + n) if s > 1 else torch.full((n, 1), 2.5), False, False), ("coarse", None, False, False)]
    if shape == RAY_SETS[0]:
        cases.append(("coarse lindisp white", None, True, True))
    return cases


def reference_pair(vcpu, wcpu, rays, z, s, lindisp, white, **knobs):
    if z is None:
        z64, z32 = V.coarse_depths(rays, s, lindisp), V.coarse_depths(rays, s, lindisp, torch.float32)
    else:
        z64 = z32 = z
    ref64 = W.render_reference(vcpu, LO, HI, wcpu, WLO, WHI, rays, z64, white_bkgd=white, **knobs)
    ref32 = W.render_reference(vcpu, LO, HI, wcpu, WLO, WHI, rays, z32, white_bkgd=white, dtype=torch.float32, **knobs)
    return ref64, ref32


def check_median(got_idx, ref64, tol, n):
    off = got_idx != ref64["median_index"]
    ties = ref64["median_gap"] <= tol
    excused = off & ties
    print(f"  median_index: {int(off.sum())} of {n} rays differ, {int(excused.sum())} excused; {int(ties.sum())} rays tie within {tol:.3e}")
    assert bool((off == excused).all())
    assert int(excused.sum()) <= 0.01 * n


@pytest.mark.parametrize("wdtype", ["f32", "f16"])
@pytest.mark.parametrize("vdtype", ["f32", "f16"])
@pytest.mark.parametrize("shape", RAY_SETS, ids=["37x33", "3x5", "1x1"])
@pytest.mark.parametrize("wg", WARPS, ids=["2x2x2", "5x4x3", "9x17x6"])
def test_every_output_matches_the_float64_reference(wg, shape, vdtype, wdtype):
    (vol, vcpu), (wrp, wcpu) = volume(DTYPES[vdtype]), warp(wg, DTYPES[wdtype])
    n, s = shape
    rays = crossing_rays(n, RAY_SEED[shape] + wg[0], near=RAY_NEAR[shape])
    for name, z, lindisp, white in depth_cases(shape):
        got = F.warped_volume_render(vol, wrp, rays.to(DEV), N_samples=s, z_vals=None if z is None else z.to(DEV), lindisp=lindisp, white_bkgd=white, **ALL)
        torch.cuda.synchronize()
        got = {k: v.cpu() for k, v in got.items()}
        ref64, ref32 = reference_pair(vcpu, wcpu, rays, z, s, lindisp, white)
        unbent = (ref64["points4"][..., 3] == 0) & (ref64["points4"][..., :3] == ref64["points"]).all(-1)
        empty = (ref64["raw"] == 0).all(-1)
        print(f"[{wg} {shape} volume {vdtype} warp {wdtype}, {name}] {int(unbent.sum())} of {unbent.numel()} samples outside the warp, "
              f"{int(empty.sum())} empty; acc_map up to {float(ref64['acc_map'].max()):.3f}")
        # empty samples and samples the warp does not reach: bit for bit
        assert torch.equal(got["raw"][empty], torch.zeros_like(got["raw"][empty]))
        assert not bool(got["points4"][..., 3][unbent].any())
        if z is not None:                                                              # (the caller's depths: p itself is torch's float32 o + d z)
            assert torch.equal(got["points4"][unbent], ref32["points4"][unbent])
        bars = {}
        for k in ("points4", "raw") + MAPS:
            bars[k] = bar(ref64[k], ref32[k], k)
            g64, r64 = got[k].double(), ref64[k]
            both = torch.isfinite(g64) & torch.isfinite(r64)
            if k != "disp_map":
                assert bool(both.all()), k
            worst = float((g64 - r64)[both].abs().max()) if bool(both.any()) else 0.0
            print(f"  {k}: kernel max error {worst:.3e}")
            assert worst <= bars[k], k
        idx = got["median_index"].long()
        check_median(idx, ref64, bars["acc_map"], n)
        rows = torch.arange(n)
        assert torch.equal(got["surface_pts"], got["points4"][rows, idx, :3]) and torch.equal(got["surface_rigidity"], got["points4"][rows, idx, 3])


# ---- 2. the fused half is the existing kernel ----------------------------------------------------------------------------------------------------
REMOVAL = 0.3            # (the 5 x 4 x 3 warp's rigidity along these rays lies on both sides of it at every S)


@pytest.mark.parametrize("vdtype", ["f32", "f16"])
@pytest.mark.parametrize("S", [1, 2, 33, 64, 65, 129, 193, 257, 385, 513, 769, 1024])
def test_volume_render_on_the_kernels_points4_returns_the_fused_bits(S, vdtype):
    vol, _ = volume(DTYPES[vdtype])
    wrp, _ = warp((5, 4, 3), torch.float16 if S % 2 else torch.float32)
    rays = crossing_rays(5, S).to(DEV)
    for z in (sorted_depths(5, S, S).to(DEV), None):
        fused = F.warped_volume_render(vol, wrp, rays, N_samples=S, z_vals=z, white_bkgd=z is None, removal_threshold=REMOVAL, **ALL)
        again = F.warped_volume_render(vol, wrp, rays, N_samples=S, z_vals=z, white_bkgd=z is None, removal_threshold=REMOVAL, **ALL)
        split = F.volume_render(vol, rays, N_samples=S, z_vals=z, points4=fused["points4"], white_bkgd=z is None, removal_threshold=REMOVAL,
                                retraw=True, weights=True, alpha=True, surface=True)
        torch.cuda.synchronize()
        if S >= 33:
            assert float(fused["acc_map"].max()) > 0.5
            assert bool((fused["points4"][..., 3] >= REMOVAL).any()) and bool((fused["points4"][..., 3] < REMOVAL).any())
        for k in split:
            assert bits_same(fused[k], split[k]), (k, z is None)
        for k in fused:
            assert bits_equal(fused[k], again[k]), k                                  # a repeated call: the same bits
        alone = F.warped_volume_render(vol, wrp, rays, N_samples=S, z_vals=z, removal_threshold=REMOVAL, composite=False, retraw=True, return_points=True)
        assert set(alone) == {"raw", "points4"} and bits_equal(alone["raw"], fused["raw"]) and bits_equal(alone["points4"], fused["points4"])


# ---- 3. the knobs --------------------------------------------------------------------------------------------------------------------------------
KNOB_RAYS, KNOB_S = 37, 65


def knob_setup(wdtype=torch.float32):
    (vol, vcpu), (wrp, wcpu) = volume(), warp((9, 17, 6), wdtype)
    rays = crossing_rays(KNOB_RAYS, 5)
    z = sorted_depths(KNOB_RAYS, KNOB_S, 6)
    return vol, vcpu, wrp, wcpu, rays, z


def run(vol, wrp, rays, z, **kw):
    out = F.warped_volume_render(vol, wrp, rays.to(DEV), N_samples=z.shape[1], z_vals=z.to(DEV), **dict(ALL, **kw))
    torch.cuda.synchronize()
    return out


def test_cutoff_freezes_the_rigid_samples():
    vol, _, wrp, _, rays, z = knob_setup()
    c = 0.5
    plain, cut, still = run(vol, wrp, rays, z), run(vol, wrp, rays, z, rigidity_cutoff=c), run(vol, wrp, rays, z, test_time_scaling=0.0)
    p, m = still["points4"][..., :3], plain["points4"][..., 3]
    frozen = m <= c
    assert bool(frozen.any()) and bool((~frozen).any()) and bool((m[frozen] > 0).any())
    assert bits_equal(cut["points4"][..., :3][frozen], p[frozen]) and not bool(cut["points4"][..., 3][frozen].any())
    assert bits_equal(cut["points4"][~frozen], plain["points4"][~frozen])
    assert bool((plain["points4"][..., :3][frozen] != p[frozen]).any())                # (without the cutoff they do move)


def test_scaling_zero_and_a_zero_warp_are_the_straight_render():
    vol, _, wrp, _, rays, z = knob_setup()
    straight = F.volume_render(vol, rays.to(DEV), N_samples=KNOB_S, z_vals=z.to(DEV), retraw=True, weights=True, alpha=True)
    zero = dict(wrp, warp=torch.zeros_like(wrp["warp"]))
    for got in (run(vol, wrp, rays, z, test_time_scaling=0.0), run(vol, zero, rays, z)):
        for k in straight:
            assert bits_same(got[k], straight[k]), k
    assert not torch.equal(run(vol, wrp, rays, z)["raw"], straight["raw"])
    # the coarse spacing as well
    coarse = F.volume_render(vol, rays.to(DEV), N_samples=KNOB_S, retraw=True)
    got = F.warped_volume_render(vol, zero, rays.to(DEV), N_samples=KNOB_S, retraw=True)
    for k in coarse:
        assert bits_same(got[k], coarse[k]), k


def test_scaling_one_is_no_scaling():
    vol, _, wrp, _, rays, z = knob_setup()
    plain, one = run(vol, wrp, rays, z), run(vol, wrp, rays, z, test_time_scaling=1.0)
    for k in plain:
        assert bits_equal(plain[k], one[k]), k


def test_removal_zeroes_the_sigma_logits_of_the_nonrigid_samples():
    vol, _, wrp, _, rays, z = knob_setup()
    t = 0.6
    plain, gone = run(vol, wrp, rays, z), run(vol, wrp, rays, z, removal_threshold=t)
    kill = plain["points4"][..., 3] >= t
    assert bool(kill.any()) and bool((~kill).any()) and bool((plain["raw"][..., 3][kill] != 0).any())
    assert bool((gone["raw"][..., 3][kill] == 0).all()) and bits_equal(gone["raw"][..., 3][~kill], plain["raw"][..., 3][~kill])
    assert bits_equal(gone["raw"][..., :3], plain["raw"][..., :3]) and bits_equal(gone["points4"], plain["points4"])
    assert not torch.equal(gone["rgb_map"], plain["rgb_map"])


KNOBS_ON = dict(rigidity_cutoff=0.35, test_time_scaling=1.7, removal_threshold=0.65)


def knob_exclusions(wcpu, rays, z, tol=None):
    """Samples whose float64 rigidity lies within the bar of the cutoff or of the threshold (the knobs are discontinuous there), and that bar: 10 x
    the float32 reference's error of the rigidity itself."""
    m64 = W.bend_reference(wcpu, WLO, WHI, W.sample_points(rays, z))[..., 3]
    m32 = W.bend_reference(wcpu, WLO, WHI, W.sample_points(rays, z, torch.float32), dtype=torch.float32)[..., 3]
    tol = bar(m64, m32, "rigidity") if tol is None else tol
    near = ((m64 - KNOBS_ON["rigidity_cutoff"]).abs() <= tol) | ((m64 - KNOBS_ON["removal_threshold"]).abs() <= tol)
    return near, tol


@pytest.mark.parametrize("wdtype", ["f32", "f16"])
def test_knobs_on_match_the_float64_reference(wdtype):
    vol, vcpu, wrp, wcpu, rays, z = knob_setup(DTYPES[wdtype])
    got = {k: v.cpu() for k, v in run(vol, wrp, rays, z, **KNOBS_ON).items()}
    ref64, ref32 = reference_pair(vcpu, wcpu, rays, z, KNOB_S, False, False, **KNOBS_ON)
    near, tol = knob_exclusions(wcpu, rays, z)
    keep_s, keep_r = ~near, ~near.any(-1)
    print(f"[knobs on, warp {wdtype}] {int(near.sum())} of {near.numel()} samples within {tol:.3e} of the cutoff or the threshold, on {int((~keep_r).sum())} rays")
    assert int(near.sum()) <= 0.01 * near.numel()
    m = ref64["points4"][..., 3]
    assert bool((m == 0).any()) and bool((m >= KNOBS_ON["removal_threshold"]).any()) and bool(((m > 0) & (m < KNOBS_ON["removal_threshold"])).any())
    for k in ("points4", "raw") + MAPS:
        keep = keep_s if k in ("points4", "raw") else keep_r
        tol_k = bar(ref64[k][keep], ref32[k][keep], k)
        g64, r64 = got[k].double()[keep], ref64[k][keep]
        both = torch.isfinite(g64) & torch.isfinite(r64)
        worst = float((g64 - r64)[both].abs().max())
        print(f"  {k}: kernel max error {worst:.3e}")
        assert worst <= tol_k, k


# ---- 4. vertices ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdtype", ["f32", "f16"])
def test_samples_on_warp_vertices_are_torchs_p_plus_m_u(wdtype):
    g = (9, 17, 6)
    gx, gy, gz = g
    lo, hi = (0.0, 0.0, 0.0), (gx - 1.0, gy - 1.0, gz - 1.0)                      # unit spacing: a vertex is its index, g_c = p_c exactly
    wrp, wcpu = warp(g, DTYPES[wdtype], lo, hi, amplitude=0.3)
    vol, _ = volume()
    iz, iy = torch.meshgrid(torch.arange(gz, dtype=torch.float32), torch.arange(gy, dtype=torch.float32), indexing="ij")
    n = gy * gz
    col = lambda v: torch.full((n, 1), float(v))
    rays = torch.cat([col(0), iy.reshape(n, 1), iz.reshape(n, 1), col(1), col(0), col(0), col(0), col(gx - 1)], -1)      # along the x-rows
    z = torch.arange(gx, dtype=torch.float32).expand(n, gx).contiguous()
    p = W.grid_vertices(lo, hi, g, torch.float32).reshape(n, gx, 3)
    w = wcpu.float().reshape(n, gx, 4)
    for scaling in (None, 1.5):
        got = F.warped_volume_render(vol, wrp, rays.to(DEV), N_samples=gx, z_vals=z.to(DEV), test_time_scaling=scaling, composite=False,
                                     return_points=True)
        assert set(got) == {"points4"}
        off = w[..., 3:] * w[..., :3]                                               # a product rounded to float32 ...
        if scaling is not None:
            off = off * scaling
        want = torch.cat([p + off, w[..., 3:]], -1)                                 # ... before the sum: an fma would differ
        assert bits_equal(got["points4"].cpu(), want), scaling
        # the render kernel (grid_fetch / grid_value, its own instantiation of the bend) as well as the lookup kernel
        fusedk = F.warped_volume_render(vol, wrp, rays.to(DEV), N_samples=gx, z_vals=z.to(DEV), test_time_scaling=scaling, return_points=True)
        assert bits_equal(fusedk["points4"].cpu(), want), scaling
        fused = (p.double() + w[..., 3:].double() * w[..., :3].double() * (scaling or 1.0)).float()
        if wdtype == "f32":                                                         # (a product of two halves is exact in float32)
            assert bool((fused != want[..., :3]).any())                             # the inputs do tell the two apart
    # the coarse spacing reaches the same vertices: near 0, far Gx - 1, Gx samples
    coarse = F.warped_volume_render(vol, wrp, rays.to(DEV), N_samples=gx, composite=False, return_points=True)
    assert bits_equal(coarse["points4"].cpu()[:, [0, -1]], torch.cat([p + w[..., 3:] * w[..., :3], w[..., 3:]], -1)[:, [0, -1]])


# ---- 5. bake_warp --------------------------------------------------------------------------------------------------------------------------------
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
@pytest.mark.parametrize("depth", [5, 7])
def test_bake_warp_holds_the_querys_bits(depth, precision):
    cfg, scene, rb, coarse, _ = modules(dict(N_importance=0, bend_depth=depth))
    g = (6, 5, 4)
    lat = torch.randn(2, cfg.latent_size, generator=torch.Generator().manual_seed(depth)).to(DEV)
    rows = F.grid_points(LO, HI, g, device=DEV)[..., :3].contiguous()                      # [Gy * Gz, Gx, 3]
    want = []
    for i in range(2):
        _, det = R.query_points(rows, coarse, lat[i:i + 1].expand(rows.shape[0], -1), detailed_output=True, precision=precision)
        want.append(torch.cat([det["unmasked_offsets"], det["rigidity_mask"]], -1).reshape(4, 5, 6, 4))
    torch.cuda.synchronize()
    assert bool((want[0][..., :3] != 0).any()) and not torch.equal(want[0], want[1])
    try:
        # the modules' knobs SET: the bake ignores them and leaves them as they are
        rb.rigidity_test_time_cutoff, rb.test_time_scaling, coarse.test_time_nonrigid_object_removal_threshold = 0.3, 0.5, 0.6
        for rpl in (1, 7):
            b = F.bake_warp({"network_fn": coarse}, lat[0], LO, HI, g, rows_per_launch=rpl, precision=precision)
            assert b["warp"].dtype == torch.float32 and tuple(b["warp"].shape) == (4, 5, 6, 4)
            assert bits_equal(b["warp"], want[0]), rpl
        assert (rb.rigidity_test_time_cutoff, rb.test_time_scaling, coarse.test_time_nonrigid_object_removal_threshold) == (0.3, 0.5, 0.6)
        half = F.bake_warp(coarse, lat[0], LO, HI, g, dtype=torch.float16, precision=precision)          # (a module instead of the dictionary)
        assert half["warp"].dtype == torch.float16 and torch.equal(half["warp"], want[0].half())
        both = F.bake_warps({"network_fn": coarse}, lat, LO, HI, g, precision=precision)
        assert tuple(both["warp"].shape) == (2, 4, 5, 6, 4) and bits_equal(both["warp"][0], want[0]) and bits_equal(both["warp"][1], want[1])
        assert both["min_point"].tolist() == b["min_point"].tolist() and both["max_point"].tolist() == b["max_point"].tolist()
    finally:
        rb.rigidity_test_time_cutoff = rb.test_time_scaling = coarse.test_time_nonrigid_object_removal_threshold = None


def test_bake_warp_refuses_a_network_without_bender():
    cfg, scene, rb, coarse, _ = modules(dict(N_importance=0, bend_depth=5))
    lat = torch.zeros(1, cfg.latent_size, device=DEV)
    with pytest.raises(R.Unsupported):
        F.bake_warp({"network_fn": F.canonical_view(coarse)}, lat, LO, HI, 4)
    _, _, _, baseline, _ = modules(dict(N_importance=0, ray_bending=False, time_conditioned_baseline=True))
    with pytest.raises(R.Unsupported):
        F.bake_warp({"network_fn": baseline}, lat, LO, HI, 4)                           # the time-conditioned baseline has no bender to bake
    with pytest.raises(ValueError):
        F.bake_warp({"network_fn": coarse}, lat, LO, HI, 4, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        F.bake_warp({"network_fn": coarse}, lat, LO, HI, (4, 1, 4))
    with pytest.raises(ValueError):
        F.bake_warps({"network_fn": coarse}, lat[0], LO, HI, 4)


# ---- 6. the accuracy series on the device ----------------------------------------------------------------------------------------------------------
def test_accuracy_series_on_the_device():
    ck, scene, rays, code = V.series_setup()
    rays, code = rays.to(DEV), code.to(DEV)
    kwargs = {"network_fn": ck.network_fn, "network_fine": ck.network_fine}
    lo, hi = V.SERIES_BOX
    vol = F.bake(kwargs, None, lo, hi, W.SERIES_VOLUME, precision="f32")
    exact = F.render_volume(vol, rays, network=ck.network_fine, latents=code, N_samples=V.SERIES_SAMPLES, precision="f32")
    series = {}
    for res in W.SERIES_WARPS:
        wrp = F.bake_warp(kwargs, code, W.SERIES_WARP_BOX[0], W.SERIES_WARP_BOX[1], res, precision="f32")
        out = F.render_baked(vol, wrp, rays, N_samples=V.SERIES_SAMPLES)
        out16 = F.render_baked(vol, dict(wrp, warp=wrp["warp"].half()), rays, N_samples=V.SERIES_SAMPLES)
        torch.cuda.synchronize()
        series[res] = (V.psnr(out["rgb_map"], exact["rgb_map"]), V.psnr(out16["rgb_map"], exact["rgb_map"]), V.psnr(out["acc_map"], exact["acc_map"]))
        print(f"[fitted_latest frame {V.SERIES_FRAME}, volume {W.SERIES_VOLUME}^3 float32, warp {res}^3] PSNR against render_volume(network=...): rgb_map "
              f"float32 warp {series[res][0]:.3f} dB, float16 warp {series[res][1]:.3f} dB, acc_map {series[res][2]:.3f} dB; "
              f"float64 on the host {SERIES_PSNR[res]:.3f} dB")
    for res in W.SERIES_WARPS:
        assert abs(series[res][0] - SERIES_PSNR[res]) <= 0.1, res
        assert abs(series[res][1] - series[res][0]) <= 0.1, res


# ---- 7. frames and refusals ----------------------------------------------------------------------------------------------------------------------
def test_render_baked_frames_and_refusals():
    vol, _ = volume()
    wrp, _ = warp((5, 4, 3))
    other, _ = warp((9, 17, 6))
    poses = [torch.tensor([[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, 0.6], [0.0, 0.0, 1.0, 6.0]]) for _ in range(2)]      # looking down -z at the box
    intrin = dict(height=6, width=8, focal_x=20.0, focal_y=20.0, center_x=4.0, center_y=3.0)
    from nonrigid_nerf_amd.driver import generate_rays
    rays = generate_rays(poses[0], intrin, 1.0, 6.0, False, DEV)
    to8b = lambda x: (255 * x.clamp(0, 1)).to(torch.uint8)
    # one warp for all frames: the dictionary of bake_warp, or a stack of one
    for one in (wrp, dict(wrp, warp=wrp["warp"][None])):
        rgbs, disps = F.render_baked_frames(vol, one, poses, intrin, 1.0, 6.0, N_samples=33)
        assert rgbs.dtype == torch.uint8 and tuple(rgbs.shape) == (2, 6, 8, 3) and tuple(disps.shape) == (2, 6, 8) and disps.dtype == torch.float32
        single = F.render_baked(vol, wrp, rays, N_samples=33)
        assert torch.equal(rgbs[0].view(-1, 3), to8b(single["rgb_map"])) and torch.equal(rgbs[0], rgbs[1]) and int(rgbs.max()) > 0
        assert same(disps[0].view(-1), single["disp_map"])
    # a warp per frame
    grid5 = W.smooth_warp(5, 4, 3, seed=99).to(DEV)
    stack = dict(wrp, warp=torch.stack([wrp["warp"], grid5], 0))
    rgbs, disps = F.render_baked_frames(vol, stack, poses, intrin, 1.0, 6.0, N_samples=33, test_time_scaling=2.0)
    for i, grid in enumerate((wrp["warp"], grid5)):
        single = F.render_baked(vol, dict(wrp, warp=grid), rays, N_samples=33, test_time_scaling=2.0)
        assert torch.equal(rgbs[i].view(-1, 3), to8b(single["rgb_map"])) and same(disps[i].view(-1), single["disp_map"])
    assert not torch.equal(disps[0], disps[1])
    # two identical calls: identical bits
    a, b = (F.render_baked(vol, other, rays, N_samples=33, surface=True, retraw=True, return_points=True, rigidity_cutoff=0.4) for _ in range(2))
    assert set(a) == {"rgb_map", "disp_map", "acc_map", "raw", "surface_pts", "surface_rigidity", "median_index", "points4"}
    for k in a:
        assert bits_equal(a[k], b[k]), k
    # refusals
    with pytest.raises(ValueError):
        F.render_baked_frames(vol, dict(wrp, warp=torch.stack([wrp["warp"]] * 3, 0)), poses, intrin, 1.0, 6.0, N_samples=33)       # 3 warps, 2 frames
    with pytest.raises(ValueError):
        F.render_baked_frames(vol, dict(wrp, warp=wrp["warp"][0]), poses, intrin, 1.0, 6.0, N_samples=33)
    with pytest.raises(R.Unsupported):
        F.render_baked(vol, wrp, rays.clone().requires_grad_(True), N_samples=33)
    with pytest.raises(R.Unsupported):
        F.render_baked(vol, dict(wrp, warp=wrp["warp"].clone().requires_grad_(True)), rays, N_samples=33)
    with pytest.raises(R.Unsupported):
        F.render_baked(dict(vol, raw=vol["raw"].clone().requires_grad_(True)), wrp, rays, N_samples=33)
    with pytest.raises(R.Unsupported):
        F.render_baked(vol, wrp, rays, z_vals=torch.ones(48, 33, device=DEV).requires_grad_(True))
    with torch.no_grad():                                                              # (with autograd off the same inputs are taken)
        assert bits_same(F.render_baked(vol, wrp, rays.clone().requires_grad_(True), N_samples=33)["rgb_map"], F.render_baked(vol, wrp, rays, N_samples=33)["rgb_map"])
    with pytest.raises(R.Unsupported):
        F.render_baked(vol, wrp, rays.cpu(), N_samples=33)
    with pytest.raises(R.Unsupported):
        F.render_baked(vol, dict(wrp, warp=wrp["warp"].cpu()), rays, N_samples=33)
    with pytest.raises(R.Unsupported):
        F.render_baked(dict(vol, raw=vol["raw"].cpu()), wrp, rays, N_samples=33)
    for bad in (wrp["warp"].double(), wrp["warp"][..., :3], wrp["warp"][:1], wrp["warp"][0]):
        with pytest.raises(ValueError):
            F.render_baked(vol, dict(wrp, warp=bad), rays, N_samples=33)
    with pytest.raises(ValueError):
        F.render_baked(vol, dict(wrp, max_point=wrp["min_point"]), rays, N_samples=33)
    with pytest.raises(ValueError):
        F.render_baked(vol, wrp, rays[:, :7], N_samples=33)
    with pytest.raises(ValueError):
        F.render_baked(vol, wrp, rays, z_vals=torch.zeros(3, 33, device=DEV))
    with pytest.raises(ValueError):
        F.render_baked(vol, wrp, rays, N_samples=0)
    with pytest.raises(ValueError):
        F.warped_volume_render(vol, wrp, rays, N_samples=33, composite=False, weights=True)
