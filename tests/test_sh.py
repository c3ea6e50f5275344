"""GPU tier of the view-dependent bakes: ``nrnerf_sh_volume_render`` through ``field.sh_volume_render`` / ``render_baked`` / ``render_volume``,
and ``field.bake(sh_degree=...)``.

1. every output against the float64 reference (tests/sh_reference.py), degrees 1 and 2, float32 and half storage, the three sources of the
bent points, one S per lane width; 2. anchors to shipped code: with zero coefficients the call IS ``render_baked`` / ``render_volume`` /
``volume_render`` on ``"raw"``, and a degree-2 record whose degree-2 coefficients are zero IS the degree-1 record; 3. bit identities: the
lookup kernel, the call on its own ``points4``, two runs; 4. ``bake``: the projection of the query's own outputs; 5. refusals.

Tolerances: 10 x the maximum error of the SAME reference evaluated in float32 on the same inputs, computed here and printed."""
import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import field as F
from nonrigid_nerf_amd import render as R
from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_scene
from tests import sh_reference as SH
from tests import volume_reference as V
from tests import warp_reference as W
from tests.test_warp import DEV, DTYPES, HI, LO, VOLUME, WHI, WLO, bar, bits_same, crossing_rays, same, sorted_depths, volume, warp

pytestmark = pytest.mark.gpu
WARP = (5, 4, 3)
MAPS = ("rgb_map", "disp_map", "acc_map", "weights", "alpha")
ALL = dict(retraw=True, weights=True, alpha=True, surface=True, return_points=True)
# (rays, samples): one S per lane width, each with a finite-difference pair across a lane boundary (S > 64: lane l ends at sample l * EPL - 1);
# the larger ones at 3 rays; a wave quartet does not divide 37.  The seed of a shape: one at which the float32 reference ALONE picks the
# float64 reference's median sample on every ray, in every case of the shape (a condition of the inputs, asserted below on the CPU)
SHAPES = [(37, 2), (37, 65), (37, 130), (37, 193), (3, 257), (3, 385), (3, 513), (3, 769), (1, 33)]
SEED = {(37, 2): 1, (37, 65): 1, (37, 130): 1, (37, 193): 1, (3, 257): 1, (3, 385): 3, (3, 513): 2, (3, 769): 1, (1, 33): 2}
PATHS = ("warp", "points4", "straight")

_records = {}


def record_cpu(degree, dtype, zero_from=None):
    """The CPU copies of a record's raw and sh in the storage dtype; ``zero_from``: the coefficients of basis functions k >= zero_from are zero."""
    vcpu = V.smooth_volume(*VOLUME, seed=sum(VOLUME)).to(dtype)                       # (tests/test_warp.py's volume)
    sh = SH.smooth_sh(*VOLUME, 2, seed=5)[..., :12 * degree].clone()                 # (degree 1: the first nine channels of degree 2's)
    if degree == 1:
        sh[..., 9:] = 0
    if zero_from is not None:
        sh[..., 3 * (zero_from - 1):] = 0
    return vcpu, sh.to(dtype)


def record(degree, dtype, zero_from=None):
    """(the volume record with "sh" on the device, the CPU copies of raw and sh in the storage dtype); built once."""
    key = (degree, dtype, zero_from)
    if key not in _records:
        vol, vcpu = volume(dtype)
        _, sh = record_cpu(degree, dtype, zero_from)
        _records[key] = (dict(vol, sh=sh.to(DEV), sh_degree=degree), vcpu, sh)
    return _records[key]


def warp_cpu(wdtype):
    return W.smooth_warp(*WARP, seed=sum(WARP), amplitude=0.15).to(wdtype)            # (tests/test_warp.py's warp)


def case_inputs(shape, path, wdtype=torch.float32, seed=None):
    """rays, explicit depths (None on the straight path: the coarse spacing), the warp's CPU grid or None, points4 or None."""
    n, s = shape
    rays = crossing_rays(n, (SEED[shape] if seed is None else seed) + s)
    z = None if path == "straight" else sorted_depths(n, s, 11 + n + s)
    wcpu = p4 = None
    if path != "straight":
        wcpu = warp_cpu(wdtype)
    if path == "points4":          # ready-made bent points: the float32 rule's own, as a bender kernel would hand them over
        p4 = W.bend_reference(wcpu, WLO, WHI, W.sample_points(rays, z, torch.float32), dtype=torch.float32)
    return rays, z, wcpu, p4


def reference_pair(vcpu, shcpu, degree, shape, path, rays, z, wcpu, p4, **kw):
    s = shape[1]
    z64, z32 = (V.coarse_depths(rays, s), V.coarse_depths(rays, s, False, torch.float32)) if z is None else (z, z)
    src = dict(warp=wcpu, warp_min=WLO, warp_max=WHI) if path == "warp" else dict(points4=p4) if path == "points4" else {}
    ref64 = SH.render_reference(vcpu, shcpu, degree, LO, HI, rays, z64, **src, **kw)
    ref32 = SH.render_reference(vcpu, shcpu, degree, LO, HI, rays, z32, dtype=torch.float32, **src, **kw)
    return ref64, ref32


def run(rec, rays, s, z, wdtype, p4, path, **kw):
    dev = lambda t: None if t is None else t.to(DEV)
    out = F.sh_volume_render(rec, dev(rays), N_samples=s, z_vals=dev(z), warp=warp(WARP, wdtype)[0] if path == "warp" else None,
                             points4=dev(p4) if path == "points4" else None, **kw)
    torch.cuda.synchronize()
    return out


# ---- 1. every output against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{s}" for n, s in SHAPES])
def test_every_output_matches_the_float64_reference(shape, degree, storage, path):
    rec, vcpu, shcpu = record(degree, DTYPES[storage])
    n, s = shape
    rays, z, wcpu, p4 = case_inputs(shape, path, DTYPES[storage])
    kw = dict(white_bkgd=degree == 2, removal_threshold=0.3 if path != "straight" else None)
    ref64, ref32 = reference_pair(vcpu, shcpu, degree, shape, path, rays, z, wcpu, p4, **kw)
    # the condition on the seed: the float32 reference alone has no median tie
    assert torch.equal(ref32["median_index"], ref64["median_index"]), "pick another seed for this shape"
    got = {k: v.cpu() for k, v in run(rec, rays, s, z, DTYPES[storage], p4, path, **kw, **ALL).items()}
    empty = (V.lookup_reference(vcpu, LO, HI, ref64["points4"][..., :3]) == 0).all(-1)
    print(f"[{shape} degree {degree} {storage} {path}] {int(empty.sum())} of {empty.numel()} samples empty; acc_map up to "
          f"{float(ref64['acc_map'].max()):.3f}; the colour logits move by up to {float((ref64['raw'] - V.lookup_reference(vcpu, LO, HI, ref64['points4'][..., :3]))[..., :3].abs().max()):.2f}")
    assert float(ref64["acc_map"].max()) > 0.5 and not bool(empty.all())
    assert torch.equal(got["raw"][empty], torch.zeros_like(got["raw"][empty]))                  # an empty sample: raw = 0 and v = 0
    for k in ("points4", "raw") + MAPS:
        tol = bar(ref64[k], ref32[k], k)
        g64, r64 = got[k].double(), ref64[k]
        both = torch.isfinite(g64) & torch.isfinite(r64)
        if k != "disp_map":
            assert bool(both.all()), k
        worst = float((g64 - r64)[both].abs().max()) if bool(both.any()) else 0.0
        print(f"  {k}: kernel max error {worst:.3e}")
        assert worst <= tol, k
    idx = got["median_index"].long()
    assert torch.equal(idx, ref64["median_index"])
    rows = torch.arange(n)
    assert torch.equal(got["surface_pts"], got["points4"][rows, idx, :3]) and torch.equal(got["surface_rigidity"], got["points4"][rows, idx, 3])
    tol = bar(ref64["surface_pts"], ref32["surface_pts"], "surface_pts")
    assert float((got["surface_pts"].double() - ref64["surface_pts"]).abs().max()) <= tol


def test_the_ray_direction_rule_on_bent_points_and_differences_on_straight_rays():
    """The mode is a field of the call: either rule on either source of points."""
    rec, vcpu, shcpu = record(2, torch.float32)
    shape = (37, 65)
    for path, ray_directions in (("warp", True), ("straight", False)):
        rays, z, wcpu, p4 = case_inputs(shape, path)
        ref64, ref32 = reference_pair(vcpu, shcpu, 2, shape, path, rays, z, wcpu, p4, ray_directions=ray_directions)
        got = run(rec, rays, shape[1], z, torch.float32, p4, path, ray_directions=ray_directions, retraw=True)
        for k in ("raw", "rgb_map"):
            assert float((got[k].cpu().double() - ref64[k]).abs().max()) <= bar(ref64[k], ref32[k], f"{path} {k}")


# ---- 2. anchors to shipped code --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("S", [2, 65, 130, 193, 257, 385, 513, 769, 1024])
def test_zero_coefficients_give_the_shipped_calls_values(S, storage):
    """A degree-1 record with zero coefficients: ``render_baked`` / ``volume_render`` / ``render_volume`` on ``"raw"``, every key, ``==`` with
    NaN equal to NaN."""
    rec0, _, _ = record(1, DTYPES[storage], zero_from=1)
    plain = {k: v for k, v in rec0.items() if k not in ("sh", "sh_degree")}
    wrp, wcpu = warp(WARP, DTYPES[storage])
    n = 5
    rays = crossing_rays(n, S).to(DEV)
    z = sorted_depths(n, S, S).to(DEV)
    knobs = dict(rigidity_cutoff=0.2, test_time_scaling=1.5, removal_threshold=0.3)
    for zz in (z, None):
        want = F.render_baked(plain, wrp, rays, N_samples=S, z_vals=zz, white_bkgd=True, surface=True, retraw=True, return_points=True, **knobs)
        got = F.render_baked(rec0, wrp, rays, N_samples=S, z_vals=zz, white_bkgd=True, surface=True, retraw=True, return_points=True, **knobs)
        assert sorted(got) == sorted(want)
        for k in want:
            assert same(got[k], want[k]), ("render_baked", k)
    kw = dict(retraw=True, weights=True, alpha=True, surface=True)
    want = F.volume_render(plain, rays, N_samples=S, z_vals=z, points4=want["points4"], removal_threshold=0.3, **kw)
    got = F.sh_volume_render(rec0, rays, N_samples=S, z_vals=z, points4=got["points4"], removal_threshold=0.3, **kw)
    assert sorted(got) == sorted(want)
    for k in want:
        assert same(got[k], want[k]), ("volume_render", k)
    want = F.render_volume(plain, rays, N_samples=S, surface=True, retraw=True)
    got = F.render_volume(rec0, rays, N_samples=S, surface=True, retraw=True)
    assert sorted(got) == sorted(want)
    for k in want:
        assert same(got[k], want[k]), ("render_volume", k)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("S", [2, 193, 769])
def test_a_degree_2_record_with_zero_degree_2_coefficients_is_the_degree_1_record(S, path):
    rec1, _, _ = record(1, torch.float32)
    rec2, _, sh2 = record(2, torch.float32, zero_from=4)
    assert bool((sh2[..., :9] != 0).any()) and torch.equal(sh2[..., :9].to(DEV), rec1["sh"][..., :9])
    rays, z, wcpu, p4 = case_inputs((3, S), path, seed=1)
    a = run(rec1, rays, S, z, torch.float32, p4, path, **ALL)
    b = run(rec2, rays, S, z, torch.float32, p4, path, **ALL)
    for k in a:
        assert same(a[k], b[k]), k


# ---- 3. bit identities -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("S", [2, 65, 130, 193, 257, 385, 513, 769, 1024])
def test_lookup_kernel_own_points4_and_two_runs_give_the_same_bits(S, degree, storage):
    rec, _, _ = record(degree, DTYPES[storage])
    wrp, _ = warp(WARP, torch.float16 if S % 2 else torch.float32)
    rays = crossing_rays(5, S).to(DEV)
    knobs = dict(rigidity_cutoff=0.2, test_time_scaling=1.5, removal_threshold=0.3)
    for z in (sorted_depths(5, S, S).to(DEV), None):
        fused = F.sh_volume_render(rec, rays, N_samples=S, z_vals=z, warp=wrp, white_bkgd=z is None, **knobs, **ALL)
        again = F.sh_volume_render(rec, rays, N_samples=S, z_vals=z, warp=wrp, white_bkgd=z is None, **knobs, **ALL)
        split = F.sh_volume_render(rec, rays, N_samples=S, z_vals=z, points4=fused["points4"], white_bkgd=z is None, removal_threshold=0.3, **ALL)
        alone = F.sh_volume_render(rec, rays, N_samples=S, z_vals=z, warp=wrp, composite=False, retraw=True, return_points=True, **knobs)
        alone_p4 = F.sh_volume_render(rec, rays, N_samples=S, z_vals=z, points4=fused["points4"], composite=False, retraw=True, removal_threshold=0.3)
        for ray_directions in (True, False):
            a = F.sh_volume_render(rec, rays, N_samples=S, z_vals=z, ray_directions=ray_directions, retraw=True)
            b = F.sh_volume_render(rec, rays, N_samples=S, z_vals=z, ray_directions=ray_directions, composite=False)
            assert bits_same(a["raw"], b["raw"]), ("straight", ray_directions)
        torch.cuda.synchronize()
        assert sorted(fused) == sorted(split) == sorted(again)
        for k in fused:
            eq = torch.equal if k == "median_index" else bits_same
            assert eq(fused[k], again[k]), ("two runs", k)
            assert eq(fused[k], split[k]), ("own points4", k)
        assert sorted(alone) == ["points4", "raw"] and bits_same(alone["raw"], fused["raw"]) and bits_same(alone["points4"], fused["points4"])
        assert bits_same(alone_p4["raw"], fused["raw"])
        assert bool((fused["raw"][..., :3] != 0).any())


# ---- 4. bake ---------------------------------------------------------------------------------------------------------------------------------------
_built = {}


def modules(ray_bending):
    if ray_bending not in _built:
        cfg = SceneConfig(N_importance=0, use_viewdirs=True, ray_bending=ray_bending)
        scene = make_scene(cfg, 2)
        rb, coarse, fine = build_modules(scene, device=DEV)
        for m in (rb, coarse, fine):
            if m is not None:
                m.requires_grad_(False)
        _built[ray_bending] = (cfg, coarse)
    return _built[ray_bending]


@pytest.mark.parametrize("ray_bending", [False, True], ids=["no bender", "behind a bender (canonical view)"])
def test_bake_is_the_projection_of_the_querys_outputs(ray_bending):
    cfg, net = modules(ray_bending)
    g = (9, 5, 7)
    kwargs = {"network_fn": net}
    rows = F.grid_points(LO, HI, g, device=DEV)[..., :3].contiguous()                      # [Gy * Gz, Gx, 3]
    dirs = torch.from_numpy(F.SH_DIRECTIONS).float().to(DEV)
    f = torch.stack([R.query_points(rows, F.canonical_view(net), None, dirs[d:d + 1].expand(rows.shape[0], -1), precision="f32")
                     for d in range(26)], 0).cpu()                                          # [26, rows, Gx, 4]
    assert float((f[1:, ..., :3] - f[0, ..., :3]).abs().max()) > 1e-3                       # (the head does depend on the direction)
    w, Y = SH.lebedev_26()[1], SH.basis(SH.lebedev_26()[0], 2)
    absf = f[..., :3].double().abs()
    for degree in (1, 2):
        mean64, sh64 = SH.bake_reference(f[..., :3], degree)
        first = None
        for rpl in (None, 1, 4):
            b = F.bake(kwargs, None, LO, HI, g, rows_per_launch=rpl, precision="f32", sh_degree=degree)
            assert b["sh_degree"] == degree and tuple(b["raw"].shape) == (7, 5, 9, 4) and tuple(b["sh"].shape) == (7, 5, 9, 12 * degree)
            if first is None:
                first = b
            assert torch.equal(b["raw"], first["raw"]) and torch.equal(b["sh"], first["sh"]), rpl          # bit-independent of the slab size
        raw, sh = first["raw"].cpu().view(35, 9, 4), first["sh"].cpu().view(35, 9, 12 * degree)
        assert torch.equal(raw[..., 3], f[0, ..., 3])                                       # sigma: the first direction's query bits
        bound0 = 64 * 2.0 ** -24 * torch.einsum("d,d...->...", w, absf)
        print(f"[degree {degree}, bender {ray_bending}] mean: max error {float((raw[..., :3].double() - mean64).abs().max()):.3e}, bar min {float(bound0.min()):.3e}")
        assert bool(((raw[..., :3].double() - mean64).abs() <= bound0).all())
        K = (degree + 1) ** 2
        bound = 64 * 2.0 ** -24 * 4 * np.pi * torch.einsum("d,dk,d...c->...kc", w, Y[:, 1:K].abs(), absf).reshape(35, 9, 3 * (K - 1))
        err = (sh[..., :3 * (K - 1)].double() - sh64[..., :3 * (K - 1)]).abs()
        print(f"  coefficients: max error {float(err.max()):.3e}, largest coefficient {float(sh64.abs().max()):.3e}")
        assert bool((err <= bound).all()) and float(sh64.abs().max()) > 1e-3
        assert not bool(sh[..., 3 * (K - 1):].any())
        half = F.bake(kwargs, None, LO, HI, g, dtype=torch.float16, precision="f32", sh_degree=degree)
        assert half["sh"].dtype == half["raw"].dtype == torch.float16
        assert torch.equal(half["raw"], first["raw"].half()) and torch.equal(half["sh"], first["sh"].half())       # the float32 bake rounded once
        errh = (half["sh"].cpu().view(35, 9, -1)[..., :3 * (K - 1)].double() - sh64[..., :3 * (K - 1)]).abs()
        assert bool((errh <= bound + 2.0 ** -11 * sh64[..., :3 * (K - 1)].abs()).all())
    zero = F.bake(kwargs, None, LO, HI, g, precision="f32", sh_degree=0)
    assert "sh" not in zero and zero["sh_degree"] == 0 and torch.equal(zero["raw"], first["raw"])
    # the record renders: with a warp and without
    rays = crossing_rays(7, 3).to(DEV)
    out = F.render_volume(first, rays, N_samples=33)
    assert bool(torch.isfinite(out["rgb_map"]).all())
    wrp, _ = warp(WARP)
    out = F.render_baked(first, wrp, rays, N_samples=33, surface=True)
    assert bool(torch.isfinite(out["rgb_map"]).all()) and "surface_pts" in out


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_sh_degree_3_is_refused():
    _, net = modules(False)
    with pytest.raises(ValueError):
        F.bake({"network_fn": net}, None, LO, HI, 4, sh_degree=3)


def test_sh_degree_on_a_plain_head_is_refused():
    cfg = SceneConfig(N_importance=0)
    _, coarse, _ = build_modules(make_scene(cfg, 0), device=DEV)
    with pytest.raises(ValueError):
        F.bake({"network_fn": coarse}, None, LO, HI, 4, sh_degree=1)


def test_with_bending_behind_a_bender_is_refused():
    cfg, net = modules(True)
    lat = torch.zeros(1, cfg.latent_size, device=DEV)
    with pytest.raises(R.Unsupported):
        F.bake({"network_fn": net}, lat, LO, HI, 4, with_bending=True, sh_degree=1)


def test_an_sh_of_the_wrong_shape_or_dtype_is_refused():
    rec, _, _ = record(2, torch.float32)
    rays = crossing_rays(3, 1).to(DEV)
    for bad in (rec["sh"][..., :12].contiguous(), rec["sh"][:-1].contiguous(), rec["sh"].half(), rec["sh"].double()):
        with pytest.raises(ValueError):
            F.render_volume(dict(rec, sh=bad), rays, N_samples=5)
    with pytest.raises(ValueError):
        F.render_volume(dict(rec, sh_degree=3), rays, N_samples=5)


def test_gradients_of_an_sh_record_are_refused():
    rec, _, _ = record(1, torch.float32)
    wrp, _ = warp(WARP)
    rays = crossing_rays(3, 1).to(DEV)
    with pytest.raises(R.Unsupported):
        F.render_baked_train(rec, wrp, rays, N_samples=5)
    with pytest.raises(R.Unsupported):
        F.grid_lookup(rec, LO, HI, rays[:, :3])
    with pytest.raises(R.Unsupported):
        F.refine_bake(rec, wrp, [(rays, torch.zeros(3, 3, device=DEV), 0)], steps=1, lr=1e-2, N_samples=5)


def test_bake_of_a_view_dependent_head_without_sh_degree_still_raises():
    _, net = modules(False)
    with pytest.raises(R.Unsupported):
        F.bake({"network_fn": net}, None, LO, HI, 4)
