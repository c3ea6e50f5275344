"""GPU tier of the field query: ``nrnerf_query`` through ``render.query_points`` / ``render.network_query_fn`` and the grid sampler
``field.sample_grid`` (ABI 10).

1. the query IS the render's own network: fed the render's ``initial_input_pts``, it returns the render's ``raw`` and detail tensors bit for
   bit in fp32 mode (stand-alone point-source bender + trunk-only kernel against the fused kernel);
2. against the reference's own ``network_query_fn`` on non-collinear points (tests/golden/query/query_points.npz);
3. the 16-bit modes at the project's bars (``PRECISION_BARS`` of tests/test_gpu_parity.py);
4. indexing invariances, bit for bit per point; 5. hand-overs; 6. the grid kernels and ``sample_grid``.
"""
import contextlib
import os
import warnings

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import _lib, field as F
from nonrigid_nerf_amd import render as R
from nonrigid_nerf_amd.synthetic import Scene, SceneConfig, build_modules, make_rays, make_scene
from oracle import nrnerf_oracle as O
from tests.helpers import TOL, compare_dict
from tests.test_gpu_parity import PRECISION_BARS
from tests.test_query_host import CASES, load_query_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETAIL_KEYS = ("input_pts", "rigidity_mask", "unmasked_offsets", "masked_offsets")

_built = {}


def modules(cfg_kw, seed=0):
    """(cfg, scene, ray bender, coarse network) of a configuration, built once per module (the handle cache keys on the network object)."""
    key = (tuple(sorted(cfg_kw.items())), seed)
    if key not in _built:
        cfg = SceneConfig(**cfg_kw)
        scene = make_scene(cfg, seed)
        rb, coarse, _ = build_modules(scene, device=DEV)
        for m in (rb, coarse):
            if m is not None:
                m.requires_grad_(False)
        _built[key] = (cfg, scene, rb, coarse)
    return _built[key]


def set_knobs(rb, net, knobs):
    if rb is not None:
        rb.rigidity_test_time_cutoff = knobs.get("rigidity_test_time_cutoff")
        rb.test_time_scaling = knobs.get("test_time_scaling")
    net.test_time_nonrigid_object_removal_threshold = knobs.get("removal_threshold")


def coarse_render(cfg_kw, n_rays, n_samples, seed=0):
    """The fp32 coarse-only render with raw and detail tensors (Model.render: render_rays keeps the reference's UnboundLocalError for
    detailed_output without a fine pass), its rays and latents."""
    cfg, scene, rb, coarse = modules(cfg_kw, seed)
    set_knobs(rb, coarse, {})
    rays, lat = make_rays(n_rays, 11, cfg)
    rays, lat = rays.to(DEV), lat.to(DEV)
    model = R.get_model(coarse, None, precision="f32", device=DEV)
    out = model.render(rays, lat, n_samples, 0, retraw=True, detailed_output=True)
    torch.cuda.synchronize()
    return cfg, coarse, rays, lat, out


SHAPES = [(37, 33), (3, 5)]       # ragged against the 16- and 32-sample blocks; a handful of samples


# ---- 1. the query is the render's own network ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["37x33", "3x5"])
@pytest.mark.parametrize("family", ["default", "deep_bender", "narrow_128", "no_bender"])
def test_query_returns_the_renders_own_bits_in_fp32(family, shape):
    cfg_kw = {"default": dict(N_importance=0), "deep_bender": dict(N_importance=0, bend_depth=7), "narrow_128": dict(N_importance=0, netwidth=128),
              "no_bender": dict(N_importance=0, ray_bending=False)}[family]
    cfg, coarse, rays, lat, out = coarse_render(cfg_kw, *shape)
    raw, det = R.query_points(out["initial_input_pts"], coarse, lat, detailed_output=True, precision="f32")
    torch.cuda.synchronize()
    assert torch.equal(det["initial_input_pts"], out["initial_input_pts"])
    assert torch.equal(raw, out["raw"]), float((raw - out["raw"]).abs().max())
    keys = DETAIL_KEYS if cfg.ray_bending else ("input_pts",)
    assert set(det) == set(keys) | {"initial_input_pts"}
    for k in keys:
        assert torch.equal(det[k], out[k]), (k, float((det[k] - out[k]).abs().max()))


@pytest.mark.parametrize("shape", SHAPES, ids=["37x33", "3x5"])
def test_query_with_view_head_behind_the_bender_in_fp32(shape):
    """sigma and the bender's tensors bit for bit; the colour logits within the <= 1 ulp-scale difference DESIGN.md section 3.3 documents for
    another instantiation of the direction encoding (finite differences from the point array instead of from the neighbouring lanes)."""
    cfg, coarse, rays, lat, out = coarse_render(dict(N_importance=0, use_viewdirs=True), *shape)
    raw, det = R.query_points(out["initial_input_pts"], coarse, lat, detailed_output=True, precision="f32")
    torch.cuda.synchronize()
    assert torch.equal(raw[..., 3], out["raw"][..., 3])
    for k in DETAIL_KEYS:
        assert torch.equal(det[k], out[k]), k
    worst = float((raw[..., :3] - out["raw"][..., :3]).abs().max())
    print(f"[view head + bender, fp32, {shape}] max |colour logit difference| query vs render = {worst:.3e}")
    assert worst <= 1e-6


def test_query_of_a_non_compiled_trunk_in_fp32():
    """--netwidth 192: the run-time-parameterised kernel on both sides (another launch shape): the project's fp32 tolerances."""
    cfg, coarse, rays, lat, out = coarse_render(dict(N_importance=0, netwidth=192), 37, 33)
    raw, det = R.query_points(out["initial_input_pts"], coarse, lat, detailed_output=True, precision="f32")
    torch.cuda.synchronize()
    fails = compare_dict(dict(det, raw=raw), {k: out[k] for k in DETAIL_KEYS + ("raw", "initial_input_pts")})
    assert not fails, "\n".join(fails)


# ---- 2. against the reference's own network_query_fn -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_query_matches_the_reference_on_non_collinear_points(name):
    cfg, scene, knobs, pts, lat, dirs, ref = load_query_case(name)
    _, _, rb, coarse = modules(CASES[name][0])
    set_knobs(rb, coarse, knobs)
    try:
        raw, det = R.query_points(pts.to(DEV), coarse, lat.to(DEV), None if dirs is None else dirs.to(DEV), detailed_output=True, precision="f32")
        torch.cuda.synchronize()
    finally:
        set_knobs(rb, coarse, {})
    got = dict(det, raw=raw)
    assert set(got) == set(ref)
    fails = compare_dict(got, ref)        # per-sample tensors atol / rtol 1e-4, raw 1e-4 of its scale
    assert not fails, "\n".join(fails)


def test_network_query_fn_has_the_references_signature_and_shapes():
    cfg, scene, knobs, pts, lat, dirs, ref = load_query_case("default_knobs")
    _, _, rb, coarse = modules(CASES["default_knobs"][0])
    set_knobs(rb, coarse, {})
    R.set_precision("f32")
    try:
        raw = R.network_query_fn(pts.to(DEV), None, {"ray_bending_latents": lat.to(DEV)}, coarse)
        raw_d, det = R.network_query_fn(pts.to(DEV), None, {"ray_bending_latents": lat.to(DEV)}, coarse, detailed_output=True)
    finally:
        R.set_precision("bf16")
    assert tuple(raw.shape) == tuple(ref["raw"].shape) and torch.equal(raw, raw_d)
    assert {k: tuple(v.shape) for k, v in det.items()} == {k: tuple(v.shape) for k, v in ref.items() if k != "raw"}


# ---- 3. the 16-bit modes at the project's bars -------------------------------------------------------------------------------------------------
def _snr(got, ref):
    err = got.double() - ref.double()
    return [float(20 * torch.log10(ref[..., c].double().std() / err[..., c].pow(2).mean().sqrt())) for c in range(4)]


def _flags_for(precision):
    # "f16": its bars are those of the f16 trunk behind the three-product 32x32x16 bender (tests/test_gpu_parity.py::_same_bender)
    return _lib.RENDER_BENDER_32X32 if precision == "f16" else 0


FAMILIES_16 = {"default": dict(N_importance=0), "no_bender": dict(N_importance=0, ray_bending=False),
               "deep_bender_viewdirs": dict(N_importance=0, bend_depth=7, use_viewdirs=True), "narrow_128": dict(N_importance=0, netwidth=128)}
_points_16 = {}


def _points_and_references(family):
    """4096 rays x 64 samples: the fp32 render's initial_input_pts, the fp32 query and the oracle on the device -- once per family."""
    if family not in _points_16:
        cfg, coarse, rays, lat, out = coarse_render(FAMILIES_16[family], 4096, 64, seed=3)
        pts = out["initial_input_pts"].clone()
        ref32 = R.query_points(pts, coarse, lat, precision="f32")
        _, scene, _, _ = modules(FAMILIES_16[family], 3)
        sc = O.scene_on(scene, DEV)
        with torch.no_grad():
            orc = O.query_network(pts, None, lat, sc.coarse, sc.bender, cfg)
        torch.cuda.synchronize()
        _points_16[family] = (coarse, pts, lat, ref32, orc)
    return _points_16[family]


@pytest.mark.parametrize("precision", ["bf16", "f16"])
@pytest.mark.parametrize("family", list(FAMILIES_16))
def test_16bit_queries_track_the_fp32_query_and_the_oracle(family, precision):
    coarse, pts, lat, ref32, orc = _points_and_references(family)
    got = R.query_points(pts, coarse, lat, precision=precision, flags=_flags_for(precision))
    torch.cuda.synchronize()
    snr, snr_o = _snr(got, ref32), _snr(got, orc)
    print(f"[{family} / {precision}] query raw SNR vs fp32 query {[round(x, 1) for x in snr]} dB, vs oracle {[round(x, 1) for x in snr_o]} dB")
    bar = PRECISION_BARS[precision][0] - 1.5
    assert min(snr) >= bar, snr
    assert min(snr_o) >= bar, snr_o


# ---- 4. indexing invariances: bit for bit per point ------------------------------------------------------------------------------------------
def _scattered_points(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, 3, generator=g) * 2 - 1) * 0.9).to(DEV)


@pytest.mark.parametrize("precision", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("family", ["default", "no_bender"])
def test_a_points_value_does_not_depend_on_where_it_sits(family, precision):
    cfg, scene, rb, coarse = modules(FAMILIES_16[family], 3)
    set_knobs(rb, coarse, {})
    pts = _scattered_points(1008)
    code = (torch.randn(1, cfg.latent_size, generator=torch.Generator().manual_seed(9)) * 0.5).to(DEV)
    q = lambda p, lat, **kw: R.query_points(p, coarse, lat, precision=precision, **kw)
    rows = lambda n: code.expand(n, -1).contiguous()          # per-row latents (stride = latent size)
    base = q(pts.reshape(1, 1008, 3), rows(1)).reshape(1008, -1)
    assert torch.equal(q(pts.reshape(63, 16, 3), rows(63)).reshape(1008, -1), base)
    assert torch.equal(q(pts.reshape(144, 7, 3), rows(144)).reshape(1008, -1), base)
    assert torch.equal(q(pts, code), base)                    # flat: rows of 64, the last one padded
    perm = torch.randperm(1008, generator=torch.Generator().manual_seed(2)).to(DEV)
    assert torch.equal(q(pts[perm].reshape(63, 16, 3), rows(63)).reshape(1008, -1), base[perm])
    # one code for the call (latent_stride 0) against per-row latents
    assert torch.equal(q(pts.reshape(63, 16, 3), code.expand(63, -1)).reshape(1008, -1), base)
    # point_stride 4 against 3
    p4 = torch.cat([pts, torch.full((1008, 1), 7.0, device=DEV)], -1).reshape(63, 16, 4)
    model = R.get_model(coarse, None, precision=precision, device=DEV)
    assert torch.equal(model.query(p4, rows(63) if model.needs_latents else None).reshape(1008, -1), base)
    # fixed against dynamic shares; the same call twice
    assert torch.equal(q(pts.reshape(63, 16, 3), rows(63), flags=_lib.RENDER_FIXED_SHARES).reshape(1008, -1), base)
    assert torch.equal(q(pts.reshape(1, 1008, 3), rows(1)).reshape(1008, -1), base)


def test_more_block_groups_than_the_bender_grid_has_waves():
    """[2049, 70] in bf16 mode: 2049 x 5 blocks of 16 samples > 2 workgroups x 8 waves x 256 CUs x 2 blocks -- every wave loops, the last row
    is ragged: repeated calls agree bit for bit, and the values meet the bar of case 3 against the fp32 query."""
    cfg, scene, rb, coarse = modules(FAMILIES_16["default"], 3)
    set_knobs(rb, coarse, {})
    pts = _scattered_points(2049 * 70, seed=6).reshape(2049, 70, 3)
    lat = (torch.randn(2049, cfg.latent_size, generator=torch.Generator().manual_seed(4)) * 0.5).to(DEV)
    a = R.query_points(pts, coarse, lat, precision="bf16")
    b = R.query_points(pts, coarse, lat, precision="bf16")
    ref = R.query_points(pts, coarse, lat, precision="f32")
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    snr = _snr(a, ref)
    print(f"[2049 x 70, bf16] query raw SNR vs fp32 query {[round(x, 1) for x in snr]} dB")
    assert min(snr) >= PRECISION_BARS["bf16"][0] - 1.5, snr


# ---- 5. hand-overs ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _saved_reference(stub):
    R._fallbacks["network_query_fn"] = stub
    try:
        yield
    finally:
        R._fallbacks.pop("network_query_fn", None)


@pytest.mark.parametrize("case", ["exact_jacobian", "odd_bender", "one_sample_view_head"])
def test_what_the_library_cannot_take_is_handed_over(case):
    cfg_kw, shape = {"exact_jacobian": (dict(N_importance=0, use_viewdirs=True, approx_nonrigid_viewdirs=False), (4, 6)),
                     "odd_bender": (dict(N_importance=0, bend_hidden=96), (4, 6)),
                     "one_sample_view_head": (dict(N_importance=0, use_viewdirs=True), (4, 1))}[case]
    cfg, scene, rb, coarse = modules(cfg_kw)
    pts = _scattered_points(shape[0] * shape[1]).reshape(*shape, 3)
    lat = torch.zeros(shape[0], cfg.latent_size, device=DEV)
    dirs = torch.nn.functional.normalize(torch.ones(shape[0], 3, device=DEV), dim=-1)
    with pytest.raises(R.Unsupported):
        R.query_points(pts, coarse, lat, dirs, precision="f32")
    assert "network_query_fn" not in R._fallbacks
    with pytest.raises(R.Unsupported):
        R.network_query_fn(pts, dirs, {"ray_bending_latents": lat}, coarse)
    seen = []

    def stub(inputs, viewdirs, api, fn, detailed_output=False):
        seen.append((inputs, viewdirs, api, fn, detailed_output))
        return "from the reference"

    R._fallback_seen.clear()
    with _saved_reference(stub), warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert R.network_query_fn(pts, dirs, {"ray_bending_latents": lat}, coarse, detailed_output=True) == "from the reference"
    assert len(seen) == 1 and seen[0][0] is pts and seen[0][3] is coarse and seen[0][4] is True
    assert any(issubclass(x.category, R.FallbackWarning) for x in w)


def test_flat_points_behind_a_view_head_with_bender_are_refused():
    cfg, scene, rb, coarse = modules(dict(N_importance=0, use_viewdirs=True))
    with pytest.raises(ValueError):
        R.query_points(_scattered_points(10), coarse, torch.zeros(1, cfg.latent_size, device=DEV), precision="f32")


# ---- 6. the grid ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [(24, 20, 17), (5, 1, 3), (1, 4, 1)], ids=["24x20x17", "G=1 in y", "G=1 in x and z"])
def test_grid_points_agree_with_the_float64_formula(res):
    lo, hi = np.array([-1.25, 0.3, -2.0]), np.array([0.75, 1.9, 3.5])
    gx, gy, gz = res
    pts = F.grid_points(lo, hi, res, device=DEV).cpu().double().reshape(gz, gy, gx, 4)
    lo32, hi32 = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)
    axis = [lo32[c] + np.arange(g) * ((hi32[c] - lo32[c]) / (g - 1) if g > 1 else 0.0) for c, g in enumerate(res)]
    want = np.stack(np.meshgrid(axis[2], axis[1], axis[0], indexing="ij")[::-1], -1)       # [gz, gy, gx, (x, y, z)]
    bound = 2 * 2.0 ** -23 * max(np.abs(lo32).max(), np.abs(hi32).max())
    err = np.abs(pts[..., :3].numpy() - want).max()
    assert err <= bound, (err, bound)
    assert float(pts[..., 3].abs().max()) == 0.0
    # a slab in the middle is the same rows
    part = F.grid_points(lo, hi, res, first_row=gy * gz // 2, n_rows=gy * gz - gy * gz // 2, device=DEV).cpu().double()
    assert torch.equal(part, pts.reshape(gy * gz, gx, 4)[gy * gz // 2:])


def _field_from_raw_torch(raw):
    sigma = torch.relu(raw[..., 3])
    rgb = (255 * torch.clip(torch.sigmoid(raw[..., :3]), 0, 1)).to(torch.uint8)            # to8b: truncating
    return sigma, rgb


def test_field_from_raw_on_random_logits():
    raw = (torch.randn(5000, 5, generator=torch.Generator().manual_seed(1)) * 6).to(DEV)
    raw[:7, 3] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 80.0, -80.0, 3.0], device=DEV)
    raw[:4, 0] = torch.tensor([100.0, -100.0, 0.0, 17.0], device=DEV)
    sigma, rgb = F.field_from_raw(raw)
    want_s, want_c = _field_from_raw_torch(raw)
    assert torch.equal(sigma, want_s)
    diff = (rgb.int() - want_c.int()).abs()
    print(f"[field_from_raw] 8-bit colours that differ from the torch restatement: {int((diff > 0).sum())} of {diff.numel()} (max {int(diff.max())})")
    assert int(diff.max()) <= 1


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_sample_grid_is_query_points_on_the_grid_and_does_not_depend_on_the_slabs(precision):
    cfg, scene, rb, coarse = modules(FAMILIES_16["default"], 3)
    set_knobs(rb, coarse, {})
    kw = {"network_fn": coarse, "network_fine": None}
    code = (torch.randn(cfg.latent_size, generator=torch.Generator().manual_seed(9)) * 0.5).to(DEV)
    lo, hi, res = (-0.8, -0.7, -0.9), (0.9, 0.6, 0.8), (24, 20, 17)
    every = F.sample_grid(kw, code, lo, hi, res, rows_per_launch=20 * 17, precision=precision)
    assert tuple(every["sigma"].shape) == (17, 20, 24) and tuple(every["rgb"].shape) == (17, 20, 24, 3) and every["rgb"].dtype == torch.uint8
    assert tuple(every["rigidity"].shape) == (17, 20, 24)
    for per in (1, 7):
        got = F.sample_grid(kw, code, lo, hi, res, rows_per_launch=per, precision=precision)
        assert all(torch.equal(got[k], every[k]) for k in ("sigma", "rgb", "rigidity")), per
    pts = F.grid_points(lo, hi, res, device=DEV)
    raw, det = R.query_points(pts[..., :3].contiguous(), coarse, code.reshape(1, -1).expand(20 * 17, -1), detailed_output=True, precision=precision)
    sigma, rgb = F.field_from_raw(raw)
    assert torch.equal(every["sigma"].reshape(-1), sigma.reshape(-1)) and torch.equal(every["rgb"].reshape(-1, 3), rgb.reshape(-1, 3))
    assert torch.equal(every["rigidity"].reshape(-1), det["rigidity_mask"].reshape(-1))


def test_sample_grid_without_bending_is_the_bender_free_models_grid():
    cfg, scene, rb, coarse = modules(FAMILIES_16["default"], 3)
    set_knobs(rb, coarse, {})
    lo, hi, res = (-0.8, -0.7, -0.9), (0.9, 0.6, 0.8), (9, 6, 5)
    got = F.sample_grid({"network_fn": coarse}, None, lo, hi, res, with_bending=False, precision="f32")
    assert set(got) == {"sigma", "rgb"}
    # the same trunk weights as a model that never had a bender
    plain_scene = Scene(SceneConfig(N_importance=0, ray_bending=False), None, scene.coarse, None)
    _, plain, _ = build_modules(plain_scene, device=DEV)
    want = F.sample_grid({"network_fn": plain}, None, lo, hi, res, precision="f32")
    assert torch.equal(got["sigma"], want["sigma"]) and torch.equal(got["rgb"], want["rgb"])
    bent = F.sample_grid({"network_fn": coarse}, torch.zeros(cfg.latent_size), lo, hi, res, precision="f32")
    assert not torch.equal(bent["sigma"], got["sigma"])


def test_density_grid_of_the_fitted_checkpoint_against_the_oracle():
    """tests/golden/fitted_latest.tar, fp32 mode, 24^3 over the scene's box: sigma = relu(raw sigma) against the oracle's query_network at the
    fp32 tolerance of `raw` (1e-4 of its scale, tests/helpers.py).  The checkpoint carries no volume extent (visualize.volume_extent_of
    answers None for it), so the box is the cube of half the far bound around the origin, where the fitted scene lives."""
    from nonrigid_nerf_amd.checkpoint import load_checkpoint
    from nonrigid_nerf_amd.visualize import volume_extent_of
    gold = os.path.join(REPO, "tests", "golden")
    ck = load_checkpoint(os.path.join(gold, "fitted_latest.tar"), N_samples=64, N_importance=128)
    ext = volume_extent_of(ck)
    if ext is None:
        far = float(np.load(os.path.join(gold, "example_sequence_96x72.npz"))["bds"].max())
        ext = (np.full(3, -0.5 * far), np.full(3, 0.5 * far))
    code = ck.latents[3]
    got = F.sample_grid(ck.render_kwargs_test, code, ext[0], ext[1], 24, fine=True, precision="f32")
    sd = lambda m: {k: v.detach().to(DEV) for k, v in m.state_dict().items()}
    pts = F.grid_points(ext[0], ext[1], 24, device=DEV)[..., :3].contiguous()
    cfg = SceneConfig()
    with torch.no_grad():
        raw = O.query_network(pts, None, code.to(DEV).reshape(1, -1).expand(24 * 24, -1), sd(ck.network_fine), sd(ck.ray_bender), cfg)
    want = torch.relu(raw[..., 3]).reshape(24, 24, 24)
    bound = TOL["raw"]["scale_atol"] * float(raw.abs().max())
    err = float((got["sigma"] - want).abs().max())
    print(f"[fitted checkpoint, 24^3, fp32] max |sigma - oracle| = {err:.3e} (bound {bound:.3e}, occupied voxels {int((want > 0).sum())})")
    assert err <= bound
