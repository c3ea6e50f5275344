"""The ray bender's training kernels (csrc/nrnerf_train_bend.h behind nrnerf_bender_forward / _backward / _wgrad and
nrnerf_bender_divergence_forward / _backward), LAYER BY LAYER against float64 (tests/bender_reference.py): every saved array from the
kernel's own saved input to it with an a-priori rounding bound, bent4 bit for bit, the weight-gradient partials added in float64 against
dz^T x over each wave's own range.  No element is excused: every relu mask is the sign of the kernel's own saved activation.

The entry points are called through ctypes.  Every output buffer starts as 0xFF bytes (NaN in bf16 and fp32) with a 4096-byte guard behind
it: every promised element is written, the slot of an empty range is exactly 0, the guards are untouched.  The shapes are the smallest
that reach each mechanism: one valid lane (1 x 1), an odd M below one bf16 chunk (3 x 5), a chunk plus one row (1 x 17), a second block
of one sample (5 x 33), M no multiple of 16 or 32 (77 x 83), and more blocks than the grid has waves, so that the grid-stride loop takes a
second trip; n_partials 4, 64 and 4096 (most ranges empty); ray_stride 11, latent_stride 40 with NaN pad columns, latent_stride 0.

Each test prints the worst residual / bound per array; the module prints the worst over its cases at the end.

Worst residual / bound seen on an MI355X over all cases below.  A bf16 store alone reaches 1 at the bottom of a binade; so does a head
expression that is ONE rounded product (dz_out4 = g_bent mask without knobs, dtz_out4 = g e m): half an ulp is the whole U32 |x| there.
The fp32 chains show how little of the accumulation bound is used.
  bender, fp32:      acts_offsets 0.274, acts_rigidity 0.333, off4.xyz 0.034, off4.w 0.072, dz_out4 0.977, dz_offsets 0.428,
                     dz_rigidity 0.250, d_latents 0.077, dW 0.251, db 0.146
  bender, bf16:      acts_offsets 0.995, acts_rigidity 0.996, off4.xyz 0.569, off4.w 0.694, dz_out4 0.977, dz_offsets 0.996,
                     dz_rigidity 0.996, d_latents 0.550, dW 0.068, db 0.041
  divergence, fp32:  acts_offsets 0.250, acts_rigidity 0.398, off4.xyz 0.032, off4.w 0.103, tacts_offsets 0.451, tacts_rigidity 0.447,
                     toff4.xyz 0.079, toff4.w 0.103, divergence 0.605, tangent 0.742, dz_out4 0.862, dtz_out4 0.978, dz_offsets 0.448,
                     dtz_offsets 0.462, dz_rigidity 0.250, dtz_rigidity 0.250, d_latents 0.097, dW 0.355, db 0.170
  divergence, bf16:  acts_offsets 0.995, acts_rigidity 0.996, off4.xyz 0.500, off4.w 0.655, tacts_offsets 0.996, tacts_rigidity 0.996,
                     toff4.xyz 0.567, toff4.w 0.742, divergence 0.605, tangent 0.742, dz_out4 0.862, dtz_out4 0.978, dz_offsets 0.996,
                     dtz_offsets 0.996, dz_rigidity 0.996, dtz_rigidity 0.996, d_latents 0.550, dW 0.281, db 0.036
  fused call against the separate pair: fp32 0.080, bf16 0.608 of the three calls' bounds
(in bf16 mode off4 and d_latents are fp32 values of a chain whose saved input is only known to bf16: the U16 |saved| |W|^T of the bound
is what they use.)  bent4 was bit for bit in every case, and bent4 / off4 of bend_div_fwd equal bend_fwd_train's bit for bit.
tanhf: allowance 5 ulp, the OpenCL C table's figure for tanh (the toolchain ships no table of the device library's own); it makes up at
most 0.118 of the off4.w bound of an fp32 model (below 0.0005 of a bf16 model's, which the saved input's rounding dominates).

What the first run found: o + d z, written with __fadd_rn / __fmul_rn, compiled to ONE fused multiply-add (those are plain operators in
the toolchain's headers and device code allows contraction): bent4 was not p + fl(mask off) of the two-rounding point in 3 x 5 already.
Fixed in csrc/nrnerf_train_bend.h (mul_rn / add_rn); no empty partial, stride or guard case failed.
"""
import ctypes as C
import functools

import pytest
import torch

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd import render as R
from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_rays, make_scene
from tests import bender_reference as BR
from tests.test_trunk_layers import DEV, Out, _stream

CUTOFF, SCALING = 0.58, 0.7
KNOBS = {"none": BR.Knobs(), "cutoff_scaling": BR.Knobs(CUTOFF, SCALING), "scaling": BR.Knobs(None, SCALING)}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    """the cached modules and handles live as long as this module's tests; the worst figures over all of them are printed at the end"""
    yield
    _handle.cache_clear()
    torch.cuda.empty_cache()
    for key in sorted(_WORST):
        print(f"\n[bender layers, worst over all cases] {key[0]}, {key[1]}: " + ", ".join(f"{g} {v:.3f}" for g, v in _WORST[key].items()))


@functools.lru_cache(maxsize=None)
def _handle(depth, precision):
    """device modules and handle of one bender depth and precision (shared by the cases; never modified after the handle exists: the packed
    images are taken at get_model)"""
    cfg = SceneConfig(N_importance=64, bend_depth=depth)
    rb, coarse, fine = build_modules(make_scene(cfg, 2), device=DEV)
    for m in (rb, coarse, fine):
        m.requires_grad_(False)
    with torch.no_grad():                      # this scene's rigidity saturates at 1: spread the masks around 0.5 so that the cutoff bites
        rb.rigidity_network[-1].weight.mul_(0.02)
        rb.rigidity_network[-1].bias.zero_()
    model = R.get_model(coarse, fine, precision=precision, device=torch.device(DEV))
    assert model.lib.nrnerf_model_trains_bender(model.handle) == 1
    return cfg, rb, model, (coarse, fine)


def _cus():
    return torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count


def _set_knobs(a, kn):
    a.has_rigidity_cutoff, a.rigidity_cutoff = int(kn.cutoff is not None), kn.cutoff or 0.0
    a.has_test_time_scaling, a.test_time_scaling = int(kn.scaling is not None), kn.scaling or 0.0


def _finish(rep, outs, kind, precision, kn, masks, label):
    for name, o in outs.items():
        rep.exact(name, o.guard_ok(), "the guard region behind the buffer was written")
        if name != "partials":          # (of a partial only [out][in] and db[:out] are promised: check_wgrad looks at those)
            rep.exact(name, bool(torch.isfinite(o.t.float()).all()), "an element the header promises was not written")
    share = getattr(rep, "tanh_share", 0.0)
    print(f"\n[{label}] worst residual / bound: {rep.summary().split(';')[0]}; tanhf allowance: at most {share:.3f} of the off4.w bound")
    worst = _WORST.setdefault((kind, precision), {})
    for k, v in rep.ratio.items():
        g = k.split("[")[0].split(" ")[0]
        worst[g] = max(worst.get(g, 0.0), v)
    worst["tanhf share of the off4.w bound"] = max(worst.get("tanhf share of the off4.w bound", 0.0), share)
    if kn.cutoff is not None and masks.numel() >= 100:
        assert float((masks == 0).float().mean()) > 0.02, "the cutoff should bite on this scene"
    assert not rep.failures, rep.failures


def run_bender(precision, depth, n_rays, S, knobs="none", ray_stride=8, latent_stride=32, un=True, mask=True, second=True, n_partials=64):
    """nrnerf_bender_forward, _backward and _wgrad on one ray batch, every array checked.  Returns what the fused-use test needs."""
    cfg, rb, model, _ = _handle(depth, precision)
    kn, b16 = KNOBS[knobs], precision != "f32"
    L, M, RD = cfg.latent_size, n_rays * S, cfg.rigidity_depth
    gen = torch.Generator().manual_seed(1000 * n_rays + S)
    r8, lat = make_rays(n_rays, 5, cfg)
    rays = torch.cat([r8, torch.randn(n_rays, ray_stride - 8, generator=gen)], 1).contiguous().to(DEV)
    latents = torch.cat([lat, torch.full((n_rays, latent_stride - L), float("nan"))], 1).contiguous().to(DEV)
    z = (2.0 + 4.0 * torch.rand(n_rays, S, generator=gen)).sort(-1).values.to(DEV)
    g_bent4, g_bent4_b = (torch.randn(M, 4, generator=gen).to(DEV) for _ in range(2))
    g_un, g_mask = torch.randn(M, 3, generator=gen).to(DEV), torch.randn(M, generator=gen).to(DEV)
    g_bent4_b, g_un, g_mask = g_bent4_b if second else None, g_un if un else None, g_mask if mask else None
    adt = torch.bfloat16 if b16 else torch.float32
    hb, hr = (depth - 1, M, cfg.bend_hidden), (RD - 1, M, cfg.rigidity_hidden)
    o = dict(bent4=Out((M, 4), torch.float32), off4=Out((M, 4), torch.float32), acts_offsets=Out(hb, adt), acts_rigidity=Out(hr, adt),
             dz_offsets=Out(hb, adt), dz_rigidity=Out(hr, adt), dz_out4=Out((M, 4), torch.float32), d_latents=Out((M, L), torch.float32),
             partials=Out((n_partials, depth + RD, BR.SLOT), torch.float32))
    ptr = lambda t: None if t is None else t.data_ptr()
    a = _lib.BenderArgs()
    a.struct_size = C.sizeof(_lib.BenderArgs)
    a.n_rays, a.n_samples = n_rays, S
    a.rays, a.ray_stride, a.latents, a.latent_stride, a.z = rays.data_ptr(), ray_stride, latents.data_ptr(), latent_stride, z.data_ptr()
    _set_knobs(a, kn)
    a.bent4, a.off4, a.acts_offsets, a.acts_rigidity = o["bent4"].ptr, o["off4"].ptr, o["acts_offsets"].ptr, o["acts_rigidity"].ptr
    _lib.check(model.lib.nrnerf_bender_forward(model.handle, C.byref(a), _stream()), "nrnerf_bender_forward")
    a.g_bent4, a.g_bent4_b, a.g_unmasked_offsets, a.g_rigidity_mask = ptr(g_bent4), ptr(g_bent4_b), ptr(g_un), ptr(g_mask)
    a.dz_offsets, a.dz_rigidity, a.dz_out4, a.d_latents = o["dz_offsets"].ptr, o["dz_rigidity"].ptr, o["dz_out4"].ptr, o["d_latents"].ptr
    _lib.check(model.lib.nrnerf_bender_backward(model.handle, C.byref(a), _stream()), "nrnerf_bender_backward")
    wa = _lib.BenderWgradArgs()
    wa.struct_size = C.sizeof(_lib.BenderWgradArgs)
    wa.n_rays, wa.n_samples = n_rays, S
    wa.rays, wa.ray_stride, wa.latents, wa.latent_stride, wa.z = rays.data_ptr(), ray_stride, latents.data_ptr(), latent_stride, z.data_ptr()
    wa.acts_offsets, wa.acts_rigidity = o["acts_offsets"].ptr, o["acts_rigidity"].ptr
    wa.dz_offsets, wa.dz_rigidity, wa.dz_out4 = o["dz_offsets"].ptr, o["dz_rigidity"].ptr, o["dz_out4"].ptr
    wa.n_partials, wa.partials = n_partials, o["partials"].ptr
    _lib.check(model.lib.nrnerf_bender_wgrad(model.handle, C.byref(wa), _stream()), "nrnerf_bender_wgrad")
    torch.cuda.synchronize()

    out = {k: v.t for k, v in o.items()}
    rep = BR.check_bender_forward(rb, b16, kn, rays, z, latents, out)
    BR.check_bender_backward(rb, b16, kn, out, g_bent4, g_bent4_b, g_un, g_mask, rep=rep)
    _, res = BR.check_bender_wgrad(rb, b16, rays, z, latents, out, out["partials"], n_partials, rep=rep)
    _finish(rep, o, "bender", precision, kn, out["bent4"][:, 3],
            f"bender {precision} depth {depth} ({n_rays}, {S}) knobs {knobs} strides {ray_stride}/{latent_stride} partials {n_partials}")
    given = dict(points=BR.points_fp32(rays, z), latents=BR.per_sample(latents, S, L).contiguous(),
                 cot=dict(g_bent4=g_bent4, g_bent4_b=g_bent4_b, g_unmasked=g_un, g_mask=g_mask))
    return out, res, given


# n_rays (None: more blocks than 2 CUs x 4 waves), S, n_partials
SHAPES = [(1, 1, 4096), (3, 5, 4), (1, 17, 64), (5, 33, 64), (77, 83, 64), (None, 33, 4096)]
SHAPE_IDS = ["one_lane", "odd_m_below_a_chunk", "a_chunk_and_a_row", "second_block_of_one_sample", "ragged", "second_trip"]


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays,S,n_partials", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("depth", [5, 7])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_bender_forward_backward_wgrad_layer_by_layer(precision, depth, n_rays, S, n_partials):
    if n_rays is None:
        n_rays = 8 * _cus() // 2 + 6
        assert n_rays * ((S + 31) // 32) > 2 * _cus() * 4
    run_bender(precision, depth, n_rays, S, n_partials=n_partials)


# (the cutoff cases run the 5-layer bender: on rays its masks lie in 0.52 .. 0.71 and the cutoff 0.58 takes three in four; the 7-layer
# bender's lie in 0.39 .. 0.51 there and are all cut -- the divergence tests' points leave one in a hundred of them uncut)
VARIANTS = {
    "wide_strides_all_cotangents_cutoff_4_partials": dict(depth=5, knobs="cutoff_scaling", ray_stride=11, latent_stride=40, n_partials=4),
    "wide_rays_no_optional_cotangent_scaling_4096_partials": dict(depth=7, knobs="scaling", ray_stride=11, un=False, mask=False, second=False, n_partials=4096),
    "wide_latents_no_mask_cotangent_4096_partials": dict(depth=7, latent_stride=40, mask=False, n_partials=4096),
    "mask_cotangent_alone_cutoff": dict(depth=5, knobs="cutoff_scaling", un=False, second=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS))
@pytest.mark.parametrize("n_rays,S", [(5, 33), (77, 83)])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_bender_strides_null_cotangents_knobs_and_partial_counts(precision, n_rays, S, variant):
    run_bender(precision, n_rays=n_rays, S=S, **VARIANTS[variant])


def run_divergence(precision, depth, n_points, knobs="none", latent_stride=32, tangent=False, render=(), bent4=False, n_partials=64, given=None):
    """nrnerf_bender_divergence_forward and _backward on independent points, every array checked.  render: which of the render pass'
    cotangents are handed in (g_bent4, g_bent4_b, g_unmasked, g_mask).  given: points, latents [M, L] and cotangents of a bender call to
    use instead of random ones."""
    cfg, rb, model, _ = _handle(depth, precision)
    kn, b16 = KNOBS[knobs], precision != "f32"
    L, M, RD = cfg.latent_size, n_points, cfg.rigidity_depth
    gen = torch.Generator().manual_seed(7 * n_points + depth)
    points = (torch.randn(M, 3, generator=gen) * torch.tensor([0.8, 0.8, 2.0])).to(DEV)
    probe = torch.randn(M, 3, generator=gen).to(DEV)
    rows = M if latent_stride else 1
    width = latent_stride or L
    latents = torch.cat([torch.randn(rows, L, generator=gen) * 0.1, torch.full((rows, width - L), float("nan"))], 1).contiguous().to(DEV)
    lat = latents[:, :L].expand(M, L) if not latent_stride else latents[:, :L]
    g_div, g_tan = torch.randn(M, generator=gen).to(DEV), torch.randn(M, 3, generator=gen).to(DEV)
    cot = dict(g_bent4=torch.randn(M, 4, generator=gen), g_bent4_b=torch.randn(M, 4, generator=gen), g_unmasked=torch.randn(M, 3, generator=gen),
               g_mask=torch.randn(M, generator=gen))
    cot = {k: (v.to(DEV) if k in render else None) for k, v in cot.items()}
    if given is not None:
        points, latents, lat = given["points"], given["latents"], given["latents"]
        cot = {k: (v if k in render else None) for k, v in given["cot"].items()}
    adt = torch.bfloat16 if b16 else torch.float32
    hb, hr = (depth - 1, M, cfg.bend_hidden), (RD - 1, M, cfg.rigidity_hidden)
    o = dict(divergence=Out((M,), torch.float32), off4=Out((M, 4), torch.float32), toff4=Out((M, 4), torch.float32),
             dz_out4=Out((M, 4), torch.float32), dtz_out4=Out((M, 4), torch.float32), d_latents=Out((M, L), torch.float32),
             partials=Out((n_partials, depth + RD + 1, BR.SLOT), torch.float32))
    for nm, shape in (("offsets", hb), ("rigidity", hr)):
        for pre in ("acts", "tacts", "dz", "dtz"):
            o[f"{pre}_{nm}"] = Out(shape, adt)
    if tangent:
        o["tangent"] = Out((M, 3), torch.float32)
    if bent4:
        o["bent4"] = Out((M, 4), torch.float32)
    ptr = lambda t: None if t is None else t.data_ptr()
    a = _lib.DivergenceArgs()
    a.struct_size = C.sizeof(_lib.DivergenceArgs)
    a.n_points, a.points, a.latents, a.latent_stride, a.probe = M, points.data_ptr(), latents.data_ptr(), latent_stride, probe.data_ptr()
    _set_knobs(a, kn)
    for k in ("divergence", "off4", "toff4", "acts_offsets", "tacts_offsets", "acts_rigidity", "tacts_rigidity"):
        setattr(a, k, o[k].ptr)
    a.tangent, a.bent4 = (o["tangent"].ptr if tangent else None), (o["bent4"].ptr if bent4 else None)
    _lib.check(model.lib.nrnerf_bender_divergence_forward(model.handle, C.byref(a), _stream()), "nrnerf_bender_divergence_forward")
    a.g_divergence, a.g_tangent = (None if tangent else g_div.data_ptr()), (g_tan.data_ptr() if tangent else None)
    for k in ("dz_offsets", "dtz_offsets", "dz_rigidity", "dtz_rigidity", "dz_out4", "dtz_out4", "d_latents", "partials"):
        setattr(a, k, o[k].ptr)
    a.n_partials = n_partials
    a.render_g_bent4, a.render_g_bent4_b = ptr(cot["g_bent4"]), ptr(cot["g_bent4_b"])
    a.render_g_unmasked_offsets, a.render_g_rigidity_mask = ptr(cot["g_unmasked"]), ptr(cot["g_mask"])
    _lib.check(model.lib.nrnerf_bender_divergence_backward(model.handle, C.byref(a), _stream()), "nrnerf_bender_divergence_backward")
    torch.cuda.synchronize()

    out = {k: v.t for k, v in o.items()}
    rep = BR.check_divergence_forward(rb, b16, kn, points, lat, probe, out)
    _, res = BR.check_divergence_backward(rb, b16, kn, points, lat, probe, out, None if tangent else g_div, g_tan if tangent else None, cot,
                                          partials=out["partials"], n_partials=n_partials, rep=rep)
    masks, _ = BR.mask_fp32(out["off4"][:, 3], kn)
    _finish(rep, o, "divergence", precision, kn, masks,
            f"divergence {precision} depth {depth} {n_points} points knobs {knobs} latent stride {latent_stride} "
            f"{'tangent' if tangent else 'divergence'} render {sorted(render)} bent4 {bent4} partials {n_partials}")
    return out, res, dict(points=points, lat=lat, probe=probe, g_div=g_div, cot=cot)


DIV_VARIANTS = {
    "alone": dict(),
    "one_code_tangent_fused_with_the_render_pass_cutoff_4096_partials":
        dict(knobs="cutoff_scaling", latent_stride=0, tangent=True, render=("g_bent4", "g_bent4_b", "g_unmasked", "g_mask"), bent4=True, n_partials=4096),
    "wide_latents_fused_two_cotangents_scaling_4_partials":
        dict(knobs="scaling", latent_stride=40, render=("g_bent4", "g_mask"), bent4=True, n_partials=4),
}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(DIV_VARIANTS), ids=list(DIV_VARIANTS))
@pytest.mark.parametrize("n_points", [1, 33, 5063, None], ids=["1", "33", "5063", "second_trip"])
@pytest.mark.parametrize("depth", [5, 7])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_divergence_forward_backward_wgrad_layer_by_layer(precision, depth, n_points, variant):
    if n_points is None:
        n_points = 32 * 4 * 2 * _cus() + 77
    run_divergence(precision, depth, n_points, **DIV_VARIANTS[variant])


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays,S", [(3, 11), (61, 83)])
@pytest.mark.parametrize("knobs", ["none", "cutoff_scaling"])
@pytest.mark.parametrize("depth", [5, 7])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fused_divergence_backward_equals_the_separate_pair(precision, depth, knobs, n_rays, S):
    """The route training takes by default: ONE nrnerf_bender_divergence_backward with the render pass' cotangents, against
    nrnerf_bender_backward + nrnerf_bender_wgrad together with nrnerf_bender_divergence_backward without them, on the same samples:
    every parameter gradient and the latent rows within the three calls' bounds (bender_reference.check_fused_against_pair)."""
    _, rb, _, _ = _handle(depth, precision)
    every = ("g_bent4", "g_bent4_b", "g_unmasked", "g_mask")
    bender = run_bender(precision, depth, n_rays, S, knobs=knobs)
    fused = run_divergence(precision, depth, n_rays * S, knobs=knobs, render=every, bent4=True, given=bender[2])
    alone = run_divergence(precision, depth, n_rays * S, knobs=knobs, given=bender[2])
    same = BR.bits_equal(fused[0]["bent4"], bender[0]["bent4"]) and BR.bits_equal(fused[0]["off4"], bender[0]["off4"])
    print(f"\n[fused vs pair] bent4 and off4 of the two forward kernels bit for bit: {same}")
    f = fused[2]
    assert torch.equal(f["probe"], alone[2]["probe"]) and torch.equal(f["g_div"], alone[2]["g_div"])
    rep = BR.check_fused_against_pair(BR.Report(), rb, precision != "f32", KNOBS[knobs], f["points"], f["lat"], f["probe"], f["g_div"], f["cot"],
                                      fused[:2], bender[:2], alone[:2])
    print(f"\n[fused vs pair {precision} depth {depth} ({n_rays}, {S}) knobs {knobs}] worst residual / bound: {rep.worst('fused vs pair'):.3f}")
    worst = _WORST.setdefault(("fused vs pair", precision), {})
    worst["gradients"] = max(worst.get("gradients", 0.0), rep.worst("fused vs pair"))
    assert not rep.failures, rep.failures
