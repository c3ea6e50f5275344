"""Native training path (nonrigid_nerf_amd/training.py over nrnerf_trunk_* / nrnerf_composite_*): gradients against the
REFERENCE's autograd (tests/golden/gradients_64_64.npz, produced by oracle/make_golden.py::run_gradients from the
unmodified reference) and against the oracle's autograd on larger, stochastic batches; device-side weight refresh; a
short optimisation run."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nonrigid_nerf_amd import render as R
from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_rays, make_scene
from tests.helpers import GOLDEN_DIR

DEV = "cuda:0"


def _modules(scene, requires_grad=True):
    rb, coarse, fine = build_modules(scene, device=DEV)
    for m in (rb, coarse, fine):
        if m is not None:
            m.requires_grad_(requires_grad)
    return rb, coarse, fine


def _named(rb, coarse, fine):
    out = {}
    for part, mod in (("bender", rb), ("coarse", coarse), ("fine", fine)):
        if mod is not None:
            for k, p in mod.named_parameters():
                out[(part, k)] = p
    return out


@pytest.fixture
def torch_ops_bender():
    """The bender as torch ops on the module's parameters: reproduces the reference's bent points bit for bit, which the
    tight gradient comparisons below need (behind the bent point sits the 2^9-frequency encoding: an ulp there moves the
    bender / latent gradients by 1e-2 of their scale; see the golden test's docstring)."""
    from nonrigid_nerf_amd import training
    old = (training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER)
    # (and the fine pass bends all S + I merged points in one call, like the reference's graph: a library GEMM's result for a
    #  row can change by an ulp with the batch it is part of, so re-using the coarse pass' points would not be bit-identical)
    training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = False, False, False
    yield
    training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = old


@pytest.mark.gpu
@pytest.mark.parametrize("fixture,cfg_kw", [("gradients_64_64", {}), ("gradients_viewdirs_64_64", dict(use_viewdirs=True)),
                                            ("gradients_exact_viewdirs_64_64", dict(use_viewdirs=True, approx_nonrigid_viewdirs=False)),
                                            ("gradients_time_conditioned_64_64", dict(ray_bending=False, time_conditioned_baseline=True)),
                                            # a NON-COMPILED architecture (oracle/make_golden.py GRAD_CFG_GENERIC): the run-time-parameterised forward /
                                            # backward-data programs, nrnerf_tn_products and the encoding kernels against the REFERENCE's autograd
                                            ("gradients_generic_192_320_64_64", dict(netdepth=6, netwidth=192, netwidth_fine=320, multires=8, skips=(2,)))],
                         ids=["default", "viewdirs", "exact_viewdirs", "time_conditioned", "generic_192_320"])
def test_gradients_match_reference_autograd_golden(torch_ops_bender, fixture, cfg_kw):
    """fp32 mode: d(sum rgb_map + sum rgb0) wrt the latent codes and a few parameters of every network, against what the
    reference's own autograd produced on the CPU (train.render under grad, z_samples detached).

    Two facts bound what "equal" can mean here, both measured (tools/experiments/debug_grads.py, profiles/r02_gradient_parity.txt):
    the reference's arithmetic evaluated on THIS device (the oracle, eager fp32 torch) lands up to 1 % of scale away
    from its own CPU result for the bender / latent gradients -- sample_pdf's `denom < 1e-5` branch (rnh:694) falls the
    other way on 3 of the 16 rays, and those gradients pass through the 2^9 encoding frequency (fp32 vs fp64 of the same
    graph differ by 1 % as well) -- while the trunk / head gradients agree to 1e-5.  So: (1) against the oracle evaluated
    at the depths this path chose, EVERY tensor within 1e-4 of scale (measured 2e-6); (2) against the golden, within
    2e-3 of scale or 1.5 x the distance of the reference's own arithmetic on this device, whichever is larger."""
    from oracle import nrnerf_oracle as O
    ref = np.load(os.path.join(GOLDEN_DIR, fixture + ".npz"))
    cfg = SceneConfig(N_importance=64, **cfg_kw)
    scene = make_scene(cfg, 0)
    rays, latents = make_rays(16, 0, cfg)
    rb, coarse, fine = _modules(scene)
    lat = latents.to(DEV).requires_grad_(True)
    R.set_precision("f32")
    out = R.batchify_rays(rays.to(DEV), {"ray_bending_latents": lat}, network_fn=coarse, network_fine=fine, network_query_fn=None,
                          N_samples=64, N_importance=64, perturb=0.0, raw_noise_std=0.0, retraw=True, _want_z_vals=True)
    # (view-dependent head: the density branch in the native trunk kernel, the colour branch on its last hidden activation;
    #  finite-difference directions of the bent points, whose gradient reaches the bender through neighbouring samples)
    assert out["rgb_map"].requires_grad and out["rgb0"].requires_grad and out["raw"].shape == (16, 128, 4 if cfg.use_viewdirs else 5)
    loss = out["rgb_map"].sum() + out["rgb0"].sum()
    loss.backward()
    assert abs(float(loss.detach()) - float(ref["loss"])) < 1e-4 * abs(float(ref["loss"]))
    named = _named(rb, coarse, fine)
    ours = {("latents", ""): lat.grad}
    ours.update({k: p.grad for k, p in named.items() if p.grad is not None})

    def oracle_grads(z_override):
        sc = O.scene_on(scene, DEV)
        leaves = {}
        for part in ("bender", "coarse", "fine"):
            d = getattr(sc, part)
            if d is None:
                continue
            for k in d:
                d[k] = d[k].clone().requires_grad_(True)
                leaves[(part, k)] = d[k]
        l2 = latents.to(DEV).clone().requires_grad_(True)
        o = O.render_rays(rays.to(DEV), l2, sc, z_fine_override=z_override)
        (o["rgb_map"].sum() + o["rgb0"].sum()).backward()
        g = {("latents", ""): l2.grad}
        g.update({k: v.grad for k, v in leaves.items() if v.grad is not None})
        return g

    # (1) every tensor, against the reference's arithmetic at the same sample depths
    at_ours = oracle_grads(out["_z_vals"].detach())
    worst = 0.0
    for k, g in at_ours.items():
        scale = float(g.abs().max()) + 1e-12
        err = float((ours[k] - g).abs().max()) / scale
        worst = max(worst, err)
        assert err <= 1e-4, (k, err)
    # (2) the golden
    free = oracle_grads(None)
    report = []
    for key in ref.files:
        if not key.startswith("grad__"):
            continue
        k = ("latents", "") if key == "grad__latents" else tuple(key.split("__", 2)[1:])
        want = torch.from_numpy(ref[key])
        scale = float(want.abs().max()) + 1e-12
        assert tuple(ours[k].shape) == tuple(want.shape), key
        err = float((ours[k].cpu() - want).abs().max()) / scale
        dev_ref = float((free[k].cpu() - want).abs().max()) / scale
        report.append((key, err, dev_ref))
        assert err <= max(2e-3, 1.5 * dev_ref), (key, err, dev_ref)
    print(f"\n[gradients, fp32] worst |ours - oracle at our depths| / scale over {len(at_ours)} tensors: {worst:.1e}; vs reference golden "
          "(ours | the oracle on this device): " + "; ".join(f"{k[6:]} {e:.1e} | {d:.1e}" for k, e, d in report))


def _oracle_grads(scene, rays, latents, seed, perturb, noise, detailed_loss, z_override=None, weights=None, dtype=torch.float32, **flags):
    """``weights``: {(part, name): tensor} to use instead of the scene's (the modules' parameters after an optimiser step)."""
    from oracle import nrnerf_oracle as O
    sc = O.scene_on(scene, DEV)
    leaves = {}
    for part in ("bender", "coarse", "fine"):
        d = getattr(sc, part)
        if d is None:
            continue
        for k in d:
            d[k] = (weights[(part, k)].detach() if weights is not None else d[k]).to(dtype).clone().requires_grad_(True)
            leaves[(part, k)] = d[k]
    # (dtype = float64: the SAME graph in double precision (the oracle is dtype-generic) -- i.e. how far the
    #  reference's own fp32 arithmetic is from the exact gradient)
    lat = latents.to(DEV).to(dtype).clone().requires_grad_(True)
    torch.manual_seed(seed)
    out = O.render_rays(rays.to(DEV), lat, sc, retraw=True, detailed_output=detailed_loss, perturb=perturb, raw_noise_std=noise,
                        z_fine_override=(z_override.to(dtype) if z_override is not None else None), dtype=dtype, **flags)
    loss = _loss(out, detailed_loss)
    loss.backward()
    return float(loss.detach()), lat.grad, {k: v.grad for k, v in leaves.items()}, out


def _loss(out, detailed):
    target = torch.linspace(0.1, 0.9, 3, device=out["rgb_map"].device)
    loss = ((out["rgb_map"] - target) ** 2).mean() + ((out["rgb0"] - target) ** 2).mean() + 0.1 * out["acc_map"].mean()
    if not bool(torch.isnan(out["disp_map"]).any()):
        # (a ray without any opacity has disp = 1 / max(1e-10, 0 / 0) = NaN, train.py:781, and autograd then turns every
        #  gradient into NaN even under a mask -- in the reference too, whose training loss never touches disp_map)
        loss = loss + 0.05 * (out["disp_map"].clamp(max=50.0)).mean() * 1e-2
    if detailed:        # the offsets regulariser's shape (train.py:219-236): detached weights x offset norms, plus the rigidity term
        w = out["visibility_weights"].detach()
        off = torch.norm(out["unmasked_offsets"], dim=-1)
        rig = out["rigidity_mask"][..., 0]
        loss = loss + 3.0 * (w * torch.pow(off + 1e-12, 2.0 - rig)).mean() + 0.01 * (w * rig).mean()
        loss = loss + 0.02 * out["fine_visibility_weights"].pow(2).mean()      # a gradient through the weights output
    return loss


@pytest.mark.gpu
@pytest.mark.parametrize("perturb,noise,detailed,cfg_kw", [(0.0, 0.0, False, dict(N_importance=64)),
                                                           (1.0, 1.0, True, dict(N_samples=48, N_importance=37)),
                                                           (1.0, 0.5, False, dict(N_importance=128, ray_bending=False)),
                                                           (1.0, 0.0, False, dict(N_importance=64, netwidth=128)),
                                                           (0.0, 0.0, False, dict(N_importance=64, _lindisp=True, _white_bkgd=True)),
                                                           (1.0, 1.0, True, dict(N_samples=48, N_importance=37, use_viewdirs=True)),
                                                           (0.0, 0.0, False, dict(N_importance=64, use_viewdirs=True, ray_bending=False)),
                                                           (1.0, 0.5, False, dict(N_importance=64, use_viewdirs=True, bend_depth=7)),
                                                           (1.0, 1.0, False, dict(N_samples=48, N_importance=37, ray_bending=False, time_conditioned_baseline=True)),
                                                           (1.0, 0.0, False, dict(N_samples=48, N_importance=37, ray_bending=False, time_conditioned_baseline=True,
                                                                                   use_viewdirs=True)),
                                                           (1.0, 1.0, True, dict(N_samples=48, N_importance=37, use_viewdirs=True, approx_nonrigid_viewdirs=False)),
                                                           (0.0, 0.0, False, dict(N_importance=64, use_viewdirs=True, approx_nonrigid_viewdirs=False, bend_depth=7)),
                                                           (1.0, 1.0, True, dict(N_samples=200, N_importance=150)),
                                                           # the native training cap went from 256 to 1024 samples per pass -- the
                                                           # composite_bwd instantiations with 6 / 12 / 16 samples per lane, trunk / bender /
                                                           # wgrad kernels beyond 8 blocks per ray, the non-split fine bender (> 256 merged)
                                                           (0.0, 0.0, False, dict(N_samples=192, N_importance=128)),
                                                           (1.0, 1.0, True, dict(N_samples=64, N_importance=450)),
                                                           (1.0, 0.0, False, dict(N_samples=600, N_importance=300)),
                                                           # round 5: architectures OUTSIDE the compiled set train on the run-time-parameterised
                                                           # kernel (training._GenericTrunk: forward with saved activations, backward-data from
                                                           # transposed weights; the bender as torch ops)
                                                           (1.0, 1.0, True, dict(N_samples=48, N_importance=37, netwidth=192, netdepth=6)),
                                                           (1.0, 0.5, False, dict(N_importance=64, netwidth=320, netdepth=5, skips=(2,), multires=6, ray_bending=False)),
                                                           (0.0, 0.0, False, dict(N_importance=64, netwidth=64, netdepth=3, skips=(), netwidth_fine=132, netdepth_fine=4)),
                                                           (1.0, 0.0, False, dict(N_samples=300, N_importance=200, netwidth=512, netdepth=2, skips=(0,), ray_bending=False)),
                                                           # ... with the view-dependent head (the rays' own directions; finite differences of bent points)
                                                           (1.0, 0.5, False, dict(N_importance=64, netwidth=192, netdepth=6, use_viewdirs=True, ray_bending=False)),
                                                           (1.0, 1.0, True, dict(N_samples=48, N_importance=37, netwidth=128, netdepth=4, skips=(1,), use_viewdirs=True,
                                                                                 multires_views=2, netwidth_fine=480, netdepth_fine=3)),
                                                           # the 128-wide trunk with the view-dependent head: rendered by compiled kernels, trained on a
                                                           # generic handle that render_rays_train asks for (MODEL_FORCE_GENERIC)
                                                           (1.0, 0.0, False, dict(N_importance=64, netwidth=128, use_viewdirs=True)),
                                                           # the time-conditioned baseline off the compiled set: the latent code as input columns of the
                                                           # run-time-parameterised kernel, its gradient from the same two outputs as the encoding's
                                                           (1.0, 1.0, False, dict(N_samples=48, N_importance=37, ray_bending=False, time_conditioned_baseline=True,
                                                                                  netwidth=192, netdepth=6)),
                                                           (1.0, 0.0, False, dict(N_importance=64, ray_bending=False, time_conditioned_baseline=True, use_viewdirs=True,
                                                                                  netwidth=128, latent_size=16)),
                                                           # exact Jacobian directions off the compiled set: the tangent through the bender's compiled training
                                                           # kernels (a generic handle carries them when the bender has the reference's hard-coded shape)
                                                           (1.0, 1.0, True, dict(N_samples=48, N_importance=37, netwidth=192, netdepth=6, use_viewdirs=True,
                                                                                 approx_nonrigid_viewdirs=False))],
                         ids=["deterministic", "stochastic_detailed_ragged", "no_bender_64_128", "narrow_128", "lindisp_white_bkgd",
                              "viewdirs_detailed_ragged", "viewdirs_no_bender", "config4_viewdirs_deep_bender", "time_conditioned_ragged",
                              "time_conditioned_viewdirs", "exact_viewdirs_detailed_ragged", "exact_viewdirs_deep_bender",
                              "350_samples_per_ray", "192_plus_128", "514_samples_detailed", "900_samples",
                              "generic_w192_d6_detailed_ragged", "generic_w320_d5_skip2_L6_no_bender", "generic_no_skip_w64_fine_w132", "generic_w512_d2_500_samples",
                              "generic_viewdirs_w192_d6_no_bender", "generic_viewdirs_w128_d4_fine_w480_detailed_ragged", "generic_forced_w128_viewdirs",
                              "generic_time_conditioned_w192_d6_ragged", "generic_time_conditioned_viewdirs_w128_latent16", "generic_exact_viewdirs_w192_d6_detailed_ragged"])
@pytest.mark.parametrize("bender", ["torch_ops", "native"])
def test_fp32_gradients_vs_oracle_autograd(perturb, noise, detailed, cfg_kw, bender):
    """Every parameter of every network + the latent codes, fp32 mode, against the oracle's autograd (eager torch on the
    GPU, same seeded random numbers) evaluated at the merged depths this path chose (see the golden test for why): 2e-3
    of each tensor's scale (measured: 2e-6 for every trunk / head tensor; up to 1e-3 for the bender and latent tensors
    on 131 rays, where a handful of relu decisions next to zero differ between the MFMA and the library GEMM rounding);
    loss with data, acc, disp, weights and regulariser terms.
    bender = "native" (nrnerf_bender_*, the default): its bent points equal the oracle's to 2e-6 but not bit for bit, and
    an ulp there moves the gradients that pass through the 2^9-frequency encoding by 1e-2 of their scale (the golden
    test's docstring; same size as fp32 vs fp64 of the reference's own graph): those tensors -- bender, latent codes -- get
    a 5e-2 bar here and their tight check in test_native_bender_forward_and_gradients_vs_torch_autograd (1e-4, bender
    alone); the trunk / head tensors keep the 2e-3 bar."""
    from nonrigid_nerf_amd import training
    flags = {k[1:]: v for k, v in cfg_kw.items() if k.startswith("_")}      # render_rays flags (train.py:799, 802), not scene settings
    cfg_kw = {k: v for k, v in cfg_kw.items() if not k.startswith("_")}
    if bender == "native" and not SceneConfig(**cfg_kw).ray_bending:
        pytest.skip("no bender in this case")
    loose = 5e-2 if bender == "native" else 2e-3
    cfg = SceneConfig(**cfg_kw)
    # view-dependent head with a bender: the directions are NORMALISED DIFFERENCES of neighbouring bent points (spacing ~ 5e-3
    # of the scene), so an ulp of a bent point is a 2e-5 relative change of a direction and reaches every gradient tensor:
    # trunk tensors get 1e-2 there (measured 2.4e-3 on the 7-layer-bender case), bender / latent tensors the loose bar; the
    # tight check of this path is the golden test above (1e-4 against the oracle at equal depths, every tensor)
    tight = 1e-2 if (cfg.use_viewdirs and cfg.ray_bending) else 2e-3
    if cfg.use_viewdirs and cfg.ray_bending:
        loose = 5e-2
    scene = make_scene(cfg, 1)
    rays, latents = make_rays(131 if cfg.N_samples + cfg.N_importance <= 400 else 37, 3, cfg)
    rb, coarse, fine = _modules(scene)
    lat = latents.to(DEV).requires_grad_(True)
    R.set_precision("f32")
    torch.manual_seed(99)
    saved = (training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER)
    # torch_ops: the oracle's bent points, bit for bit (the fine pass then bends all merged points in one call, see the fixture)
    training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = bender == "native", False, bender == "native"
    out = R.render_rays(rays.to(DEV), coarse, None, cfg.N_samples, retraw=True, perturb=perturb, N_importance=cfg.N_importance,
                        network_fine=fine, raw_noise_std=noise, additional_pixel_information={"ray_bending_latents": lat},
                        detailed_output=detailed, _want_z_vals=True, **flags)
    training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = saved
    z_ours = out.pop("_z_vals").detach()
    loss = _loss(out, detailed)
    loss.backward()
    l_ref, glat_ref, g_ref, out_ref = _oracle_grads(scene, rays, latents, 99, perturb, noise, detailed, z_override=z_ours, **flags)
    assert set(out) == set(k for k in out_ref if not k.startswith("_"))
    for k in ("rgb_map", "rgb0", "acc_map"):
        assert torch.allclose(out[k], out_ref[k].detach(), atol=1e-4), k
    assert abs(float(loss.detach()) - l_ref) <= 1e-4 * abs(l_ref)
    named = _named(rb, coarse, fine)
    fails, worst = [], 0.0
    if cfg.ray_bending:
        scale = float(glat_ref.abs().max()) + 1e-12
        worst = float((lat.grad - glat_ref).abs().max()) / scale
        if worst > loose:
            fails.append(("latents", worst))
    for (part, name), gr in g_ref.items():
        g = named[(part, name)].grad
        if gr is None:
            continue
        scale = float(gr.abs().max()) + 1e-12
        err = float((g - gr).abs().max()) / scale
        worst = max(worst, err)
        if err > (loose if part == "bender" else tight):
            fails.append((part, name, err))
    print(f"\n[gradients vs oracle autograd, fp32, {bender} bender] worst error / scale {worst:.1e}")
    assert not fails, fails
    # free-running (the oracle draws its own importance samples): the sample_pdf branch may move a sample on a few rays
    torch.manual_seed(99)
    free = O_render_free(scene, rays, latents, perturb, noise, detailed, **flags)
    moved = ((z_ours - free).abs() > 2e-5).float().mean().item()
    assert moved < 0.02, moved


def O_render_free(scene, rays, latents, perturb, noise, detailed, **flags):
    from oracle import nrnerf_oracle as O
    with torch.no_grad():
        return O.render_rays(rays.to(DEV), latents.to(DEV), O.scene_on(scene, DEV), detailed_output=detailed, perturb=perturb,
                             raw_noise_std=noise, **flags)["_z_vals"]


@pytest.mark.gpu
@pytest.mark.parametrize("width,detailed,views,S,I", [(256, False, False, 64, 64), (128, False, False, 64, 64), (256, True, False, 64, 64),
                                                      (256, False, True, 64, 64), (256, False, False, 192, 128), (256, True, False, 300, 400),
                                                      (128, False, False, 64, 450), (192, True, False, 64, 64), (320, False, False, 64, 300),
                                                      (320, False, True, 64, 64)],
                         ids=["w256", "w128", "w256_detailed_loss", "w256_viewdirs", "w256_192_plus_128", "w256_700_samples_detailed", "w128_514_samples",
                              "generic_w192_detailed_loss", "generic_w320_364_samples", "generic_w320_viewdirs"])
def test_bf16_gradients_point_the_same_way(width, detailed, views, S, I):
    """bf16 training mode (bf16 activations and d z in block-tile layout, relu bit masks, trunk_wgrad): gradient direction and
    size against fp32 mode (row-major arrays, trunk_wgrad_f32), both compiled trunk widths -- and above 256 samples per pass (up to
    NRNERF_MAX_SAMPLES: more than 8 blocks per ray in every training kernel, composite_bwd with 6 / 12 samples per lane, the fine pass
    bending all merged samples instead of the split bender)."""
    cfg = SceneConfig(N_samples=S, N_importance=I, netwidth=width, use_viewdirs=views)
    scene = make_scene(cfg, 1)
    # (512 rays at every size: the rigidity network's gradients are sums with heavy cancellation -- on 96 rays bf16 and fp32 modes disagree
    #  about them at 64 + 64 samples as much as at 300 + 400, tools/experiments/debug_bf16_grads_large.py)
    rays, latents = make_rays(512, 3, cfg)
    grads = {}
    for prec in ("f32", "bf16"):
        rb, coarse, fine = _modules(scene)
        lat = latents.to(DEV).requires_grad_(True)
        R.set_precision(prec)
        out = R.render_rays(rays.to(DEV), coarse, None, S, N_importance=I, network_fine=fine,
                            additional_pixel_information={"ray_bending_latents": lat}, detailed_output=detailed)
        _loss(out, detailed).backward()             # detailed: + the offsets / rigidity regulariser terms and a weights term
        g = {k: p.grad.flatten().float() for k, p in _named(rb, coarse, fine).items() if p.grad is not None}
        g[("latents", "")] = lat.grad.flatten()
        grads[prec] = g
    bad, seen = [], []
    for k, g32 in grads["f32"].items():
        g16 = grads["bf16"][k]
        if float(g32.norm()) < 1e-10:
            continue
        cos = float(torch.dot(g32, g16) / (g32.norm() * g16.norm() + 1e-30))
        ratio = float(g16.norm() / g32.norm())
        seen.append((k, round(cos, 4), round(ratio, 4)))
        # the bender's and the latent codes' gradients pass through the 2^9 encoding frequency: noisier under bf16
        loose = k[0] in ("bender", "latents")
        # (the rigidity network's: sums with heavy cancellation, see above -- measured norm ratios 0.81 .. 1.42 over these cases, cosine >= 0.94)
        hi = 1.5 if "rigidity_network" in k[1] else 1.4
        # (view-dependent head: the bender also receives the gradient of the finite-difference directions, differences of neighbouring bent
        #  points divided by their ~5e-3 spacing -- measured cosines 0.945 on the compiled 256-wide case, 0.89 on the 320-wide generic one)
        lo = (0.85 if views else 0.9) if loose else 0.97
        if not (cos > lo and ((0.6 < ratio < hi) if loose else (0.9 < ratio < 1.1))):
            bad.append((k, round(cos, 4), round(ratio, 4)))
    far = sorted(seen, key=lambda r: -abs(r[2] - 1.0))[:3]
    print(f"\n[bf16 vs fp32 gradients, W{width} {S}+{I}] furthest norm ratios: {far}; lowest cosine {min(r[1] for r in seen)}")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("bender", [False, "torch_ops", "native"], ids=["no_bender", "torch_ops_bender", "native_bender"])
def test_generic_training_sees_an_optimiser_step_in_forward_and_backward_weights(bender):
    """A non-compiled architecture keeps TWO images of every trunk weight on the device -- the forward program's and the transposed
    one of the backward-data program (csrc/nrnerf_pack.cpp::gen_pack_mlp_bwd) -- and an optimiser step must reach both through the
    device-side re-pack (nrnerf_model_update_device: the source maps of the transposed fragments).  Gradients after a large step
    against the oracle's autograd on the stepped weights, fp32 mode, 2e-3 of each tensor's scale as in the test above (stale
    transposed weights would leave d_pre, hence every gradient but the head's, at the old weights' values).  ``native_bender``: the bender's
    compiled training kernels on the generic handle (its bender has the reference's hard-coded shape) -- their weight images are re-packed
    by the same call; bent points then differ from the oracle's by ulps, which the 2^9-frequency encoding turns into 1e-2 of a gradient's
    scale (the golden test's docstring): 2e-2 / 5e-2 bars there."""
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(N_importance=64, netwidth=192, netdepth=6, netwidth_fine=320, netdepth_fine=5, skips=(2,), ray_bending=bool(bender))
    scene = make_scene(cfg, 1)
    rays, latents = make_rays(96, 3, cfg)
    rb, coarse, fine = _modules(scene)
    named = _named(rb, coarse, fine)
    lat = latents.to(DEV).requires_grad_(True)
    R.set_precision("f32")
    calls = {"dev": 0}
    orig = R.Model.update_from_device

    def counting(self, *a, **k):
        ok = orig(self, *a, **k)
        calls["dev"] += int(ok)
        return ok

    def ours():
        for p_ in named.values():
            p_.grad = None
        out = R.render_rays(rays.to(DEV), coarse, None, cfg.N_samples, retraw=True, N_importance=cfg.N_importance, network_fine=fine,
                            additional_pixel_information={"ray_bending_latents": lat}, _want_z_vals=True)
        z = out.pop("_z_vals").detach()
        _loss(out, False).backward()
        return z

    R.Model.update_from_device = counting
    saved = (training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER)
    training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = bender == "native", False, bender == "native"
    try:
        ours()
        torch.manual_seed(5)
        with torch.no_grad():           # "an optimiser step": every parameter moves by ~10 % of its scale, in place
            for p_ in named.values():
                p_.add_(torch.randn_like(p_) * 0.1 * p_.abs().mean())
        z = ours()
    finally:
        R.Model.update_from_device = orig
        training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = saved
    assert calls["dev"] >= 1, "the second call did not take the device-side re-pack"
    _, _, g_ref, _ = _oracle_grads(scene, rays, latents, 0, 0.0, 0.0, False, z_override=z, weights=named)
    # the yardstick for the bars below ("a measurement, not an allowance"): the oracle's OWN fp32 arithmetic against the same
    # graph in fp64, per tensor -- behind the bent point sits the 2^9-frequency encoding, so an ulp of the point moves the bender's and,
    # with the native bender (another fp32 rounding of the bent points), every downstream gradient by this much
    _, _, g_64, _ = _oracle_grads(scene, rays, latents, 0, 0.0, 0.0, False, z_override=z, weights=named, dtype=torch.float64)
    fails, worst, worst_ref, by_part = [], 0.0, 0.0, {}
    for (part, name), gr in g_ref.items():
        if gr is None:
            continue
        scale = float(gr.abs().max()) + 1e-12
        err = float((named[(part, name)].grad - gr).abs().max()) / scale
        e3264 = float((gr.double() - g_64[(part, name)]).abs().max()) / scale
        worst, worst_ref = max(worst, err), max(worst_ref, e3264)
        w = by_part.setdefault(part, [0.0, 0.0])
        w[0], w[1] = max(w[0], err), max(w[1], e3264)
        if err > (5e-2 if part == "bender" else (2e-2 if bender == "native" else 2e-3)):
            fails.append((part, name, err, e3264))
    print(f"\n[generic training after a step, fp32, {bender or 'no'} bender] worst error / scale {worst:.1e} (the oracle's fp32 vs fp64 on the same "
          f"tensors: {worst_ref:.1e}); per part ours | oracle fp32-vs-fp64: " + ", ".join(f"{k} {a:.1e} | {b:.1e}" for k, (a, b) in by_part.items())
          + f"; device re-packs {calls['dev']}")
    assert not fails, fails
    # ... and the bars ARE of that size: no part of the model may sit further from the fp32 oracle than 10 x the distance the oracle's
    # own fp32 arithmetic has from fp64 on that part (or the plain fp32 tolerance of a trunk without a bender in front, 2e-3).  With the
    # native bender -- another fp32 rounding of the bent points, i.e. a perturbation AT the bender's output -- the trunks downstream are
    # held to the bender part's figure (measured on the MI355X: bender 1.2e-2 | 3.9e-3, coarse 4.4e-3 | 1.2e-4, fine 1.5e-3 | 1.5e-3)
    b_bender = by_part.get("bender", [0.0, 0.0])[1] if bender == "native" else 0.0
    for k, (a, b) in by_part.items():
        assert a <= max(2e-3, 10.0 * max(b, b_bender)), (k, a, b, b_bender)


@pytest.mark.gpu
def test_generic_training_fits_the_example_sequence():
    """test_native_training_fits_the_example_sequence... for an architecture outside the compiled set (coarse 6 x 192, fine 5 x 320 with
    the skip behind layer 2; the bender as torch ops): 200 Adam steps of 1024 rays in bf16 from the reference's initialisation take the
    batch PSNR past 17 dB, every step's weights (forward and transposed images) refreshed on the device."""
    from nonrigid_nerf_amd.modules import NeRFWeights, RayBenderWeights
    from oracle.fit_checkpoint import frame_rays, init_bender_like_reference, load_fixture
    fx = load_fixture()
    F_, H, W = fx["images"].shape[:3]
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    rb = RayBenderWeights()
    init_bender_like_reference(rb)
    coarse = NeRFWeights(D=6, W=192, output_ch=5, num_ray_samples=64)
    fine = NeRFWeights(D=5, W=320, skips=(2,), output_ch=5, num_ray_samples=128)
    for m in (rb, coarse, fine):
        m.to(DEV)
    coarse.ray_bender = fine.ray_bender = (rb,)
    codes = torch.zeros(F_, 32, device=DEV, requires_grad=True)
    opt = torch.optim.Adam(list(coarse.parameters()) + list(fine.parameters()) + list(rb.parameters()) + [codes], lr=5e-4)
    rays_all = torch.stack([frame_rays(fx["poses"][f], fx["intrin"], fx["near"], fx["far"]) for f in range(F_)], 0).to(DEV)
    target_all = fx["images"].reshape(F_, H * W, 3).to(DEV)
    R.set_precision("bf16")
    calls = {"dev": 0}
    orig = R.Model.update_from_device

    def counting(self, *a, **k):
        ok = orig(self, *a, **k)
        calls["dev"] += int(ok)
        return ok

    R.Model.update_from_device = counting
    psnrs = []
    try:
        for step in range(200):
            img = torch.from_numpy(rng.randint(F_, size=1024)).to(DEV)
            pix = torch.from_numpy(rng.randint(H * W, size=1024)).to(DEV)
            rays, target = rays_all[img, pix], target_all[img, pix]
            opt.zero_grad(set_to_none=True)
            out = R.batchify_rays(rays, {"ray_bending_latents": codes[img]}, chunk=32768, network_fn=coarse, network_fine=fine,
                                  network_query_fn=None, N_samples=64, N_importance=64, perturb=1.0, raw_noise_std=1.0, retraw=True)
            mse = ((out["rgb_map"] - target) ** 2).mean()
            (mse + ((out["rgb0"] - target) ** 2).mean()).backward()
            opt.step()
            for g in opt.param_groups:
                g["lr"] = 5e-4 / (20.0 * (-(step - 1000) / 1000) + 1.0)                # warm-up, train.py:1636-1640
            psnrs.append(-10.0 * np.log10(float(mse.detach())))
    finally:
        R.Model.update_from_device = orig
        R.set_precision("f32")
    print(f"\n[generic training, 6 x 192 / 5 x 320, bf16] batch PSNR: first 5 steps {np.mean(psnrs[:5]):.2f} dB, last 20 steps {np.mean(psnrs[-20:]):.2f} dB; "
          f"device refreshes {calls['dev']}")
    assert np.all(np.isfinite(psnrs))
    assert np.mean(psnrs[-20:]) > 17.0 and np.mean(psnrs[-20:]) > np.mean(psnrs[:5]) + 4.0, (psnrs[:5], psnrs[-20:])
    assert calls["dev"] >= 195, calls


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_generic_architecture_trains_faster_than_eager_autograd(precision):
    """What the native path for a non-compiled architecture buys: forward + loss + backward of 2048 rays x (64 + 128) samples of a
    192-wide trunk (no bender), against the same iteration as eager torch ops with autograd (the oracle; fp32) on this device.
    Printed; the bar is only that it is not slower (beyond timing noise)."""
    import time
    from oracle import nrnerf_oracle as O
    cfg = SceneConfig(N_samples=64, N_importance=128, netwidth=192, ray_bending=False)
    scene = make_scene(cfg, 1)
    rays, latents = make_rays(2048, 3, cfg)
    rays, lat_dev = rays.to(DEV), latents.to(DEV)
    rb, coarse, fine = _modules(scene)
    R.set_precision(precision)
    target = torch.linspace(0.1, 0.9, 3, device=DEV)

    def ours():
        out = R.render_rays(rays, coarse, None, 64, N_importance=128, network_fine=fine, perturb=1.0, raw_noise_std=1.0)
        (((out["rgb_map"] - target) ** 2).mean() + ((out["rgb0"] - target) ** 2).mean()).backward()

    sc = O.scene_on(scene, DEV)
    for d in (sc.coarse, sc.fine):
        for k in d:
            d[k] = d[k].clone().requires_grad_(True)

    def eager():
        out = O.render_rays(rays, lat_dev, sc, perturb=1.0, raw_noise_std=1.0)
        (((out["rgb_map"] - target) ** 2).mean() + ((out["rgb0"] - target) ** 2).mean()).backward()

    def timed(fn):
        for _ in range(3):
            fn()
        best = 1e9
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / 5)
        return best
    t_ours, t_eager = timed(ours), timed(eager)
    R.set_precision("f32")
    print(f"\n[generic training, W192 D8, 2048 rays x (64 + 128), {precision}] native {t_ours * 1e3:.2f} ms per forward + backward; "
          f"eager torch autograd (fp32) {t_eager * 1e3:.2f} ms: {t_eager / t_ours:.2f} x")
    assert t_ours < 1.15 * t_eager          # (measured: fp32 13.7 vs 21.9 ms, 1.60 x; bf16 6.5 ms, 3.37 x)


@pytest.mark.gpu
def test_native_training_fits_the_example_sequence_and_refreshes_weights_on_the_device():
    """The reference's training loop (train.py:1543-1642: random rays over all images, perturb = 1, raw_noise_std = 1,
    data term on rgb_map and rgb0, Adam 5e-4 with warm-up) through the drop-in boundary on the down-sampled example
    sequence, from the reference's initialisation: 200 steps of 1024 rays in bf16 must take the batch PSNR from ~11 dB
    past 17 dB (the oracle-driven fit of oracle/fit_checkpoint.py is at ~19-20 dB after 250 steps), with every step's
    weight refresh done by nrnerf_model_update_device (no host round trip) and gradients reaching the latent codes."""
    from nonrigid_nerf_amd.modules import NeRFWeights, RayBenderWeights
    from oracle.fit_checkpoint import frame_rays, init_bender_like_reference, load_fixture
    fx = load_fixture()
    F_, H, W = fx["images"].shape[:3]
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    rb = RayBenderWeights()
    init_bender_like_reference(rb)
    coarse, fine = NeRFWeights(output_ch=5, num_ray_samples=64), NeRFWeights(output_ch=5, num_ray_samples=128)
    for m in (rb, coarse, fine):
        m.to(DEV)
    coarse.ray_bender = fine.ray_bender = (rb,)
    codes = torch.zeros(F_, 32, device=DEV, requires_grad=True)
    params = list(coarse.parameters()) + list(fine.parameters()) + list(rb.parameters()) + [codes]
    opt = torch.optim.Adam(params, lr=5e-4)
    rays_all = torch.stack([frame_rays(fx["poses"][f], fx["intrin"], fx["near"], fx["far"]) for f in range(F_)], 0).to(DEV)
    target_all = fx["images"].reshape(F_, H * W, 3).to(DEV)
    R.set_precision("bf16")
    calls = {"dev": 0}
    orig = R.Model.update_from_device

    def counting(self, *a, **k):
        ok = orig(self, *a, **k)
        calls["dev"] += int(ok)
        return ok

    R.Model.update_from_device = counting
    psnrs, gcodes = [], []
    try:
        for step in range(200):
            img = torch.from_numpy(rng.randint(F_, size=1024)).to(DEV)
            pix = torch.from_numpy(rng.randint(H * W, size=1024)).to(DEV)
            rays, target = rays_all[img, pix], target_all[img, pix]
            opt.zero_grad(set_to_none=True)
            out = R.batchify_rays(rays, {"ray_bending_latents": codes[img]}, chunk=32768, network_fn=coarse, network_fine=fine,
                                  network_query_fn=None, N_samples=64, N_importance=64, perturb=1.0, raw_noise_std=1.0, retraw=True)
            mse = ((out["rgb_map"] - target) ** 2).mean()
            loss = mse + ((out["rgb0"] - target) ** 2).mean()
            loss.backward()
            opt.step()
            lr = 5e-4 / (20.0 * (-(step - 1000) / 1000) + 1.0)                       # warm-up, train.py:1636-1640
            for g in opt.param_groups:
                g["lr"] = lr
            psnrs.append(-10.0 * np.log10(float(mse.detach())))
            gcodes.append(float(codes.grad.abs().max()))
    finally:
        R.Model.update_from_device = orig
    print(f"\n[native training, bf16] batch PSNR: first 5 steps {np.mean(psnrs[:5]):.2f} dB, last 20 steps {np.mean(psnrs[-20:]):.2f} dB; "
          f"device refreshes {calls['dev']}")
    assert np.all(np.isfinite(psnrs))
    assert np.mean(psnrs[-20:]) > 17.0 and np.mean(psnrs[-20:]) > np.mean(psnrs[:5]) + 4.0, (psnrs[:5], psnrs[-20:])
    assert calls["dev"] >= 195, calls
    assert max(gcodes[100:]) > 0.0, "no gradient reaches the latent codes"


@pytest.mark.gpu
@pytest.mark.parametrize("knobs,bend_depth", [(dict(), 5), (dict(rigidity_test_time_cutoff=0.58, test_time_scaling=0.7), 5), (dict(), 7)],
                         ids=["plain", "cutoff_scaling", "deep_bender"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_native_bender_forward_and_gradients_vs_torch_autograd(precision, knobs, bend_depth):
    """nrnerf_bender_forward / _backward (csrc/nrnerf_train_bend.h, always fp32) against torch.autograd over the same
    layers written as torch ops (training.bend), on the bender ALONE -- without the 2^9-frequency encoding behind it the
    comparison is well conditioned: outputs within 2e-6, every gradient (latent codes, all 15 / 19 parameter tensors) within
    1e-4 of its scale, for random upstream gradients of all three differentiable outputs; ragged sample count."""
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(N_importance=64, bend_depth=bend_depth)
    scene = make_scene(cfg, 2)
    N, S = 77, 83
    rays, latents = make_rays(N, 5, cfg)
    rays = rays.to(DEV)
    rb, coarse, fine = _modules(scene)
    for k, v in knobs.items():
        setattr(rb, k, v)
    with torch.no_grad():                      # this scene's rigidity saturates at 1: spread the masks around 0.5 so the cutoff bites
        rb.rigidity_network[-1].weight.mul_(0.02)
        rb.rigidity_network[-1].bias.zero_()
    R.set_precision(precision)
    model = R.get_model(coarse, fine, precision=precision, device=torch.device(DEV))
    gen = torch.Generator(device="cpu").manual_seed(17)
    z = (2.0 + 4.0 * torch.rand(N, S, generator=gen)).sort(-1).values.to(DEV)
    g_bent, g_un, g_mask = (torch.randn(N, S, c, generator=gen).to(DEV) for c in (3, 3, 1))

    def run(native):
        for p in rb.parameters():
            p.grad = None
        lat = latents.to(DEV).clone().requires_grad_(True)
        if native:
            bent, d = training.bend_native(model, rb, rays, z, lat)
        else:
            pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
            old, training.BATCHED_BENDER = training.BATCHED_BENDER, False
            bent, d = training.bend(rb, pts, lat[:, None, :].expand(N, S, lat.shape[-1]).reshape(N * S, -1))
            training.BATCHED_BENDER = old
            bent, d = bent.reshape(N, S, 3), {k: v.reshape(N, S, -1) for k, v in d.items()}
        loss = (bent * g_bent).sum() + (d["unmasked_offsets"] * g_un).sum() + (d["rigidity_mask"] * g_mask).sum() \
            + 0.3 * (d["masked_offsets"] * g_un.flip(0)).sum()
        loss.backward()
        grads = {"latents": lat.grad.clone()}
        grads.update({k: p.grad.clone() for k, p in rb.named_parameters()})
        return bent.detach(), {k: v.detach() for k, v in d.items()}, grads

    bent_t, d_t, g_t = run(False)
    bent_n, d_n, g_n = run(True)
    assert float((bent_n - bent_t).abs().max()) <= 2e-6
    for k in d_t:
        assert float((d_n[k] - d_t[k]).abs().max()) <= 2e-6, k
    if knobs:
        assert float((d_t["rigidity_mask"] == 0).float().mean()) > 0.02, "the cutoff should bite on this scene"
    assert set(g_n) == set(g_t) and len(g_t) == 2 * bend_depth + 6
    worst = 0.0
    # bf16 model + nrnerf_bender_wgrad: the weight-gradient contraction runs on the bf16 matrix pipe with operands rounded in
    # registers (fp32 accumulation): 2^-9 relative per element, averaged over 6 391 samples -> 1e-2 of scale (measured 5.3e-3); the latent
    # codes' gradient (backward-data kernel, exact fp32) and every fp32-model gradient keep the 1e-4 bar
    for k, want in g_t.items():
        scale = float(want.abs().max()) + 1e-12
        err = float((g_n[k] - want).abs().max()) / scale
        worst = max(worst, err)
        bar = 1e-2 if (precision != "f32" and k != "latents") else 1e-4
        assert err <= bar, (k, err, bar)
    print(f"\n[native bender vs torch autograd, {precision} model] worst gradient error / scale {worst:.1e}")


def _block_tiles(x, N, S):
    """[N*S, c <= 64] -> bf16 [B, 64, 32]: per block of 32 consecutive samples of a ray a [64 x 32] tile with the samples
    contiguous, rows >= c and the columns beyond a ray's end zero -- the operand layout of nrnerf_trunk_wgrad."""
    c, bpr = int(x.shape[1]), (S + 31) // 32
    t = torch.zeros(N, bpr * 32, 64, dtype=torch.bfloat16, device=x.device)
    t[:, :S, :c] = x.view(N, S, c)
    return t.view(N * bpr, 32, 64).transpose(1, 2).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("width,n_rays,S,views", [(256, 37, 192, False), (256, 5, 85, False), (128, 64, 64, False), (256, 11, 85, True)],
                         ids=["w256", "w256_ragged", "w128", "w256_viewdirs"])
def test_trunk_wgrad_kernel_vs_einsum(width, n_rays, S, views):
    """nrnerf_trunk_wgrad (bf16 mode: all weight / bias gradients of the trunk in one call over the [block][feature][32
    samples] arrays) on random bf16 arrays against fp32 einsums over the same values: hidden layers, the two encoding
    products, the head, the bias sums; ragged block counts; both compiled trunk widths.  fp32 accumulation on both sides,
    so 1e-4 of scale.  The two operands the call builds itself -- encoding of the points, head gradient, in block tiles --
    against torch (one bf16 ulp: sin / cos implementations differ in the last fp32 bit).  ``views``: a model with the
    view-dependent head -- three more products over the colour branch's saved arrays (d z_v^T h_7, d z_v^T enc(direction),
    hv^T d raw) and d z_v's row sums, and the direction encoding as a third operand."""
    import ctypes as C
    from nonrigid_nerf_amd import _lib, training
    cfg = SceneConfig(N_importance=64, netwidth=width, use_viewdirs=views)
    scene = make_scene(cfg, 0)
    rb, coarse, fine = _modules(scene, requires_grad=False)
    R.set_precision("bf16")
    model = R.get_model(coarse, fine, precision="bf16", device=torch.device(DEV))
    D, W, M = 8, width, n_rays * S
    nblk = n_rays * ((S + 31) // 32)
    gen = torch.Generator().manual_seed(4)
    mk = lambda *shape: (torch.randn(*shape, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    acts, d_pre = mk(D, nblk, W, 32).abs(), mk(D, nblk, W, 32)
    pts4 = (torch.randn(M, 4, generator=gen) * 0.4).to(DEV)
    g4 = torch.randn(M, 4, generator=gen).to(DEV)
    scratch = torch.full((3, nblk, 64, 32), float("nan"), dtype=torch.bfloat16, device=DEV)
    kch = 7
    stride = _lib.wgrad_stride_views(D, W) if views else _lib.wgrad_stride(D, W)
    parts = torch.zeros(kch, stride, device=DEV)          # the 64-column jobs fill fewer records: zero-filled by the caller
    a = _lib.WgradArgs()
    a.struct_size = C.sizeof(_lib.WgradArgs)
    a.n_rays, a.n_samples, a.n_partials = n_rays, S, kch
    a.acts, a.d_pre, a.pts4, a.d_raw4 = acts.data_ptr(), d_pre.data_ptr(), pts4.data_ptr(), g4.data_ptr()
    a.enc, a.g_head, a.partials = scratch[0].data_ptr(), scratch[1].data_ptr(), parts.data_ptr()
    if views:
        hv, d_pre_v = mk(nblk, W // 2, 32).abs(), mk(nblk, W // 2, 32)
        dirs = F.normalize(torch.randn(M, 3, generator=gen), dim=-1).to(DEV)
        a.dirs, a.hv, a.d_pre_v, a.encv = dirs.data_ptr(), hv.data_ptr(), d_pre_v.data_ptr(), scratch[2].data_ptr()
    _lib.check(model.lib.nrnerf_trunk_wgrad(model.handle, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nrnerf_trunk_wgrad")
    torch.cuda.synchronize()
    enc_t, g_t = scratch[0], scratch[1]
    want_enc = _block_tiles(training.posenc(pts4[:, :3], 10), n_rays, S).float()
    assert float((enc_t.float() - want_enc).abs().max()) <= 2.0 ** -7 and bool((enc_t[:, 63] == 0).all())
    assert torch.equal(g_t, _block_tiles(g4, n_rays, S))
    tot = parts.sum(0)
    o = 0
    dwh = tot[o:o + (D - 1) * W * W].view(D - 1, W, W); o += (D - 1) * W * W
    dwe = tot[o:o + 2 * W * 64].view(2, W, 64); o += 2 * W * 64
    dwo = tot[o:o + W * 64].view(W, 64); o += W * 64
    db = tot[o:o + (D + 1) * W].view(D + 1, W)
    A, Z = acts.float(), d_pre.float()

    def close(got, want, what):
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 1e-4 * scale, (what, float((got - want).abs().max()), scale)

    for i in range(1, D):
        close(dwh[i - 1], torch.einsum("bfs,bgs->fg", Z[i], A[i - 1]), f"hidden {i}")
        close(db[i], Z[i].sum((0, 2)), f"bias {i}")
    close(db[0], Z[0].sum((0, 2)), "bias 0")
    close(dwe[0], torch.einsum("bfs,bgs->fg", Z[0], enc_t.float()), "encoding, layer 0")
    close(dwe[1], torch.einsum("bfs,bgs->fg", Z[5], enc_t.float()), "encoding, skip layer")
    close(dwo, torch.einsum("bfs,bgs->fg", A[D - 1], g_t.float()), "head")
    if views:
        o += (D + 1) * W
        V = W // 2
        dwf = tot[o:o + V * W].view(V, W); o += V * W
        dwd = tot[o:o + V * 64].view(V, 64); o += V * 64
        dwr = tot[o:o + V * 64].view(V, 64); o += V * 64
        dbv = tot[o:o + V]
        assert o + V == stride
        encv_t = scratch[2]
        want_v = _block_tiles(training.posenc(dirs, 4), n_rays, S).float()
        assert float((encv_t.float() - want_v).abs().max()) <= 2.0 ** -7 and bool((encv_t[:, 27:] == 0).all())
        Zv, Hv = d_pre_v.float(), hv.float()
        close(dwf, torch.einsum("bfs,bgs->fg", Zv, A[D - 1]), "folded views layer")
        close(dbv, Zv.sum((0, 2)), "folded views bias")
        close(dwd, torch.einsum("bfs,bgs->fg", Zv, encv_t.float()), "direction columns")
        close(dwr, torch.einsum("bfs,bgs->fg", Hv, g_t.float()), "rgb_linear, transposed")


@pytest.mark.gpu
@pytest.mark.parametrize("width,n_rays,S,kch,views", [(256, 37, 192, 7, False), (256, 5, 85, 3, False), (256, 1, 3, 4, False), (128, 64, 64, 28, False),
                                                      (256, 7, 85, 5, True)],
                         ids=["w256", "w256_ragged", "w256_three_samples", "w128", "w256_viewdirs"])
def test_trunk_wgrad_fp32_kernel_vs_einsum(width, n_rays, S, kch, views):
    """nrnerf_trunk_wgrad in fp32 mode (trunk_wgrad_f32: v_mfma_f32_32x32x2_f32 over the row-major arrays the fp32 forward /
    backward kernels write) on random arrays against float64 einsums over the same values: hidden layers, the two encoding
    products, the head, the bias sums; sample counts that are no multiple of the kernel's group of eight and fewer samples
    than workgroups; both compiled trunk widths.  Exact fp32 products, fp32 accumulation in a different order: 2e-6 of
    scale.  The two operands the call builds itself (encoding rows, head-gradient rows) against torch.  ``views``: with the
    colour branch's three products (see the bf16 test)."""
    import ctypes as C
    from nonrigid_nerf_amd import _lib, training
    cfg = SceneConfig(N_importance=64, netwidth=width, use_viewdirs=views)
    scene = make_scene(cfg, 0)
    rb, coarse, fine = _modules(scene, requires_grad=False)
    R.set_precision("f32")
    model = R.get_model(coarse, fine, precision="f32", device=torch.device(DEV))
    D, W, M = 8, width, n_rays * S
    gen = torch.Generator().manual_seed(5)
    mk = lambda *shape: (torch.randn(*shape, generator=gen) * 0.5).to(DEV)
    acts, d_pre = mk(D, M, W).abs(), mk(D, M, W)
    pts4 = (torch.randn(M, 4, generator=gen) * 0.4).to(DEV)
    g4 = torch.randn(M, 4, generator=gen).to(DEV)
    scratch = torch.full((3, M, 64), float("nan"), device=DEV)
    stride = _lib.wgrad_stride_views(D, W) if views else _lib.wgrad_stride(D, W)
    parts = torch.zeros(kch, stride, device=DEV)          # the 64-column jobs fill fewer records: zero-filled by the caller
    a = _lib.WgradArgs()
    a.struct_size = C.sizeof(_lib.WgradArgs)
    a.n_rays, a.n_samples, a.n_partials = n_rays, S, kch
    a.acts, a.d_pre, a.pts4, a.d_raw4 = acts.data_ptr(), d_pre.data_ptr(), pts4.data_ptr(), g4.data_ptr()
    a.enc, a.g_head, a.partials = scratch[0].data_ptr(), scratch[1].data_ptr(), parts.data_ptr()
    if views:
        hv, d_pre_v = mk(M, W // 2).abs(), mk(M, W // 2)
        dirs = F.normalize(torch.randn(M, 3, generator=gen), dim=-1).to(DEV)
        a.dirs, a.hv, a.d_pre_v, a.encv = dirs.data_ptr(), hv.data_ptr(), d_pre_v.data_ptr(), scratch[2].data_ptr()
    _lib.check(model.lib.nrnerf_trunk_wgrad(model.handle, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nrnerf_trunk_wgrad")
    torch.cuda.synchronize()
    enc_r, g_r = scratch[0], scratch[1]
    assert float((enc_r[:, :63] - training.posenc(pts4[:, :3], 10)).abs().max()) <= 2e-6 and bool((enc_r[:, 63] == 0).all())
    assert torch.equal(g_r[:, :4], g4) and bool((g_r[:, 4:] == 0).all())
    tot = parts.double().sum(0)
    o = 0
    dwh = tot[o:o + (D - 1) * W * W].view(D - 1, W, W); o += (D - 1) * W * W
    dwe = tot[o:o + 2 * W * 64].view(2, W, 64); o += 2 * W * 64
    dwo = tot[o:o + W * 64].view(W, 64); o += W * 64
    db = tot[o:o + (D + 1) * W].view(D + 1, W)
    A, Z, E, G = acts.double(), d_pre.double(), enc_r.double(), g_r.double()

    def close(got, want, what):
        scale = float(want.abs().max())
        assert float((got - want).abs().max()) <= 2e-6 * scale, (what, float((got - want).abs().max()), scale)

    for i in range(1, D):
        close(dwh[i - 1], Z[i].t() @ A[i - 1], f"hidden {i}")
        close(db[i], Z[i].sum(0), f"bias {i}")
    close(db[0], Z[0].sum(0), "bias 0")
    close(dwe[0], Z[0].t() @ E, "encoding, layer 0")
    close(dwe[1], Z[5].t() @ E, "encoding, skip layer")
    close(dwo, A[D - 1].t() @ G, "head")
    if views:
        o += (D + 1) * W
        V = W // 2
        dwf = tot[o:o + V * W].view(V, W); o += V * W
        dwd = tot[o:o + V * 64].view(V, 64); o += V * 64
        dwr = tot[o:o + V * 64].view(V, 64); o += V * 64
        dbv = tot[o:o + V]
        assert o + V == stride
        encv_r = scratch[2]
        assert float((encv_r[:, :27] - training.posenc(dirs, 4)).abs().max()) <= 2e-6 and bool((encv_r[:, 27:] == 0).all())
        Zv, Hv, Ev = d_pre_v.double(), hv.double(), encv_r.double()
        close(dwf, Zv.t() @ A[D - 1], "folded views layer")
        close(dbv, Zv.sum(0), "folded views bias")
        close(dwd, Zv.t() @ Ev, "direction columns")
        close(dwr, Hv.t() @ G, "rgb_linear, transposed")


@pytest.mark.gpu
@pytest.mark.parametrize("S,I,details", [(64, 64, True), (64, 128, True), (37, 11, False), (128, 128, True)])
def test_merge_rows_kernel_vs_gather_both_directions(S, I, details):
    """nrnerf_merge_rows (the split fine bender's row merge): forward against a sort of the depths, inverse = the
    permutation undone, and -- under autograd, through training._MergeRows -- gradients against torch.gather's."""
    from nonrigid_nerf_amd import training
    N = 53
    gen = torch.Generator().manual_seed(S * 131 + I)
    zc = torch.sort(torch.rand(N, S, generator=gen), 1).values
    zn = torch.sort(torch.rand(N, I, generator=gen), 1).values
    zm, order = torch.sort(torch.cat([zc, zn], 1), dim=1, stable=True)
    rank_new = torch.argsort(order, 1)[:, S:].to(torch.uint8).to(DEV)        # row of new sample i among the merged depths
    mk = lambda n, k: torch.randn(N, n, 4, generator=gen).to(DEV)[..., :k].requires_grad_(True)
    c4, n4 = torch.randn(N, S, 4, generator=gen).to(DEV).requires_grad_(True), torch.randn(N, I, 4, generator=gen).to(DEV).requires_grad_(True)
    cu, nu = mk(S, 3), mk(I, 3)
    idx = order.to(DEV)

    def want(c, n):
        both = torch.cat([c, n], 1)
        return both.gather(1, idx[..., None].expand(N, S + I, both.shape[-1]))

    if details:
        bent, unm, mask = training._MergeRows.apply(c4[..., :3], cu, c4[..., 3:4], n4[..., :3], nu, n4[..., 3:4], rank_new)
        assert torch.equal(bent, want(c4, n4)[..., :3]) and torch.equal(mask, want(c4, n4)[..., 3:4]) and torch.equal(unm, want(cu, nu))
        w1, w2, w3 = (torch.randn_like(t) for t in (bent, unm, mask))
        ((bent * w1).sum() + (unm * w2).sum() + (mask * w3).sum()).backward()
        got = [t.grad.clone() for t in (c4, n4, cu, nu)]
        for t in (c4, n4, cu, nu):
            t.grad = None
        m4, mu = want(c4, n4), want(cu, nu)
        ((m4[..., :3] * w1).sum() + (mu * w2).sum() + (m4[..., 3:4] * w3).sum()).backward()
        for g, t in zip(got, (c4, n4, cu, nu)):
            assert torch.equal(g, t.grad)
    else:
        bent, unm, mask = training._MergeRows.apply(c4[..., :3], None, None, n4[..., :3], None, None, rank_new)
        assert unm is None and mask is None and torch.equal(bent, want(c4, n4)[..., :3])
        w1 = torch.randn_like(bent)
        (bent * w1).sum().backward()
        got = [c4.grad.clone(), n4.grad.clone()]
        c4.grad = n4.grad = None
        (want(c4, n4)[..., :3] * w1).sum().backward()
        assert torch.equal(got[0], c4.grad) and torch.equal(got[1], n4.grad)


@pytest.mark.gpu
def test_reduce_partials_kernel_vs_sum_and_index():
    """nrnerf_reduce_partials: records added in the documented fixed order into an arbitrary layout; flagged positions stop at the short count
    (whatever the later records hold -- NaN here -- is never read), negative positions give 0."""
    from nonrigid_nerf_amd import _lib, training
    P, stride, n_short = 11, 5000, 4
    gen = torch.Generator().manual_seed(3)
    parts = torch.randn(P, stride, generator=gen).to(DEV)
    short_cols = torch.arange(1000, 1300)
    parts[n_short:, short_cols.to(DEV)] = float("nan")
    index = torch.randint(0, stride, (7001,), generator=gen).to(torch.int32)
    is_short = (index >= 1000) & (index < 1300)
    pad = torch.rand(index.shape, generator=gen) < 0.1
    coded = torch.where(is_short, index | _lib.REDUCE_SHORT, index)
    coded = torch.where(pad, torch.full_like(coded, -1), coded).to(DEV)
    got = training._reduce_partials(parts, n_short, coded)
    torch.cuda.synchronize()
    def in_kernel_order(n_records):                       # eight interleaved groups, each in order, then the groups in order
        groups = []
        for g in range(8):
            acc = torch.zeros(stride, device=DEV)
            for p_ in range(g, n_records, 8):
                acc = acc + parts[p_].nan_to_num(0.0)
            groups.append(acc)
        tot = groups[0]
        for g in range(1, 8):
            tot = tot + groups[g]
        return tot
    full, short = in_kernel_order(P), in_kernel_order(n_short)
    want = torch.where(is_short.to(DEV), short[index.long().to(DEV)], full[index.long().to(DEV)])
    want = torch.where(pad.to(DEV), torch.zeros_like(want), want)
    assert torch.equal(got, want)
    # nrnerf_reduce_partials_aux: the column sums of a second array land at four chosen positions (index -2 there: left alone by the
    # regular reduction), everything else as above; a skipped channel (-1) keeps what the buffer held; twice the same bits
    for n_aux in (1, 63, 6144, 16384):
        aux = torch.randn(n_aux, 4, generator=gen).to(DEV)
        pos = [17, 6000, -1, 3]
        coded2 = coded.clone()
        for p_ in pos:
            if p_ >= 0:
                coded2[p_] = -2
        outs = [training._reduce_partials(parts, n_short, coded2, aux, pos) for _ in range(2)]
        torch.cuda.synchronize()
        assert torch.equal(outs[0][[17, 6000, 3]], outs[1][[17, 6000, 3]])
        keep = torch.ones(7001, dtype=torch.bool, device=DEV)
        keep[[17, 6000, 3]] = False
        assert torch.equal(outs[0][keep], want[keep])
        ref = aux.double().sum(0)
        for c, p_ in enumerate(pos):
            if p_ >= 0:
                assert abs(float(outs[0][p_]) - float(ref[c])) <= 1e-5 * (float(aux[:, c].abs().sum()) + 1e-20), (n_aux, c)


@pytest.mark.gpu
def test_tile_row_sums_kernel_vs_torch():
    """nrnerf_tile_row_sums: rows of 32 bf16 added in fp32 (the per-ray bias gradient of the time-conditioned baseline)."""
    from nonrigid_nerf_amd import _lib
    gen = torch.Generator().manual_seed(9)
    for n_rows in (1, 255, 70001):
        x = torch.randn(n_rows, 32, generator=gen).to(torch.bfloat16).to(DEV)
        out = torch.full((n_rows,), float("nan"), device=DEV)
        _lib.check(_lib.load().nrnerf_tile_row_sums(x.data_ptr(), n_rows, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "nrnerf_tile_row_sums")
        torch.cuda.synchronize()
        want = x.double().sum(1)
        assert float((out.double() - want).abs().max()) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("W,S", [(256, 128), (256, 85), (128, 64)])
def test_tiles_to_rows_kernel_vs_permute(W, S):
    """nrnerf_tiles_to_rows: [block][feature][32 samples] bf16 tiles -> [ray][sample][feature] rows, ragged sample counts."""
    from nonrigid_nerf_amd import _lib
    N, bpr = 19, (S + 31) // 32
    gen = torch.Generator().manual_seed(S)
    tiles = torch.randn(N * bpr, W, 32, generator=gen).to(torch.bfloat16).to(DEV)
    rows = torch.full((N, S, W), float("nan"), dtype=torch.bfloat16, device=DEV)
    _lib.check(_lib.load().nrnerf_tiles_to_rows(tiles.data_ptr(), N, S, W, rows.data_ptr(), torch.cuda.current_stream().cuda_stream), "nrnerf_tiles_to_rows")
    torch.cuda.synchronize()
    want = tiles.view(N, bpr, W, 32).permute(0, 1, 3, 2).reshape(N, bpr * 32, W)[:, :S]
    assert torch.equal(rows, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-6), (torch.bfloat16, 8e-3)])
def test_direction_encoding_kernel_vs_torch_autograd(dtype, tol):
    """nrnerf_direction_encoding (training._DirectionEncoding) against finite_difference_dirs + posenc under autograd:
    the encoding rows and the gradient wrt the bent points (through the encoding, the normalisation, both differences a
    point takes part in, and sample 0 sharing sample 1's direction)."""
    from nonrigid_nerf_amd import training
    N, S, L = 37, 53, 4
    gen = torch.Generator().manual_seed(2)
    walk = torch.cumsum(torch.rand(N, S, 3, generator=gen) * 0.02 + 0.001, 1) + torch.randn(N, 1, 3, generator=gen)      # points marching along a ray
    b4 = torch.zeros(N, S, 4)
    b4[..., :3] = walk
    b4 = b4.to(DEV).requires_grad_(True)
    bent = b4[..., :3]
    enc = training._DirectionEncoding.apply(bent, L, dtype)
    want = training.posenc(training.finite_difference_dirs(bent), L).reshape(N * S, -1)
    assert enc.dtype == dtype and float((enc.float() - want).abs().max()) <= tol
    w = torch.randn(N * S, 3 + 6 * L, generator=gen).to(DEV)
    (enc.float() * w).sum().backward()
    got = b4.grad.clone()
    b4.grad = None
    (want * w).sum().backward()
    scale = float(b4.grad.abs().max())
    assert float((got - b4.grad).abs().max()) <= (2e-5 if dtype == torch.float32 else 2e-2) * scale, (float((got - b4.grad).abs().max()), scale)
    assert float(got[..., 3].abs().max()) == 0.0


def _oracle_leaves(scene):
    from oracle import nrnerf_oracle as O
    sc = O.scene_on(scene, DEV)
    leaves = {}
    for part in ("bender", "coarse", "fine"):
        d = getattr(sc, part)
        if d is None:
            continue
        for k in d:
            d[k] = d[k].clone().requires_grad_(True)
            leaves[(part, k)] = d[k]
    return sc, leaves


@pytest.mark.gpu
@pytest.mark.parametrize("bend_depth,exact,knobs", [(5, False, {}), (5, True, {}), (7, False, {}),
                                                     (5, False, dict(rigidity_test_time_cutoff=0.5, test_time_scaling=0.7))],
                         ids=["approx", "exact", "deep_bender", "knobs"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_native_divergence_regulariser_vs_autograd_double_backward(precision, bend_depth, exact, knobs):
    """compute_divergence_loss (run_nerf_helpers.py:22-116) on the HIP library -- one forward-mode tangent through the
    bender, two-chain backward (nrnerf_bender_divergence_*) -- against the oracle's restatement, which does what the
    reference does: a vector-Jacobian product with create_graph=True and autograd's double backward.  Same seed, so the
    same probe vectors (drawn per chunk: 3 chunks here).  Value per ray and every gradient (all bender tensors, the latent
    codes) within 1e-4 of scale (forward / backward-data kernels: exact fp32 whatever the model's precision; the weight-gradient
    contraction of a bf16 model rounds its operands to bf16: 1e-2)."""
    from oracle import nrnerf_oracle as O
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(N_importance=64, bend_depth=bend_depth)
    scene = make_scene(cfg, 3)
    rb, coarse, fine = _modules(scene)
    rb.rigidity_test_time_cutoff = knobs.get("rigidity_test_time_cutoff")
    rb.test_time_scaling = knobs.get("test_time_scaling")
    R.set_precision(precision)
    R.get_model(coarse, fine)                                  # what a render call leaves behind: the packed model of this bender
    n_rays, S = 83, 61                                         # 5063 points: not a multiple of 32
    g = torch.Generator().manual_seed(5)
    pts = ((torch.rand(n_rays * S, 3, generator=g) - 0.5) * 1.2).to(DEV)
    codes = (torch.randn(6, cfg.latent_size, generator=g) * 0.1).to(DEV).requires_grad_(True)
    ids = torch.randint(0, 6, (n_rays,), generator=g).to(DEV)
    w = torch.rand(n_rays * S, generator=g).to(DEV)

    def expand(c):
        lat = c[ids]
        return lat.view(n_rays, 1, -1).expand(n_rays, S, lat.shape[-1]).reshape(-1, lat.shape[-1])     # train.py:256-262

    torch.manual_seed(31)
    ours = training.compute_divergence_loss(None, pts.clone(), expand(codes), rb, exact, 2048, n_rays, weights=w, backprop_into_weights=False)
    assert ours.shape == (n_rays,) and ours.requires_grad
    ours.mean().backward()
    sc, leaves = _oracle_leaves(scene)
    codes_o = codes.detach().clone().requires_grad_(True)
    torch.manual_seed(31)
    want = O.compute_divergence_loss(pts.clone(), expand(codes_o), sc.bender, exact, 2048, n_rays, weights=w, backprop_into_weights=False,
                                     knobs=O.Knobs(**knobs))
    want.mean().backward()
    scale = float(want.abs().max())
    assert scale > 0 and float((ours.detach() - want.detach()).abs().max()) <= 1e-4 * scale, (float((ours.detach() - want.detach()).abs().max()), scale)
    named = dict(rb.named_parameters())
    worst = 0.0
    for (part, k), leaf in leaves.items():
        if part != "bender":
            continue
        gs = float(leaf.grad.abs().max()) + 1e-20
        err = float((named[k].grad - leaf.grad).abs().max()) / gs
        worst = max(worst, err)
        assert err <= (1e-4 if precision == "f32" else 1e-2), (k, err)
    gs = float(codes_o.grad.abs().max()) + 1e-20
    assert float((codes.grad - codes_o.grad).abs().max()) / gs <= 1e-4
    # after both runs the generator is in the same state (the probes were drawn in the same amounts)
    print(f"\n[divergence {precision} depth {bend_depth} exact={exact} knobs={bool(knobs)}] worst gradient error / scale: {worst:.1e}")


@pytest.mark.gpu
@pytest.mark.parametrize("native_bender", [False, True], ids=["torch_ops_bender", "native_bender"])
def test_native_full_training_iteration_vs_oracle_and_reference_golden(native_bender):
    """The reference's training iteration with the shipped loss weights (configs/example_sequence.txt: offsets 60,
    divergence 3, rigidity 5e-4; 64 + 64 samples, perturb, raw noise) through the drop-in entry points -- render_rays
    under autograd with detailed outputs, compute_divergence_loss -- in fp32 mode, no eager reference-module call anywhere:
      (1) against the oracle's restatement on THIS device with the same seed, evaluated at the merged depths this path
          chose: per-ray loss 1e-4, every gradient tensor 2e-3 of scale (5e-2 for bender / latent tensors with the
          native bender, whose bent points differ from torch's by an ulp; see test_fp32_gradients_vs_oracle_autograd);
      (2) against the REFERENCE's own result on the CPU (tests/golden/train_step_64_64.npz; different random stream, so
          only what does not depend on it: shapes, and that the oracle on the CPU reproduces it -- tests/test_oracle_golden.py)."""
    from nonrigid_nerf_amd import training
    from tests.test_oracle_golden import load_train_step_golden, oracle_train_step
    ts, scene, rays, codes, image_ids, target, z = load_train_step_golden()
    rb, coarse, fine = _modules(scene)
    R.set_precision("f32")
    codes_d = codes.to(DEV).requires_grad_(True)
    lat = codes_d[image_ids.to(DEV)]
    kw = dict(network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=ts["N_samples"], N_importance=ts["N_importance"],
              perturb=ts["perturb"], raw_noise_std=ts["raw_noise_std"], _want_z_vals=True)
    saved = (training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER)
    training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = native_bender, False, native_bender
    try:
        torch.manual_seed(ts["render_seed"])
        loss, extras = training.training_loss(rays.to(DEV), lat, target.to(DEV), kw, offsets_loss_weight=ts["offsets_loss_weight"],
                                              divergence_loss_weight=ts["divergence_loss_weight"], rigidity_loss_weight=ts["rigidity_loss_weight"],
                                              global_step=ts["global_step"], N_iters=ts["N_iters"], chunk=ts["chunk"])
        loss.mean().backward()
    finally:
        training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = saved
    assert tuple(loss.shape) == tuple(z["out__loss_per_ray"].shape)
    l_ref, g_ref, _ = oracle_train_step(ts, scene, rays, codes, image_ids, target, device=DEV, z_fine_override=extras["_z_vals"].detach())
    assert float((loss.detach() - l_ref).abs().max()) <= 1e-4 * float(l_ref.abs().max()), float((loss.detach() - l_ref).abs().max())
    named = _named(rb, coarse, fine)
    ours = {("codes", ""): codes_d.grad}
    ours.update({k: p.grad for k, p in named.items() if p.grad is not None})
    assert set(ours) == set(g_ref), set(ours) ^ set(g_ref)
    rows = []
    for k, gr in g_ref.items():
        scale = float(gr.abs().max()) + 1e-20
        err = float((ours[k] - gr).abs().max()) / scale
        rows.append((err, k))
        bar = 5e-2 if (native_bender and k[0] in ("bender", "codes")) else 2e-3
        assert err <= bar, (k, err, bar)
    rows.sort(reverse=True)
    print(f"\n[full training iteration, fp32, native_bender={native_bender}] loss max err {float((loss.detach() - l_ref).abs().max()):.2e}; "
          "worst gradient tensors (err / scale): " + "; ".join(f"{k[0]}.{k[1]} {e:.1e}" for e, k in rows[:5]))
    # every parameter the reference's step gives a gradient to got one here, and nothing else
    ref_keys = {tuple(k.split("__", 2)[1:]) for k in z.files if k.startswith("gradnorm__")}
    assert {k for k in ours if k[0] != "codes"} == ref_keys


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("native_bender", [False, True], ids=["torch_ops_bender", "native_bender"])
def test_two_pass_backward_with_retain_graph_like_the_reference_loop(native_bender, precision):
    """train.py:1594-1608: rays of TEST images only optimise their latent codes -- the reference masks the per-ray losses
    with the test indicator, calls ``backward(retain_graph=True)``, resets the gradients of every network weight (the codes
    keep theirs), then back-propagates the training rays' mean WITHOUT retain_graph.  So every native autograd Function of
    an iteration runs its backward TWICE on the same saved arrays.  Both precisions: the two passes against ONE pass over
    the same graph with the equivalent combined loss (weights: training rays only; codes: all rays), 1e-5 of scale (measured:
    bit-identical in bf16 mode); fp32 additionally against the oracle's autograd doing the same two passes on this device at
    the same merged depths (bars of the full-iteration test above)."""
    from nonrigid_nerf_amd import training
    from oracle import nrnerf_oracle as O
    cfg = SceneConfig(N_importance=64)
    scene = make_scene(cfg, 0)
    n = 48
    rays, lat_cpu = make_rays(n, 5, cfg)
    target = torch.linspace(0.1, 0.9, 3).expand(n, 3).contiguous().to(DEV)
    is_test = (torch.arange(n) % 3 == 0).to(DEV).float()
    w = dict(offsets_loss_weight=60.0, divergence_loss_weight=3.0, rigidity_loss_weight=0.0005, global_step=100000, chunk=32768)
    R.set_precision(precision)
    saved = (training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER)
    training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = native_bender, False, native_bender

    def ours(two_pass):
        rb, coarse, fine = _modules(scene)
        lat = lat_cpu.to(DEV).requires_grad_(True)
        kw = dict(network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=64, N_importance=64, perturb=1.0,
                  raw_noise_std=1.0, _want_z_vals=True)
        torch.manual_seed(11)
        loss, extras = training.training_loss(rays.to(DEV), lat, target, kw, N_iters=200000, **w)
        named = _named(rb, coarse, fine)
        if two_pass:
            (is_test * loss).mean().backward(retain_graph=True)                  # train.py:1595-1598
            assert any(p.grad is not None for p in named.values())
            for p in named.values():
                p.grad = None                                                    # train.py:1599-1604
            ((1 - is_test) * loss).mean().backward()                            # train.py:1606-1608
        else:
            # one pass with the same result: the weights see the training rays only, the codes all rays
            g_lat_test, = torch.autograd.grad((is_test * loss).mean(), lat, retain_graph=True)
            ((1 - is_test) * loss).mean().backward()
            lat.grad = lat.grad + g_lat_test
        grads = {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None}
        grads[("codes", "")] = lat.grad.detach().clone()
        return loss.detach(), grads, extras["_z_vals"].detach()

    try:
        loss, g2, z = ours(True)
        # (1) the two passes against ONE pass over the same graph: exercises exactly the re-entrancy of the native Functions
        _, g1, _ = ours(False)
        assert set(g2) == set(g1)
        for k in g1:
            err = float((g2[k] - g1[k]).abs().max()) / (float(g1[k].abs().max()) + 1e-20)
            assert err <= 1e-5, ("two passes vs one", k, err)
        if precision == "f32":
            # (2) and against the oracle's autograd doing the reference's two passes
            sc, leaves = _oracle_leaves(scene)
            lat_o = lat_cpu.to(DEV).clone().requires_grad_(True)
            torch.manual_seed(11)
            loss_o, _ = O.training_loss(rays.to(DEV), lat_o, sc, target, n_iters=200000, z_fine_override=z, **w)
            (is_test * loss_o).mean().backward(retain_graph=True)
            for t in leaves.values():
                t.grad = None
            ((1 - is_test) * loss_o).mean().backward()
            g_ref = {k: t.grad for k, t in leaves.items() if t.grad is not None}
            g_ref[("codes", "")] = lat_o.grad
            assert float((loss - loss_o.detach()).abs().max()) <= 1e-4 * float(loss_o.abs().max())
            # bender / latent tensors pass through the 2^9 encoding frequency: an ulp of a bent point is 1e-2 of their scale
            # (measured here: 8.4e-3 with the torch-op bender, whose points equal the oracle's only up to the GEMM's batch shape)
            bar = lambda k: (5e-2 if native_bender else 2e-2) if k[0] in ("bender", "codes") else 2e-3
        else:
            g_ref = g1
            bar = lambda k: 1e-5       # the same kernels on the same saved arrays: only the ORDER of two fp32 additions differs
    finally:
        training.NATIVE_BENDER, training.BATCHED_BENDER, training.SPLIT_FINE_BENDER = saved
    assert set(g2) == set(g_ref), set(g2) ^ set(g_ref)
    worst = max((float((g2[k] - g_ref[k]).abs().max()) / (float(g_ref[k].abs().max()) + 1e-20), k) for k in g_ref)
    print(f"\n[two-pass backward, {precision}, native_bender={native_bender}] worst gradient error / scale {worst[0]:.1e} ({worst[1]})")
    for k in g_ref:
        err = float((g2[k] - g_ref[k]).abs().max()) / (float(g_ref[k].abs().max()) + 1e-20)
        assert err <= bar(k), (k, err)


@pytest.mark.gpu
def test_training_iteration_replayed_from_a_hip_graph():
    """training.GraphedStep: the whole iteration (device-side weight re-pack, forward with fresh random numbers, the shipped
    loss, backward, Adam) captured once and replayed.  The replays must train (loss falls on a fixed batch; the random numbers of
    the stochastic branches come from torch's generator, whose Philox offsets torch advances per replay) and after ``sync()`` the packed
    weights the no-grad render uses are the trained ones (equal to a handle built from scratch)."""
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(N_importance=64)
    rb, coarse, fine = training._fresh_training_modules(cfg, torch.device(DEV), 64)
    params = []
    for m in (rb, coarse, fine):
        m.requires_grad_(True)
        params += list(m.parameters())
    codes = torch.zeros(4, cfg.latent_size, device=DEV, requires_grad=True)
    opt = torch.optim.Adam(params + [codes], lr=5e-4, fused=True, capturable=True)
    rays, _ = make_rays(256, 5, cfg)
    rays = rays.to(DEV)
    frame = torch.randint(0, 4, (256,), device=DEV)
    target = 0.5 + 0.4 * torch.sin(3.0 * rays[:, 3:6])
    kw = dict(network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=64, N_importance=64, perturb=1.0, raw_noise_std=1.0)
    R.set_precision("bf16")

    def loss_of(rays, target, frame, global_step):
        loss, _ = training.training_loss(rays, codes[frame], target, kw, offsets_loss_weight=60.0, divergence_loss_weight=3.0,
                                         rigidity_loss_weight=0.0005, global_step=global_step, N_iters=200000, chunk=32768)
        return loss.mean()

    gstep = torch.zeros((), device=DEV)
    graphed = training.GraphedStep(loss_of, dict(rays=rays, target=target, frame=frame, global_step=gstep), opt, [coarse])
    losses = [float(graphed(global_step=gstep.fill_(float(i)))) for i in range(60)]
    assert all(l == l for l in losses)
    assert sum(losses[-10:]) / 10 < 0.8 * sum(losses[:5]) / 5, (losses[:5], losses[-10:])
    graphed.sync()
    with torch.no_grad():
        got = R.batchify_rays(rays, {"ray_bending_latents": codes[frame].detach()}, chunk=32768, **{**kw, "perturb": 0.0, "raw_noise_std": 0.0})
        R.invalidate(coarse)
        want = R.batchify_rays(rays, {"ray_bending_latents": codes[frame].detach()}, chunk=32768, **{**kw, "perturb": 0.0, "raw_noise_std": 0.0})
    assert torch.equal(got["rgb_map"], want["rgb_map"]), "after sync() the packed weights must be the trained parameters"
    print(f"\n[graphed training step] loss {losses[0]:.4f} -> {losses[-1]:.4f} over 60 replays")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fused", "foreach", "plain"])
def test_an_optimiser_step_of_any_kind_reaches_the_packed_weights(kind):
    """torch.optim.Adam(fused=True) leaves Tensor._version alone (torch 2.10), so the handle's staleness check also counts
    optimiser steps (render._watch_optimizers): after ONE step of a fused / foreach / plain Adam the next render must use
    the stepped weights -- equal, bit for bit, to a handle packed from scratch (render.invalidate) -- and differ from the
    render before the step."""
    cfg = SceneConfig(N_importance=64)
    scene = make_scene(cfg, 2)
    rb, coarse, fine = _modules(scene)
    params = [p for m in (rb, coarse, fine) for p in m.parameters()]
    opt = torch.optim.Adam(params, lr=1e-2, fused=True) if kind == "fused" else torch.optim.Adam(params, lr=1e-2, foreach=(kind == "foreach"))
    rays, lat = make_rays(64, 1, cfg)
    rays, lat = rays.to(DEV), lat.to(DEV)
    R.set_precision("bf16")
    kw = dict(N_samples=cfg.N_samples, N_importance=cfg.N_importance, network_fine=fine, additional_pixel_information={"ray_bending_latents": lat})

    def render():
        with torch.no_grad():
            return R.render_rays(rays, coarse, **kw)["rgb_map"].clone()

    before = render()
    g = torch.Generator().manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    after = render()
    assert not torch.equal(after, before), "the step did not reach the packed weights"
    R.invalidate(coarse)
    assert torch.equal(render(), after)


@pytest.mark.gpu
@pytest.mark.parametrize("with_rgb0,with_offsets,with_div,S,rows4,mean", [(True, True, True, 64, True, True), (False, True, False, 83, False, False),
                                                                          (True, False, True, 37, False, True), (True, False, False, 64, False, False),
                                                                          (True, True, True, 83, True, False)])
def test_fused_loss_kernel_vs_torch_autograd(with_rgb0, with_offsets, with_div, S, rows4, mean):
    """nrnerf_loss_forward / _backward (csrc/nrnerf_loss.hip; training._FusedLoss) against the same terms written as the reference writes
    them (train.py:207-287, rnh:10-13, 61-69) under torch.autograd: per-ray loss and every gradient, incl. torch's conventions at the
    singular points (a zero offset vector: d|x|/dx = 0, d(n^e)/de = 0).  ``rows4``: offsets and rigidity as the xyz / w parts of [N,S,4] rows
    (what render_rays hands out; read where they lie).  ``mean``: the mean over the rays from the kernel's own launch and its gradient handed
    back as a scalar, against loss.mean() -- twice, the counter behind it has to be back at zero."""
    from nonrigid_nerf_amd import training
    g = torch.Generator().manual_seed(S)
    N = 301
    mk = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    rgb_map, rgb0, target = torch.sigmoid(mk(N, 3)).requires_grad_(True), torch.sigmoid(mk(N, 3)).requires_grad_(True), torch.rand(N, 3, generator=g).to(DEV)
    w = torch.rand(N, S, generator=g).to(DEV)
    off = (0.01 * mk(N, S, 3))
    off[::7, ::5] = 0.0                                   # singular points
    rig = torch.rand(N, S, 1, generator=g).to(DEV)
    rig[::11, ::3] = 1.0
    if rows4:           # leaves = the [N,S,4] rows; the loss sees two views of them
        rows_a = torch.cat([off, torch.zeros(N, S, 1, device=DEV)], -1).requires_grad_(True)
        rows_b = torch.cat([torch.zeros(N, S, 3, device=DEV), rig], -1).requires_grad_(True)
        off, rig = rows_a[..., :3], rows_b[..., 3:4]
    else:
        off = off.requires_grad_(True)
        rig = rig.requires_grad_(True)
    alpha = 3.0 * mk(N, S)
    div = mk(N * S).requires_grad_(True)
    ow, rw, dw = 60.0 * 0.37, 5e-4, 3.0 * 0.37
    upstream = torch.rand(N, generator=g).to(DEV)

    def eager():
        img2mse = lambda x, y: torch.mean(((x - y) ** 2).view(N, -1), dim=1)
        loss = img2mse(rgb_map, target)
        if with_rgb0:
            loss = loss + img2mse(rgb0, target)
        if with_offsets:
            wf = w.detach().view(-1)
            ol = torch.mean((wf * torch.pow(torch.norm(off.view(-1, 3), dim=-1), 2.0 - rig.view(-1))).view(N, -1), dim=-1)
            ol = ol + rw * torch.mean((wf * rig.view(-1)).view(N, -1), dim=-1)
            loss = loss + ow * ol
        if with_div:
            wd = (1.0 - torch.exp(-torch.relu(alpha.view(-1)))).detach()
            loss = loss + dw * torch.mean((wd * torch.abs(div) ** 2).view(N, -1), dim=-1)
        return loss, loss.mean()

    def fused():
        return training._FusedLoss.apply(rgb_map, rgb0 if with_rgb0 else None, target, w if with_offsets else None, off if with_offsets else None,
                                         rig if with_offsets else None, alpha if with_div else None, div if with_div else None,
                                         ow if with_offsets else 0.0, rw, dw if with_div else 0.0, None, mean)

    leaves = [rgb_map, rgb0, rows_a if rows4 else off, rows_b if rows4 else rig, div]
    res = {}
    for name, fn in (("eager", eager), ("fused", fused), ("fused again", fused)):
        for t in leaves:
            t.grad = None
        loss, m = fn()
        if mean:
            assert m is not None and abs(float(m) - float(loss.mean())) <= 2e-6 * abs(float(loss.mean())), (name, float(m), float(loss.mean()))
            ((loss * upstream).sum() + 7.0 * m).backward()
        else:
            assert name == "eager" or m is None
            (loss * upstream).sum().backward()
        res[name] = (loss.detach().clone(), [None if t.grad is None else t.grad.clone() for t in leaves])
    assert torch.equal(res["fused"][0], res["fused again"][0])
    le, lf = res["eager"][0], res["fused"][0]
    assert torch.allclose(le, lf, rtol=2e-5, atol=1e-7), float((le - lf).abs().max())
    for nm, ge, gf in zip(("rgb_map", "rgb0", "offsets", "rigidity", "divergence"), res["eager"][1], res["fused"][1]):
        if ge is None:
            assert gf is None or float(gf.abs().max()) == 0.0, nm
            continue
        assert gf is not None and torch.isfinite(gf).all(), nm
        scale = float(ge.abs().max()) + 1e-20
        assert float((ge - gf).abs().max()) <= 2e-5 * scale, (nm, float((ge - gf).abs().max()) / scale)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,tol", [("f32", 2e-5), ("bf16", 2e-2)])
@pytest.mark.parametrize("frozen_bender", [False, True], ids=["trained_bender", "frozen_bender"])
@pytest.mark.parametrize("pooled", [False, True], ids=["reference_draw_order", "pooled_draws"])
def test_divergence_term_riding_on_the_coarse_bender_evaluation_gives_the_same_gradients(precision, tol, frozen_bender, pooled):
    """training_loss with SHARED_DIVERGENCE (the divergence regulariser's backward and the coarse samples' bender backward as ONE
    nrnerf_bender_divergence_backward that takes the render pass' cotangents too -- training._DivergenceOnBender) against the two separate
    autograd nodes the reference's graph has (train.py:245-287 on top of :221-242): same random draws, same loss, every gradient equal up
    to the order of additions (fp32) / to the 16-bit arrays' rounding (bf16: the shared pass reads the activations the divergence forward
    saved, the separate one those of the render's own bender forward); with the bender frozen the latent codes still get both terms.
    ``pooled_draws``: the probe vectors are known before the render, so the divergence FORWARD is the coarse samples' bender evaluation too
    (nrnerf_divergence_args.bent4; no nrnerf_bender_forward launch for them) -- against the separate nodes fed the same pooled numbers."""
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(N_importance=64)
    scene = make_scene(cfg, 1)
    rays, latents = make_rays(300, 3, cfg)
    target = torch.rand(300, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    R.set_precision(precision)
    out = {}
    try:
        for shared in (False, True):
            rb, coarse, fine = _modules(scene)
            if frozen_bender:
                rb.requires_grad_(False)
            lat = latents.to(DEV).requires_grad_(True)
            kw = dict(network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=64, N_importance=64, perturb=1.0, raw_noise_std=1.0)
            old, training.SHARED_DIVERGENCE = training.SHARED_DIVERGENCE, shared
            old_pool, training.POOLED_DRAWS = training.POOLED_DRAWS, pooled
            try:
                torch.manual_seed(11)
                loss, _ = training.training_loss(rays.to(DEV), lat, target, kw, offsets_loss_weight=60.0, divergence_loss_weight=3.0,
                                                 rigidity_loss_weight=5e-4, global_step=120000, N_iters=200000, mean=True)
                loss.backward()
            finally:
                training.SHARED_DIVERGENCE, training.POOLED_DRAWS = old, old_pool
            grads = {k: p.grad.clone() for k, p in _named(rb, coarse, fine).items() if p.grad is not None}
            grads[("latents", "")] = lat.grad.clone()
            out[shared] = (loss.detach().clone(), grads)
    finally:
        R.set_precision("f32")
    # (reference draw order: the forward is the same launches either way; pooled: the bent points come from another kernel's instance of
    #  the same arithmetic)
    assert torch.allclose(out[True][0], out[False][0], rtol=(5e-3 if pooled else 1e-6), atol=1e-8)
    assert set(out[True][1]) == set(out[False][1])
    assert frozen_bender == (not any(k[0] == "bender" for k in out[True][1]))
    # pooled: the two kernels' bent points agree to ONE ulp (1.2e-7, tools/experiments/r06_compare_bender_forwards.py), and an ulp of a bent
    # point is 1e-2 of the scale of every gradient behind the 2^9 encoding frequency (the golden test's docstring): the loose bar of the
    # native-bender comparisons applies; the tight check of the shared backward is the reference-draw-order variant
    # (measured on 300 rays: worst element 8e-2 of a tensor's scale, cosine > 0.999 -- hence direction + a bar on the worst element)
    for k, ge in out[False][1].items():
        gs = out[True][1][k]
        scale = float(ge.abs().max()) + 1e-20
        err = float((ge - gs).abs().max()) / scale
        if pooled:
            cos = float(torch.nn.functional.cosine_similarity(ge.flatten().double(), gs.flatten().double(), dim=0))
            assert cos >= 0.995 and err <= 0.2, (k, cos, err)
        else:
            assert err <= tol, (k, err)


@pytest.mark.gpu
@pytest.mark.parametrize("lindisp,jitter", [(False, True), (True, True), (False, False)])
def test_sample_depths_points_kernel_equals_the_reference_expression_bit_for_bit(lindisp, jitter):
    """nrnerf_sample_depths_points: the coarse depths as nrnerf_sample_depths writes them and, from the same launch, the sample points
    ``rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]`` (train.py:871-873) with torch's own two roundings."""
    from nonrigid_nerf_amd import _lib
    cfg = SceneConfig()
    rays, _ = make_rays(777, 4, cfg)
    rays = rays.to(DEV).contiguous()
    N, S = 777, 37
    u = torch.rand(N, S, generator=torch.Generator().manual_seed(5)).to(DEV) if jitter else None
    z0, z1 = torch.empty(N, S, device=DEV), torch.empty(N, S, device=DEV)
    pts = torch.empty(N, S, 3, device=DEV)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    _lib.check(lib.nrnerf_sample_depths(rays.data_ptr(), int(rays.shape[1]), u.data_ptr() if jitter else None, N, S, int(lindisp), z0.data_ptr(), st), "d")
    _lib.check(lib.nrnerf_sample_depths_points(rays.data_ptr(), int(rays.shape[1]), u.data_ptr() if jitter else None, N, S, int(lindisp), z1.data_ptr(),
                                               pts.data_ptr(), st), "dp")
    torch.cuda.synchronize()
    assert torch.equal(z0, z1)
    assert torch.equal(pts, rays[:, None, 0:3] + rays[:, None, 3:6] * z0[:, :, None])


@pytest.mark.gpu
def test_pooled_draws_feed_a_training_iteration_with_the_same_distributions():
    """training.POOLED_DRAWS: one torch.rand + one torch.randn call per iteration instead of the reference's six -- shapes, ranges and
    moments of what the kernels receive, the noise scaled by raw_noise_std, and a seeded iteration that is reproducible and differentiable
    (its numbers are NOT the reference's: another position in the generator's stream, which is why the switch is off by default)."""
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(N_importance=64)
    rays, latents = make_rays(512, 3, cfg)
    kw = dict(N_samples=64, N_importance=64, perturb=1.0, raw_noise_std=0.5)
    torch.manual_seed(3)
    rnd, e = training._pooled_draws(rays.to(DEV), kw, True)
    assert tuple(rnd["u_coarse"].shape) == (512, 64) and tuple(rnd["u_fine"].shape) == (512, 64)
    assert tuple(rnd["noise_coarse"].shape) == (512, 64) and tuple(rnd["noise_fine"].shape) == (512, 128) and tuple(e.shape) == (512 * 64, 3)
    for u in (rnd["u_coarse"], rnd["u_fine"]):
        assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 and abs(float(u.mean()) - 0.5) < 0.01
    for n_, std in ((rnd["noise_coarse"], 0.5), (rnd["noise_fine"], 0.5), (e, 1.0)):
        assert abs(float(n_.mean())) < 0.02 * std + 1e-3 and abs(float(n_.std()) - std) < 0.02 * std
    scene = make_scene(cfg, 1)
    target = torch.rand(512, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    R.set_precision("f32")
    old, training.POOLED_DRAWS = training.POOLED_DRAWS, True
    try:
        res = []
        for _ in range(2):
            rb, coarse, fine = _modules(scene)
            lat = latents.to(DEV).requires_grad_(True)
            kwr = dict(network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=64, N_importance=64, perturb=1.0, raw_noise_std=1.0)
            torch.manual_seed(11)
            loss, _ = training.training_loss(rays.to(DEV), lat, target, kwr, offsets_loss_weight=60.0, divergence_loss_weight=3.0,
                                             rigidity_loss_weight=5e-4, global_step=120000, N_iters=200000, mean=True)
            loss.backward()
            res.append((float(loss), lat.grad.clone(), rb.network[0].weight.grad.clone()))
    finally:
        training.POOLED_DRAWS = old
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert torch.isfinite(res[0][1]).all() and float(res[0][2].abs().max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays,n_codes,latent", [(1024, 8, 32), (777, 300, 32), (16384, 3, 64), (5, 4, 7)])
def test_code_gradients_kernel_vs_indexing_backward(n_rays, n_codes, latent):
    """nrnerf_code_gradients (training.select_codes' backward: the gradient of ``codes[index]``, train.py:173-188) against autograd's own
    indexing backward in float64; codes no ray selects get zeros; two calls give the same bits (rays are added in a fixed order)."""
    from nonrigid_nerf_amd import training
    g = torch.Generator().manual_seed(n_rays)
    codes = torch.randn(n_codes, latent, generator=g).to(DEV).requires_grad_(True)
    index = torch.randint(0, max(1, n_codes - 1), (n_rays,), generator=g).to(DEV)          # (the last code is never selected)
    up = torch.randn(n_rays, latent, generator=g).to(DEV)
    got = []
    for _ in range(2):
        codes.grad = None
        (training.select_codes(codes, index) * up).sum().backward()
        got.append(codes.grad.clone())
    assert torch.equal(got[0], got[1])
    ref = torch.zeros(n_codes, latent, dtype=torch.float64, device=DEV).index_add_(0, index, up.double())
    scale = float(ref.abs().max()) + 1e-20
    assert float((got[0].double() - ref).abs().max()) <= 2e-6 * scale
    if n_codes > 1:
        assert float(got[0][n_codes - 1].abs().max()) == 0.0


@pytest.mark.gpu
def test_training_loss_with_the_fused_loss_equals_the_eager_terms():
    """training.training_loss (the shipped recipe: data term + offsets / rigidity + divergence regularisers) with its loss terms on
    nrnerf_loss_* against the same call with eager torch ops (FUSED_LOSS = False): same random draws, same loss, same gradients."""
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(N_importance=64)
    scene = make_scene(cfg, 1)
    rays, latents = make_rays(257, 3, cfg)
    target = torch.rand(257, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    R.set_precision("f32")
    out = {}
    for fused in (False, True):
        rb, coarse, fine = _modules(scene)
        lat = latents.to(DEV).requires_grad_(True)
        kw = dict(network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=64, N_importance=64, perturb=1.0, raw_noise_std=1.0)
        old, training.FUSED_LOSS = training.FUSED_LOSS, fused
        try:
            torch.manual_seed(11)
            loss, _ = training.training_loss(rays.to(DEV), lat, target, kw, offsets_loss_weight=60.0, divergence_loss_weight=3.0,
                                             rigidity_loss_weight=5e-4, global_step=120000, N_iters=200000, mean=fused)
            (loss if fused else loss.mean()).backward()        # (the fused call: the mean from the loss kernel's own launch)
        finally:
            training.FUSED_LOSS = old
        grads = {k: p.grad.clone() for k, p in _named(rb, coarse, fine).items() if p.grad is not None}
        grads[("latents", "")] = lat.grad.clone()
        out[fused] = ((loss if fused else loss.mean()).detach().clone(), grads)
    assert torch.allclose(out[True][0], out[False][0], rtol=1e-5, atol=1e-7)
    assert set(out[True][1]) == set(out[False][1])
    for k, ge in out[False][1].items():
        gf = out[True][1][k]
        scale = float(ge.abs().max()) + 1e-20
        assert float((ge - gf).abs().max()) <= 1e-4 * scale, (k, float((ge - gf).abs().max()) / scale)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_kw", [dict(N_importance=64), dict(N_importance=64, netwidth=128), dict(N_importance=64, use_viewdirs=True)],
                         ids=["default", "narrow_128", "viewdirs_not_rehomed"])
def test_fused_adam_equals_torch_adam_and_leaves_the_packed_weights_fresh(cfg_kw):
    """training.FusedAdam (nrnerf_adam_step: Adam + the device-side weight re-pack in ONE launch; reference optimiser train.py:655-658):
    five steps on random gradients must leave the parameters where torch.optim.Adam leaves a copy of them (fp32, <= 1e-5 of the
    update + a few ulps), a host-side ``param_group["lr"]`` decay is honoured (train.py:1625-1630), the next render uses the stepped weights without
    another re-pack (equal, bit for bit, to a handle packed from scratch), the state round-trips through torch.optim.Adam's state_dict,
    and the modules' parameters / state_dict are ordinary tensors although they live in one flat vector."""
    import copy
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(**cfg_kw)
    scene = make_scene(cfg, 2)
    rb, coarse, fine = _modules(scene)
    rb2, coarse2, fine2 = copy.deepcopy(rb), copy.deepcopy(coarse), copy.deepcopy(fine)
    coarse2.ray_bender, fine2.ray_bender = (rb2,), (rb2,)
    codes = torch.zeros(4, cfg.latent_size, device=DEV, requires_grad=True)
    codes2 = codes.detach().clone().requires_grad_(True)
    named, named2 = _named(rb, coarse, fine), _named(rb2, coarse2, fine2)
    params, params2 = list(named.values()) + [codes], list(named2.values()) + [codes2]
    sd_before = {k: v.detach().clone() for k, v in coarse.state_dict().items()}
    opt = training.FusedAdam(params, lr=1e-2, betas=(0.9, 0.999), networks=(coarse, fine))
    ref = torch.optim.Adam(params2, lr=1e-2, betas=(0.9, 0.999))
    assert opt.repacks_weights == (not cfg.use_viewdirs)
    for k, v in coarse.state_dict().items():               # re-homing moved the storage, not the values
        assert torch.equal(v, sd_before[k]), k
    rays, lat = make_rays(64, 1, cfg)
    rays, lat = rays.to(DEV), lat.to(DEV)
    R.set_precision("bf16")
    kw = dict(N_samples=cfg.N_samples, N_importance=cfg.N_importance, network_fine=fine, additional_pixel_information={"ray_bending_latents": lat})

    def render():
        with torch.no_grad():
            return R.render_rays(rays, coarse, **kw)["rgb_map"].clone()

    before = render()
    g = torch.Generator().manual_seed(0)
    start = {k: p.detach().clone() for k, p in named.items()}
    for it in range(5):
        for (k, p), p2 in zip(list(named.items()) + [("codes", codes)], params2):
            gr = torch.randn(p.shape, generator=g).to(DEV) * (0.0 if (it == 2 and k == "codes") else 1.0)
            p.grad, p2.grad = gr.clone(), gr.clone()
        lr = 1e-2 * (0.5 ** it)
        for grp in opt.param_groups + ref.param_groups:
            grp["lr"] = lr
        opt.step()
        ref.step()
    worst = 0.0
    for (k, p), p2 in zip(list(named.items()) + [("codes", codes)], params2):
        moved = (p2.detach() - (start[k] if k != "codes" else 0.0)).abs().max().item()
        worst = max(worst, (p.detach() - p2.detach()).abs().max().item() / max(moved, 1e-12))
        assert (p.detach() - p2.detach()).abs().max().item() <= 1e-5 * max(moved, 1e-3) + 1e-7, k        # (a few fp32 ulps of the parameter after five steps)
    print(f"\\n[FusedAdam vs torch.optim.Adam, 5 steps] worst |difference| / |update| over all tensors: {worst:.2e}; "
          f"segments of the last launch: {opt.last_segments}")
    launches = []
    if opt.repacks_weights:
        model = R.get_model(coarse, fine)
        lib_update = model.update_from_device
        model.update_from_device = lambda *a, **k: (launches.append(1), lib_update(*a, **k))[1]
    after = render()
    assert not torch.equal(after, before), "the steps did not reach the packed weights"
    assert not launches, "the render after a fused step re-packed the weights again"
    R.invalidate(coarse)
    if cfg.use_viewdirs:        # (the device-side refresh folds feature_linear into the views layer with fp32 device products, the host packer on
        assert (render() - after).abs().max().item() < 2e-3           #  the host: two roundings of the folded matrix, as test_device_side_weight_refresh_* states)
    else:
        assert torch.equal(render(), after), "packed weights after the fused step differ from a fresh pack of the parameters"
    # state_dict round trip with torch's Adam (the reference checkpoints its optimiser, train.py:1680-1698)
    sd = opt.state_dict()
    ref.load_state_dict(copy.deepcopy(sd))
    opt2 = training.FusedAdam(params, lr=1e-2, networks=(coarse, fine))
    opt2.load_state_dict(copy.deepcopy(ref.state_dict()))
    for p in params:
        assert torch.equal(opt2.state[p]["exp_avg"], opt.state[p]["exp_avg"]) and torch.equal(opt2.state[p]["exp_avg_sq"], opt.state[p]["exp_avg_sq"])
    assert float(opt2.state[params[0]]["step"]) == 5.0
    assert all(isinstance(p, torch.nn.Parameter) for p in coarse.parameters())


@pytest.mark.gpu
def test_training_iteration_with_the_fused_optimiser_replayed_from_a_hip_graph():
    """GraphedStep + FusedAdam(networks=...): the captured iteration has NO re-pack at its start (the optimiser's launch leaves the handles
    fresh at its end), trains, and after any replay a no-grad render uses the trained weights without a sync() or another re-pack."""
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(N_importance=64)
    rb, coarse, fine = training._fresh_training_modules(cfg, torch.device(DEV), 64)
    params = []
    for m in (rb, coarse, fine):
        m.requires_grad_(True)
        params += list(m.parameters())
    codes = torch.zeros(4, cfg.latent_size, device=DEV, requires_grad=True)
    opt = training.FusedAdam(params + [codes], lr=5e-4, networks=(coarse, fine))
    rays, _ = make_rays(256, 5, cfg)
    rays = rays.to(DEV)
    frame = torch.randint(0, 4, (256,), device=DEV)
    target = 0.5 + 0.4 * torch.sin(3.0 * rays[:, 3:6])
    kw = dict(network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=64, N_importance=64, perturb=1.0, raw_noise_std=1.0)
    R.set_precision("bf16")

    def loss_of(rays, target, frame, global_step):
        loss, _ = training.training_loss(rays, training.select_codes(codes, frame), target, kw, offsets_loss_weight=60.0, divergence_loss_weight=3.0,
                                         rigidity_loss_weight=0.0005, global_step=global_step, N_iters=200000, chunk=32768)
        return loss.mean()

    gstep = torch.zeros((), device=DEV)
    graphed = training.GraphedStep(loss_of, dict(rays=rays, target=target, frame=frame, global_step=gstep), opt, [coarse])
    assert graphed.repacks
    losses = [float(graphed(global_step=gstep.fill_(float(i)))) for i in range(60)]
    assert all(l == l for l in losses)
    assert sum(losses[-10:]) / 10 < 0.8 * sum(losses[:5]) / 5, (losses[:5], losses[-10:])
    with torch.no_grad():
        got = R.batchify_rays(rays, {"ray_bending_latents": codes[frame].detach()}, chunk=32768, **{**kw, "perturb": 0.0, "raw_noise_std": 0.0})
        R.invalidate(coarse)
        want = R.batchify_rays(rays, {"ray_bending_latents": codes[frame].detach()}, chunk=32768, **{**kw, "perturb": 0.0, "raw_noise_std": 0.0})
    assert torch.equal(got["rgb_map"], want["rgb_map"]), "after a replay the packed weights must be the trained parameters"
    print(f"\\n[graphed training step, fused optimiser] loss {losses[0]:.4f} -> {losses[-1]:.4f} over 60 replays")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,wo,wi,wi2", [(4097, 192, 192, 51), (1000, 100, 320, 27), (70000, 448, 256, 63), (129, 4, 128, 8), (64, 130, 36, 3)])
def test_tn_products_kernel_vs_einsum(dtype, M, wo, wi, wi2):
    """nrnerf_tn_products (csrc/nrnerf_gen_train.hip: the weight / bias gradients of a non-compiled trunk over its ROW-MAJOR saved arrays;
    bf16 through LDS transpose reads, fp32 on 16x16x4 MFMAs) against torch: a product with a bias row, a second product of the same `a`
    written into the neighbouring columns of the same matrix (the skip layer's [encoding | activation] weight), a sub-matrix operand
    (column offset + leading dimension, as the view-dependent head's halves), widths that are no multiple of the 128-wide panels or of
    a 16-byte piece (100 bf16 columns: the element-wise edge path), row counts that are no multiple of the 64-sample tile."""
    from nonrigid_nerf_amd import training
    g = torch.Generator().manual_seed(3)
    a = (torch.randn(M, wo + 6, generator=g) * 0.5).to(DEV).to(dtype)
    b = torch.randn(M, wi, generator=g).to(DEV).to(dtype)
    b2 = torch.randn(M, wi2, generator=g).to(DEV).to(dtype)
    ldo = wi + wi2
    o_w, o_b, o_s = 7, 7 + wo * ldo, 7 + wo * ldo + wo + 5
    total = o_s + (wo - 2) * wi + 3
    jobs = [(a, 0, b, 0, wo, wi, ldo, o_w, o_b), (a, 0, b2, 0, wo, wi2, ldo, o_w + wi, None),
            (a, 2, b, 0, wo - 2, wi, wi, o_s, None)]                      # columns 2.. of a: a sub-matrix operand
    got = training._tn_products(jobs, M, total, torch.device(DEV))
    torch.cuda.synchronize()
    af, bf, b2f = a.double(), b.double(), b2.double()
    want_w = torch.cat([af[:, :wo].T @ bf, af[:, :wo].T @ b2f], 1)
    want_s = af[:, 2:wo].T @ bf
    scale = float(want_w.abs().max())
    tol = (2e-3 if dtype == torch.bfloat16 else 2e-5) * scale      # (fp32 accumulation of M products; the operands are exact in both modes)
    assert (got[o_w:o_w + wo * ldo].view(wo, ldo).double() - want_w).abs().max().item() <= tol
    assert (got[o_b:o_b + wo].double() - af[:, :wo].sum(0)).abs().max().item() <= tol
    assert (got[o_s:o_s + (wo - 2) * wi].view(wo - 2, wi).double() - want_s).abs().max().item() <= tol
    covered = torch.zeros(total, dtype=torch.bool)
    covered[o_w:o_w + wo * ldo] = True
    covered[o_b:o_b + wo] = True
    covered[o_s:o_s + (wo - 2) * wi] = True
    assert bool((got.cpu()[~covered] == 0).all()), "positions no job covers must be zero"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("L,stride,n_lat", [(10, 4, 0), (4, 3, 0), (8, 4, 16), (0, 3, 0)])
def test_encoding_rows_kernels_vs_torch_autograd(dtype, L, stride, n_lat):
    """nrnerf_encoding_forward / _backward (Embedder.embed of 3-vectors as rows, rnh:120-150, and its transposed Jacobian; with the
    time-conditioned baseline's code columns appended) against torch ops under autograd."""
    from nonrigid_nerf_amd import training
    g = torch.Generator().manual_seed(5)
    N, S = 37, 19
    M = N * S
    src = (torch.randn(M, stride, generator=g) * 0.7).to(DEV)
    codes = torch.randn(N, n_lat, generator=g).to(DEV) if n_lat else None
    n_enc = 3 + 6 * L
    cols = training._pad8(n_enc + n_lat)
    enc = training._encoding_rows(src, stride, L, M, cols, dtype, codes, S)
    p = src[:, :3].detach().clone().requires_grad_(True)
    want = training.posenc(p, L)
    tol = 2e-6 if dtype == torch.float32 else 8e-3
    assert (enc[:, :n_enc].float() - want.detach()).abs().max().item() <= tol
    if n_lat:
        assert torch.equal(enc[:, n_enc:n_enc + n_lat].float(), codes.to(dtype).float()[:, None, :].expand(N, S, n_lat).reshape(M, n_lat))
    assert bool((enc[:, n_enc + n_lat:] == 0).all())
    d0 = torch.randn(M, n_enc + n_lat, generator=g).to(DEV)
    d1 = torch.randn(M, n_enc + n_lat, generator=g).to(DEV)
    for second in (None, d1):
        got = training._encoding_backward(src, stride, L, d0, second, n_enc + n_lat, M)
        gsum = d0 if second is None else d0 + d1
        ref, = torch.autograd.grad(want, p, gsum[:, :n_enc], retain_graph=True)
        scale = float(ref.abs().max())
        assert (got[:, :3] - ref).abs().max().item() <= 1e-5 * scale and bool((got[:, 3] == 0).all())


def _refresh_cases():
    shapes = [("default", dict(N_importance=64)), ("narrow_128", dict(N_importance=64, netwidth=128)), ("viewdirs", dict(N_importance=64, use_viewdirs=True)),
              ("generic_192", dict(N_importance=64, netwidth=192, netdepth=6))]
    # (view-dependent head on the device route: the refreshed views layer -- feature_linear folded in by an fp32 device GEMM -- differs from
    #  the host packer's by an ulp, test_device_side_weight_refresh_equals_a_fresh_pack; the host route covers that shape's images bit for bit)
    return [pytest.param(kw, route, id=f"{name}-{route}") for name, kw in shapes for route in ("host", "device")
            if not (kw.get("use_viewdirs") and route == "device")]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_kw,route", _refresh_cases())
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_a_refreshed_handle_trains_like_a_fresh_one(precision, cfg_kw, route):
    """The TRAINING images of a handle (transposed trunk weights, bender-less forward images of the view-dependent head, the bender's fp32
    forward / backward images; off the compiled set the backward programs and the width-class trunks with theirs) follow a weight refresh
    like the render images do: after an in-place change of every parameter, one training_loss(...).backward() on the cached handle --
    refreshed by ``nrnerf_model_update`` (host) or ``nrnerf_model_update_device`` (device) -- gives the loss and every parameter / latent
    gradient of the same iteration on copies of the modules, i.e. on a freshly created handle.  Bit for bit: the comparison two fresh handles
    pass against each other (asserted here too, as the yardstick; run-to-run results are deterministic, profiles/r06_soak_determinism.txt)."""
    import copy
    from nonrigid_nerf_amd import training
    cfg = SceneConfig(**cfg_kw)
    scene = make_scene(cfg, 1)
    rays, latents = make_rays(96, 3, cfg)
    rays = rays.to(DEV)
    target = torch.rand(96, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    R.set_precision(precision)
    w = dict(offsets_loss_weight=60.0, divergence_loss_weight=3.0, rigidity_loss_weight=5e-4, global_step=120000, N_iters=200000)

    def iteration(mods):
        rb, coarse, fine = mods
        for p_ in _named(rb, coarse, fine).values():
            p_.grad = None
        lat = latents.to(DEV).requires_grad_(True)
        kw = dict(network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=64, N_importance=64, perturb=1.0, raw_noise_std=1.0)
        torch.manual_seed(11)
        loss, _ = training.training_loss(rays, lat, target, kw, **w)
        loss.mean().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in _named(rb, coarse, fine).items() if p.grad is not None}
        grads[("latents", "")] = lat.grad.clone()
        return loss.detach().clone(), grads

    def clone(mods):
        rb2, coarse2, fine2 = copy.deepcopy(mods[0]), copy.deepcopy(mods[1]), copy.deepcopy(mods[2])
        coarse2.ray_bender, fine2.ray_bender = (rb2,), (rb2,)
        return rb2, coarse2, fine2

    mods = _modules(scene)
    iteration(mods)                                   # creates and caches the handle, old weights
    with torch.no_grad():
        for p_ in _named(*mods).values():
            p_.mul_(1.03).add_(0.001)
    used = {"device": 0, "host": 0, "created": 0}
    orig_dev, orig_host, orig_init = R.Model.update_from_device, R.Model.update, R.Model.__init__

    def dev_route(self, *a, **k):
        if route == "host":
            return False
        ok = orig_dev(self, *a, **k)
        used["device"] += int(ok)
        return ok

    def host_route(self, *a, **k):
        ok = orig_host(self, *a, **k)
        used["host"] += int(ok)
        return ok

    def init(self, *a, **k):
        used["created"] += 1
        return orig_init(self, *a, **k)

    R.Model.update_from_device, R.Model.update, R.Model.__init__ = dev_route, host_route, init
    try:
        loss_r, g_r = iteration(mods)
    finally:
        R.Model.update_from_device, R.Model.update, R.Model.__init__ = orig_dev, orig_host, orig_init
    assert used["created"] == 0 and used[route] >= 1 and used["host" if route == "device" else "device"] == 0, used
    loss_a, g_a = iteration(clone(mods))              # fresh handles (new modules: new cache entries), the changed weights
    loss_b, g_b = iteration(clone(mods))
    assert torch.equal(loss_a, loss_b) and set(g_a) == set(g_b) and all(torch.equal(g_a[k], g_b[k]) for k in g_a), "two fresh handles disagree"
    assert torch.equal(loss_r, loss_a)
    assert set(g_r) == set(g_a)
    for k in g_a:
        assert torch.equal(g_r[k], g_a[k]), (k, float((g_r[k] - g_a[k]).abs().max()))
