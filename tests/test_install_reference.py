"""`install()` on the REAL reference module (build container only: /root/reference does not exist on the GPU box, so
this file is skipped there).  Without a GPU every call is ineligible ("rays are not on a ROCm device") and must be
handed to the reference's own functions saved by install(): the rebinding of the module globals
(train.py:125, 402), the keyword forwarding and the restore are what is checked, against the committed reference
outputs."""
import os
import sys
import types

import pytest
import torch

REF = os.environ.get("NRNERF_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def reference():
    if not os.path.isfile(os.path.join(REF, "train.py")):
        pytest.skip("reference checkout not present")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import make_golden as G
    old_get_device = torch.Tensor.get_device
    H, T = G.import_reference()
    yield G, H, T
    torch.Tensor.get_device = old_get_device
    for m in ("train", "run_nerf_helpers"):
        sys.modules.pop(m, None)
    sys.path.remove(REF)


def test_install_rebinds_the_reference_module_and_falls_back_without_a_gpu(reference):
    from nonrigid_nerf_amd import render as R
    from tests.helpers import load_golden, compare_dict
    G, H, T = reference
    meta, cfg, scene, rays, latents, ref = load_golden("ragged_chunks")          # 37 rays in chunks of 16
    kw, rb, coarse, fine = G.reference_kwargs(H, T, scene)
    orig_rr, orig_br = T.render_rays, T.batchify_rays
    calls = {"rr": 0}

    def counting_render_rays(*a, **k):
        calls["rr"] += 1
        return orig_rr(*a, **k)

    T.render_rays = counting_render_rays                    # what install() must save and defer to
    undo = R.install(T, precision="f32")
    try:
        assert T.render_rays is R.render_rays and T.batchify_rays is R.batchify_rays
        with torch.no_grad():
            rgb, disp, acc, extras = T.render(rays[:, 0:3], rays[:, 3:6], chunk=meta["chunk"],
                                              additional_pixel_information={"ray_bending_latents": latents}, **kw)
        assert calls["rr"] >= 1, "the saved reference render_rays was never reached"
        out = {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, **extras}
        assert set(out) == set(ref)
        assert not compare_dict(out, ref, tol_scale=0.02)
    finally:
        undo()
        assert T.render_rays is counting_render_rays and T.batchify_rays is orig_br
        T.render_rays = orig_rr


def test_without_install_an_ineligible_call_fails_loudly():
    """No reference function saved -> no silent CPU path: the boundary raises."""
    from nonrigid_nerf_amd import render as R
    from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_rays, make_scene
    cfg = SceneConfig(N_importance=0)
    rb, coarse, fine = build_modules(make_scene(cfg, 0))
    rays, lat = make_rays(4, 0, cfg)
    with torch.no_grad(), pytest.raises(R.Unsupported):
        R.render_rays(rays, coarse, N_samples=cfg.N_samples, additional_pixel_information={"ray_bending_latents": lat})


@pytest.mark.gpu
def test_real_reference_modules_render_through_the_hip_path_on_a_gpu(reference):
    """The route a user of the reference takes on a GPU box: the reference's own ``NeRF`` / ``ray_bending`` modules on
    the device, ``install(train)``, then the reference's ``train.render`` (what free_viewpoint_rendering.py:202-337 calls
    through ``render_path``), with the editing knobs mutated between calls (fvr:264-283).  The HIP path must take every
    call (the saved reference ``render_rays`` is never reached) and reproduce the committed reference outputs.

    Needs a reference checkout on the GPU box: set NRNERF_REFERENCE=/path/to/nonrigid_nerf (the driver's GPU boxes have
    none, so there this test is skipped and the route is covered with the attribute-compatible holders of
    nonrigid_nerf_amd/modules.py only)."""
    from nonrigid_nerf_amd import render as R
    from tests.helpers import load_golden, compare_dict, split_knobs
    G, H, T = reference
    dev = torch.device("cuda:0")
    T.device = dev
    # (the last two: architectures outside the compiled set -- the reference's own NeRF(D=6, W=192) / NeRF(D=10, W=320) etc. land on
    #  the run-time-parameterised kernel, csrc/nrnerf_generic.h, instead of falling back)
    for name in ("headline_64_128", "knobs_64_64", "generic_192_320_detailed", "generic_viewdirs_96_160"):
        meta, cfg, scene, rays, latents, ref = load_golden(name)
        knobs, flags = split_knobs(meta["knobs"])
        kw, rb, coarse, fine = G.reference_kwargs(H, T, scene)
        for m in (rb, coarse, fine):
            if m is not None:
                m.to(dev)
        orig_rr = T.render_rays
        reached = []
        T.render_rays = lambda *a, **k: (reached.append(1), orig_rr(*a, **k))[1]
        undo = R.install(T, precision="f32")
        try:
            rb.rigidity_test_time_cutoff = knobs.get("rigidity_test_time_cutoff")          # fvr:264-283
            rb.test_time_scaling = knobs.get("test_time_scaling")
            for m in (coarse, fine):
                m.test_time_nonrigid_object_removal_threshold = knobs.get("removal_threshold")
            kw.update(flags)
            with torch.no_grad():
                rgb, disp, acc, extras = T.render(rays[:, 0:3].to(dev), rays[:, 3:6].to(dev), chunk=meta["chunk"],
                                                  additional_pixel_information={"ray_bending_latents": latents.to(dev)},
                                                  detailed_output=bool(meta["detailed"]), retraw=bool(meta["retraw"]), **kw)
            assert not reached, "the call fell back to the reference's render_rays instead of the HIP path"
            out = {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, **extras}
            assert set(out) == set(ref) and all(v.is_cuda for v in out.values())
            coarse_keys = [k for k in ("rgb0", "disp0", "acc0", "visibility_weights", "input_pts", "rigidity_mask") if k in ref]
            fails = compare_dict(out, ref, keys=coarse_keys)
            fails += compare_dict(out, ref, keys=["rgb_map", "acc_map"], frac_ok=0.10, outlier_atol=2e-2)
            assert not fails, "\n".join(fails)
        finally:
            undo()
            T.render_rays = orig_rr


def _to_device(H, T, G, scene, dev):
    kw, rb, coarse, fine = G.reference_kwargs(H, T, scene)
    for m in (rb, coarse, fine):
        if m is not None:
            m.to(dev)
    return kw, rb, coarse, fine


class _Spy:
    """Counts the calls that reach a saved reference function (what install() keeps as the fallback)."""

    def __init__(self, module, name):
        self.module, self.name, self.orig, self.calls = module, name, getattr(module, name), 0
        setattr(module, name, self)

    def __call__(self, *a, **k):
        self.calls += 1
        return self.orig(*a, **k)

    def restore(self):
        setattr(self.module, self.name, self.orig)


@pytest.mark.gpu
def test_reference_render_path_and_dataparallel_wrapper_run_on_the_hip_path(reference):
    """(a) the reference's own frame driver ``train.render_path`` (train.py:419-553) with ``detailed_output=True`` -- what
    free_viewpoint_rendering.py runs by default -- and (b) the reference's ``render_wrapper_class`` under
    ``nn.DataParallel`` (``get_parallelized_render_function``, train.py:300-323: the bender tuple is re-attached inside
    ``forward``), both after ``install(train)`` with the reference's REAL modules on the GPU.  Every render call must be
    taken by the HIP path (the saved reference ``render_rays`` is never reached) and reproduce the committed outputs of
    the reference (tests/golden/render_path_2frames.npz)."""
    import numpy as np
    from nonrigid_nerf_amd import render as R
    from nonrigid_nerf_amd.synthetic import SceneConfig, make_scene
    from tests.helpers import GOLDEN_DIR, synthetic_camera
    G, H, T = reference
    dev = torch.device("cuda:0")
    T.device = dev
    z = np.load(os.path.join(GOLDEN_DIR, "render_path_2frames.npz"))
    scene = make_scene(SceneConfig(N_importance=64), 0)
    kw, rb, coarse, fine = _to_device(H, T, G, scene, dev)
    cams = [synthetic_camera(k, H=8, W=12) for k in range(2)]
    poses, intrins = [c.to(dev) for c, _ in cams], [i for _, i in cams]
    codes = torch.from_numpy(z["in__codes"]).to(dev)
    spy = _Spy(T, "render_rays")
    undo = R.install(T)                                    # no precision given: the drop-in must stay fp32
    try:
        assert R.get_precision() == "f32"
        with torch.no_grad():
            rgbs, disps, details = T.render_path(poses, intrins, 32768, kw, codes, detailed_output=True)
            par = T.get_parallelized_render_function(coarse_model=coarse, fine_model=fine, ray_bender=rb)
            kw_par = {k: v for k, v in kw.items() if k not in ("network_fn", "network_fine", "ray_bender")}
            rgbs2, disps2 = T.render_path(poses, intrins, 32768, kw_par, codes, detailed_output=False, parallelized_render_function=par)      # train.py:550-553
        assert spy.calls == 0, "a call fell back to the reference's render_rays instead of the HIP path"
    finally:
        undo()
        spy.restore()
    for got_rgb, got_disp in ((rgbs, disps), (rgbs2, disps2)):
        # fine-pass maps: a few rays take the other `denom < 1e-5` branch of sample_pdf, so: most pixels
        # at the fp32 tolerance, the rest bounded -- the bars of the golden render tests (tests/test_gpu_parity.py)
        err = np.abs(np.asarray(got_rgb) - z["out__rgbs"]).max(-1)
        assert (err <= 1e-4).mean() >= 0.90 and err.max() <= 2e-2, ((err <= 1e-4).mean(), err.max())
        d, dr = np.asarray(got_disp), z["out__disps"]
        assert ((np.isnan(d) & np.isnan(dr)) | (np.abs(d - dr) <= 1e-4 + 1e-3 * np.abs(dr))).mean() >= 0.90
    assert np.array_equal(np.asarray(rgbs), np.asarray(rgbs2)), "the DataParallel wrapper route renders different pixels than the plain route"
    assert len(details) == 2
    per_pass = ("visibility_weights", "opacity_alpha", "initial_input_pts", "unmasked_offsets", "masked_offsets", "input_pts", "rigidity_mask")
    assert set(details[0]) == {"rgb0", "disp0", "acc0", "z_std"} | set(per_pass) | {"fine_" + k for k in per_pass}      # train.py:955-972
    for k in ("fine_visibility_weights", "fine_input_pts", "fine_rigidity_mask"):
        want = z["out__" + k + "_0"]
        got = details[0][k].reshape(want.shape)
        close = np.isclose(got, want, atol=2e-4, rtol=1e-3)
        assert close.mean() >= 0.97, (k, close.mean())               # a few rays take the other sample_pdf branch


@pytest.mark.gpu
@pytest.mark.parametrize("views,width", [(False, 256), (True, 256), ("exact", 256), (False, 192), (True, 192)],
                         ids=["default", "use_viewdirs", "use_viewdirs_exact", "generic_w192", "generic_w192_use_viewdirs"])
def test_reference_training_iteration_runs_natively_after_install(reference, capsys, views, width):
    """(c) one iteration of the reference's ``training_wrapper_class.forward`` + ``backward`` (train.py:152-287, 1594-1597)
    with the shipped loss weights (configs/example_sequence.txt: offsets 60, divergence 3, rigidity 5e-4, 64 + 64 samples,
    perturb, raw noise 1), on the reference's REAL modules on the GPU: once eagerly (the unmodified reference on this
    device) and once after ``install(train, precision="f32")``.  After install no call may reach the reference's
    ``render_rays`` or ``compute_divergence_loss`` -- the whole iteration, second-order term included, is native -- and
    with the same seed the loss and every parameter gradient must agree with the eager run.  ``use_viewdirs``: the reference's
    view-dependent head (rnh:284-304) with finite-difference directions -- both of its branches run inside the training
    kernels (csrc/nrnerf_train.h, VIEWS), so this is the reference's own autograd through alpha / feature / views / rgb layers
    against theirs.  ``exact``: exact_nonrigid_viewdirs (rnh:358-385) -- the reference differentiates THROUGH the bender's Jacobian
    (three reverse passes with create_graph=True); here one forward-mode tangent and the divergence kernels' two-chain backward.
    ``width`` 192 (round 5): an architecture outside the compiled set -- render_rays trains on the run-time-parameterised kernel
    (training._GenericTrunk, bender as torch ops); only the divergence regulariser, whose native form needs the bender's compiled training
    kernels, is the reference's own function there."""
    import argparse
    from nonrigid_nerf_amd import render as R
    G, H, T = reference
    dev = torch.device("cuda:0")
    T.device = dev
    ts = G.TRAIN_STEP
    n_rays = 1024                                             # N_rand of the shipped config
    from nonrigid_nerf_amd.synthetic import SceneConfig, make_rays, make_scene
    cfg = SceneConfig(N_importance=ts["N_importance"], use_viewdirs=bool(views), approx_nonrigid_viewdirs=(views != "exact"), netwidth=width)
    scene = make_scene(cfg, ts["seed"])
    rays, _ = make_rays(n_rays, ts["seed"], cfg)
    g = torch.Generator().manual_seed(11)
    codes0 = torch.randn(ts["n_frames"], cfg.latent_size, generator=g) * 0.1
    image_ids = torch.randint(0, ts["n_frames"], (n_rays,), generator=g)
    target = torch.rand(n_rays, 3, generator=g).to(dev)
    args = argparse.Namespace(offsets_loss_weight=ts["offsets_loss_weight"], divergence_loss_weight=ts["divergence_loss_weight"],
                              rigidity_loss_weight=ts["rigidity_loss_weight"], chunk=ts["chunk"], N_iters=ts["N_iters"],
                              N_samples=ts["N_samples"], ray_bending_latent_size=cfg.latent_size)
    bpi = torch.stack([image_ids, torch.zeros_like(image_ids), torch.zeros_like(image_ids)], 1)

    def one_step(installed):
        kw, rb, coarse, fine = _to_device(H, T, G, scene, dev)
        kw.update(perturb=ts["perturb"], raw_noise_std=ts["raw_noise_std"])
        codes = [c.clone().to(dev).requires_grad_(True) for c in codes0]
        wrapper = T.training_wrapper_class(coarse, codes, fine_model=fine, ray_bender=rb)
        spies, undo = [], None
        if installed:
            spies = [_Spy(T, "render_rays"), _Spy(T, "compute_divergence_loss")]
            undo = R.install(T, precision="f32")
            assert T.compute_divergence_loss is not spies[1]
        try:
            torch.manual_seed(ts["render_seed"])
            loss = wrapper(args, rays[:, 0:3].to(dev), rays[:, 3:6].to(dev), 100, dict(kw), target, ts["global_step"], 0,
                           {"imageid_to_timestepid": list(range(ts["n_frames"]))}, bpi)
            loss.mean().backward()
            torch.cuda.synchronize()
            reached = [s.calls for s in spies]
        finally:
            if undo is not None:
                undo()
            for s in spies:
                s.restore()
        grads = {("codes", str(i)): c.grad for i, c in enumerate(codes)}
        for part, mod in (("bender", rb), ("coarse", coarse), ("fine", fine)):
            grads.update({(part, k): p.grad for k, p in mod.named_parameters() if p.grad is not None})
        return loss.detach(), grads, reached

    l_ref, g_ref, _ = one_step(False)
    l_hip, g_hip, reached = one_step(True)
    if width == 256:
        assert reached == [0, 0], f"calls that reached the reference's render_rays / compute_divergence_loss: {reached}"
    else:
        assert reached[0] == 0, f"calls that reached the reference's render_rays: {reached[0]}"
    assert set(g_hip) == set(g_ref), set(g_hip) ^ set(g_ref)
    # a few rays take the other `denom < 1e-5` branch of sample_pdf: per-ray loss with outliers, mean tight
    rel = (l_hip - l_ref).abs() / (l_ref.abs() + 1e-6)
    assert float((rel < 1e-3).float().mean()) >= 0.9, float((rel < 1e-3).float().mean())
    assert abs(float(l_hip.mean()) - float(l_ref.mean())) <= 2e-3 * abs(float(l_ref.mean()))
    rows = []
    for k, gr in g_ref.items():
        gh = g_hip[k]
        cos = float((gh * gr).sum() / (gh.norm() * gr.norm() + 1e-30))
        err = float((gh - gr).abs().max() / (gr.abs().max() + 1e-30))
        rows.append((err, cos, k))
        assert cos >= 0.99, (k, cos, err)
    rows.sort(reverse=True)
    with capsys.disabled():
        print(f"\n[reference training iteration, {n_rays} rays, real modules, width {width}{(', use_viewdirs, exact Jacobian directions' if views == 'exact' else ', use_viewdirs') if views else ''}] mean loss eager {float(l_ref.mean()):.6f} vs installed "
              f"{float(l_hip.mean()):.6f}; per-ray loss within 1e-3: {float((rel < 1e-3).float().mean()):.3f}; calls reaching the reference's "
              f"render_rays / compute_divergence_loss after install: {reached}; {len(rows)} gradient tensors, min cosine "
              f"{min(c for _, c, _ in rows):.5f}; largest max-error / scale: " + "; ".join(f"{k[0]}.{k[1]} {e:.1e} (cos {c:.5f})" for e, c, k in rows[:6]))


@pytest.mark.gpu
@pytest.mark.parametrize("views", [False, True], ids=["default", "use_viewdirs"])
def test_reference_training_loop_is_faster_after_install(reference, capsys, views):
    """What a user of the reference gains by the two-line drop-in, measured on the reference's REAL modules and its own
    ``training_wrapper_class`` (train.py:152-287) with the shipped recipe, N_rand = 1024: forward + backward + Adam step
    (train.py:1594-1610), eagerly on this device (the unmodified reference) and after ``install()`` in "f32" (the default:
    exact) and "bf16" mode.  Asserts only that the drop-in is not slower; the numbers go to profiles/."""
    import argparse
    import time
    from nonrigid_nerf_amd import render as R
    G, H, T = reference
    dev = torch.device("cuda:0")
    T.device = dev
    ts = G.TRAIN_STEP
    n_rays = 1024
    from nonrigid_nerf_amd.synthetic import SceneConfig, make_rays, make_scene
    cfg = SceneConfig(N_importance=ts["N_importance"], use_viewdirs=views)
    scene = make_scene(cfg, ts["seed"])
    rays, _ = make_rays(n_rays, ts["seed"], cfg)
    g = torch.Generator().manual_seed(11)
    codes0 = torch.randn(ts["n_frames"], cfg.latent_size, generator=g) * 0.1
    image_ids = torch.randint(0, ts["n_frames"], (n_rays,), generator=g)
    target = torch.rand(n_rays, 3, generator=g).to(dev)
    args = argparse.Namespace(offsets_loss_weight=ts["offsets_loss_weight"], divergence_loss_weight=ts["divergence_loss_weight"],
                              rigidity_loss_weight=ts["rigidity_loss_weight"], chunk=ts["chunk"], N_iters=ts["N_iters"],
                              N_samples=ts["N_samples"], ray_bending_latent_size=cfg.latent_size)
    bpi = torch.stack([image_ids, torch.zeros_like(image_ids), torch.zeros_like(image_ids)], 1)
    ro, rd = rays[:, 0:3].to(dev), rays[:, 3:6].to(dev)

    def ms_per_iteration(precision, iters):
        kw, rb, coarse, fine = _to_device(H, T, G, scene, dev)
        kw.update(perturb=ts["perturb"], raw_noise_std=ts["raw_noise_std"])
        codes = [c.clone().to(dev).requires_grad_(True) for c in codes0]
        wrapper = T.training_wrapper_class(coarse, codes, fine_model=fine, ray_bender=rb)
        params = list(coarse.parameters()) + list(fine.parameters()) + list(rb.parameters()) + codes
        opt = torch.optim.Adam(params, lr=5e-4, betas=(0.9, 0.999))                    # train.py:655-658
        undo = R.install(T, precision=precision) if precision else None
        try:
            def it(i):
                opt.zero_grad()
                loss = wrapper(args, ro, rd, 100, dict(kw), target, ts["global_step"] + i, 0,
                               {"imageid_to_timestepid": list(range(ts["n_frames"]))}, bpi)
                loss.mean().backward()
                opt.step()
            for i in range(3):
                it(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(iters):
                it(3 + i)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e3
        finally:
            if undo is not None:
                undo()

    eager = ms_per_iteration(None, 10)
    f32 = ms_per_iteration("f32", 30)
    bf16 = ms_per_iteration("bf16", 30)
    with capsys.disabled():
        print(f"\n[reference training loop, {n_rays} rays, real modules{', use_viewdirs' if views else ''}, shipped recipe, forward + backward + Adam] unmodified reference on this "
              f"GPU (eager PyTorch-ROCm): {eager:.1f} ms / iteration; after install(): f32 {f32:.2f} ms ({eager / f32:.1f} x), "
              f"bf16 {bf16:.2f} ms ({eager / bf16:.1f} x)")
    assert f32 < eager and bf16 < eager


def test_install_rebinds_compute_divergence_loss_and_falls_back_without_a_gpu(reference):
    """install() also rebinds ``train.compute_divergence_loss`` (star-imported from run_nerf_helpers, called at
    train.py:266).  On CPU tensors the native kernels cannot take the call: it must reach the saved reference function with
    every argument intact and return the reference's result (same seed, same probes)."""
    from nonrigid_nerf_amd import render as R
    from nonrigid_nerf_amd.synthetic import SceneConfig, make_scene
    G, H, T = reference
    scene = make_scene(SceneConfig(N_importance=64), 0)
    kw, rb, coarse, fine = G.reference_kwargs(H, T, scene)
    g = torch.Generator().manual_seed(3)
    n_rays, S = 5, 7
    pts = (torch.rand(n_rays * S, 3, generator=g) - 0.5)
    lat = (torch.randn(n_rays, 32, generator=g) * 0.1).view(n_rays, 1, -1).expand(n_rays, S, 32).reshape(-1, 32)
    w = torch.rand(n_rays * S, generator=g)
    orig = T.compute_divergence_loss
    torch.manual_seed(11)
    want = orig(None, pts.clone(), lat, rb, False, 16, n_rays, weights=w, backprop_into_weights=False)
    undo = R.install(T)
    try:
        assert T.compute_divergence_loss is not orig
        torch.manual_seed(11)
        got = T.compute_divergence_loss(None, pts.clone(), lat, rb, False, 16, n_rays, weights=w, backprop_into_weights=False)
    finally:
        undo()
    assert T.compute_divergence_loss is orig
    assert got.shape == (n_rays,) and torch.equal(got, want)
