"""Generate tests/golden/query/query_points.npz: the UNMODIFIED reference's own ``network_query_fn`` (create_nerf, train.py:633-649 ->
run_network, train.py:57-105) with ``detailed_output=True`` on seeded NON-COLLINEAR points -- every other golden evaluates the
networks on points that lie along camera rays.

Runs on the CPU, where the reference lives (``NRNERF_REFERENCE``, as oracle/make_golden.py, whose import recipe and module
construction are reused by import):   python tools/make_query_golden.py

The fixture lives in a directory of its own: tests/helpers.py takes every ``tests/golden/*.npz`` it does not list by name for a
render_rays case.  The file holds tensors only: per case ``<case>__points [6, 7, 3]``, ``<case>__latents [6, latent_size]``, ``<case>__viewdirs [6, 3]``
and ``<case>__out__<key>`` for ``raw`` and every detail key the reference returns.  The weights are a pure function of the seed
(nonrigid_nerf_amd.synthetic.make_scene), the configurations are CASES below (tests/test_query_host.py imports them).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_ROWS, N_SAMPLES, SEED = 6, 7, 0
CASES = {
    # name: (SceneConfig kwargs, knobs); N_samples = the row length (the reference's finite-difference directions reshape by num_ray_samples)
    "default_knobs": (dict(N_samples=N_SAMPLES, N_importance=0), dict(rigidity_test_time_cutoff=0.45, test_time_scaling=0.5, removal_threshold=0.6)),
    "deep_bender_viewdirs": (dict(N_samples=N_SAMPLES, N_importance=0, use_viewdirs=True, bend_depth=7), {}),
    "viewdirs_no_bender": (dict(N_samples=N_SAMPLES, N_importance=0, use_viewdirs=True, ray_bending=False), {}),
    "time_conditioned": (dict(N_samples=N_SAMPLES, N_importance=0, ray_bending=False, time_conditioned_baseline=True), {}),
}


def case_inputs(name, cfg):
    """Seeded, non-collinear points inside the scene's depth range, per-row latent codes and unit directions (CPU generator)."""
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    pts = (torch.rand(N_ROWS, N_SAMPLES, 3, generator=g) * 2.0 - 1.0) * 0.8
    lat = torch.randn(N_ROWS, cfg.latent_size, generator=g) * 0.5
    d = torch.randn(N_ROWS, 3, generator=g)
    return pts, lat, d / d.norm(dim=-1, keepdim=True)


def main(out_path=None):
    from oracle import make_golden as MG
    from nonrigid_nerf_amd.synthetic import SceneConfig, make_scene
    H, T = MG.import_reference()
    arrays = {}
    for name, (cfg_kw, knobs) in CASES.items():
        cfg = SceneConfig(**cfg_kw)
        scene = make_scene(cfg, SEED)
        kw, rb, coarse, _ = MG.reference_kwargs(H, T, scene)
        if rb is not None:
            rb.rigidity_test_time_cutoff = knobs.get("rigidity_test_time_cutoff")
            rb.test_time_scaling = knobs.get("test_time_scaling")
        coarse.test_time_nonrigid_object_removal_threshold = knobs.get("removal_threshold")
        pts, lat, dirs = case_inputs(name, cfg)
        with torch.no_grad():
            raw, details = kw["network_query_fn"](pts, dirs if cfg.use_viewdirs else None, {"ray_bending_latents": lat}, coarse,
                                                  detailed_output=True)
        arrays[f"{name}__points"] = pts.numpy()
        arrays[f"{name}__latents"] = lat.numpy()
        arrays[f"{name}__viewdirs"] = dirs.numpy()
        arrays[f"{name}__out__raw"] = raw.numpy().astype(np.float32)
        for k, v in details.items():
            arrays[f"{name}__out__{k}"] = v.detach().numpy().astype(np.float32)
        print(name, {k: tuple(v.shape) for k, v in details.items()}, "raw", tuple(raw.shape))
    out_path = out_path or os.path.join(REPO, "tests", "golden", "query", "query_points.npz")
    np.savez_compressed(out_path, **arrays)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
