#!/usr/bin/env python
"""Throughput of the field query on the fitted checkpoint (tests/golden/fitted_latest.tar), per precision: points/s of
``render.query_points`` on scattered points, voxels/s of ``field.sample_grid``, and -- to read the two side by side -- the samples/s
of a coarse-only ``render_rays`` call over the same number of samples; with the kernels the query took (``nrnerf_profile``).
    python tools/query_bench.py [rows] [samples] [grid] [repeats]          (defaults 16384 64 128 10)
One JSON line per precision."""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nonrigid_nerf_amd import field as F  # noqa: E402
from nonrigid_nerf_amd import render as R  # noqa: E402
from nonrigid_nerf_amd.checkpoint import load_checkpoint  # noqa: E402


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats


def main():
    rows, samples, grid, repeats = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 16384), (2, 64), (3, 128), (4, 10)))
    dev = torch.device("cuda:0")
    gold = os.path.join(REPO, "tests", "golden")
    ck = load_checkpoint(os.path.join(gold, "fitted_latest.tar"), N_samples=samples, N_importance=128, device=dev)
    z = np.load(os.path.join(gold, "example_sequence_96x72.npz"))
    near, far = float(z["bds"].min()) * 0.9, float(z["bds"].max())
    g = torch.Generator().manual_seed(0)
    pts = ((torch.rand(rows, samples, 3, generator=g) * 2 - 1) * 0.5 * far).to(dev)
    code = ck.latents[3].reshape(1, -1)
    lat = code.expand(rows, -1)
    o = torch.zeros(rows, 3)
    d = torch.nn.functional.normalize(torch.randn(rows, 3, generator=g), dim=-1)
    rays = torch.cat([o, d, torch.full((rows, 1), near), torch.full((rows, 1), far)], -1).to(dev)
    lo, hi = np.full(3, -0.5 * far), np.full(3, 0.5 * far)
    for prec in ("f32", "bf16", "f16"):
        R.set_precision(prec)
        model = R.get_model(ck.network_fn, None, device=dev)
        with torch.no_grad():
            t_q = timed(lambda: R.query_points(pts, ck.network_fn, lat), repeats)
            t_g = timed(lambda: F.sample_grid(ck.render_kwargs_test, code, lo, hi, grid, fine=False), max(1, repeats // 3))
            t_r = timed(lambda: R.render_rays(rays, ck.network_fn, N_samples=samples, N_importance=0,
                                              additional_pixel_information={"ray_bending_latents": lat}), repeats)
            model.profile_begin()
            R.query_points(pts, ck.network_fn, lat)
            prof = model.profile_end()
        kernels = {k: dict(kernel=v["kernel"], ms=round(v["ms"], 4)) for k, v in prof.items() if v["launches"]}
        print(json.dumps(dict(precision=prec, rows=rows, samples=samples, query_points_per_s=rows * samples / t_q,
                              grid=grid, sample_grid_voxels_per_s=grid ** 3 / t_g,
                              coarse_only_render_samples_per_s=rows * samples / t_r, query_kernels=kernels)))
    R.set_precision("bf16")


if __name__ == "__main__":
    main()
