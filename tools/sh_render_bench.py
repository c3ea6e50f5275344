#!/usr/bin/env python
"""One 512 x 384 frame of the view-dependent fitted checkpoint (tests/golden/fitted_config4.tar: view-dependent head + 7-layer bender, frame 3
of the example sequence), 192 samples per ray, rendered from a view-dependent bake (``field.bake(sh_degree=2)``, cut down to degrees 1 and 0)
plus a baked warp -- ``field.render_baked``: ONE ``nrnerf_sh_volume_render`` launch, no network -- in one process on one device:
    * canonical bakes of 128^3 and 256^3 over the box of the resolution series, float32 and float16 storage; warps of 32^3 and 64^3 (half);
    * medians of device-event timings of the whole ``render_baked`` call at degrees 0 (the record's ``"raw"`` alone: the kernel of
      ``nrnerf_warped_volume_render``, the floor), 1 and 2, each alone on the stream after a warm-up, and of the network's own frame
      (``render.batchify_rays``: the fine network on the same 192 samples, bf16);
    * PSNR of each degree against the network's frame: through ``render_volume(network=...)`` (the exact bender: what the grid and the
      truncated expansion cost) and through the 32^3 and 64^3 warps.
    python tools/sh_render_bench.py [repeats]          (default 20)
One JSON line per (volume, storage, degree).  The script has no time limit of its own: run it under one, ``timeout -k 10 900 python
tools/sh_render_bench.py``."""
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nonrigid_nerf_amd import field as F  # noqa: E402
from nonrigid_nerf_amd import render as R  # noqa: E402
from nonrigid_nerf_amd.checkpoint import load_checkpoint  # noqa: E402
from nonrigid_nerf_amd.driver import generate_rays  # noqa: E402

BOX = ((-0.8, -0.9, -1.4), (1.25, 0.8, 0.0))
FRAME, WIDTH, SAMPLES = 3, 512, 192


def event_ms(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * float(np.log10(mse))


def of_degree(base, degree, dtype):
    """The degree-2 bake cut down: the functions are orthonormal under the rule, so a lower degree's coefficients are the same numbers."""
    rec = {"raw": base["raw"].to(dtype), "min_point": base["min_point"], "max_point": base["max_point"]}
    if degree >= 1:
        sh = base["sh"][..., :12 * degree].clone()
        if degree == 1:
            sh[..., 9:] = 0
        rec.update(sh=sh.to(dtype), sh_degree=degree)
    return rec


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    gold = os.path.join(REPO, "tests", "golden")
    ck = load_checkpoint(os.path.join(gold, "fitted_config4.tar"), N_samples=64, N_importance=128, device=dev)
    for m in (ck.ray_bender, ck.network_fn, ck.network_fine):
        if m is not None:
            m.requires_grad_(False)
    z = np.load(os.path.join(gold, "example_sequence_96x72.npz"))
    near, far = float(z["bds"].min()) * 0.9, float(z["bds"].max())
    s = WIDTH / float(z["hwf"][1])
    h = int(round(float(z["hwf"][0]) * s))
    intrin = dict(height=h, width=WIDTH, focal_x=float(z["hwf"][2]) * s, focal_y=float(z["hwf"][2]) * s, center_x=WIDTH / 2, center_y=h / 2)
    rays = generate_rays(torch.from_numpy(z["poses"][FRAME]), intrin, near, far, False, dev)
    n = int(rays.shape[0])
    code = ck.latents[FRAME].to(dev).reshape(1, -1)
    net = ck.network_fine if ck.network_fine is not None else ck.network_fn
    R.set_precision("bf16")
    with torch.no_grad():
        network = lambda: R.batchify_rays(rays, {"ray_bending_latents": code.expand(n, -1)}, network_fn=net, network_fine=None,
                                          N_samples=SAMPLES, N_importance=0)
        ref = network()["rgb_map"]
        net_ms, net_min = event_ms(network, max(3, repeats // 4))
        warps = {res: F.bake_warp(net, code, BOX[0], BOX[1], res, dtype=torch.float16, precision="bf16") for res in (32, 64)}
        for res in (128, 256):
            base = F.bake({"network_fn": net}, None, BOX[0], BOX[1], res, precision="bf16", sh_degree=2)
            for dtype in (torch.float32, torch.float16):
                floor_ms = None
                for degree in (0, 1, 2):
                    rec = of_degree(base, degree, dtype)
                    fused = lambda: F.render_baked(rec, warps[32], rays, N_samples=SAMPLES)
                    f_ms, f_min = event_ms(fused, repeats)
                    floor_ms = f_ms if degree == 0 else floor_ms
                    exact = F.render_volume(rec, rays, network=net, latents=code, N_samples=SAMPLES, precision="bf16")["rgb_map"]
                    print(json.dumps(dict(what="sh bake", volume=res, storage=str(dtype).replace("torch.", ""), degree=degree,
                                          record_mib=round(sum(v.numel() * v.element_size() for v in rec.values() if torch.is_tensor(v)) / 2 ** 20, 1),
                                          rays=n, samples=SAMPLES, repeats=repeats, render_baked_ms=round(f_ms, 4), render_baked_min_ms=round(f_min, 4),
                                          over_degree_0=round(f_ms / floor_ms, 2), network_frame_ms=round(net_ms, 3),
                                          network_over_render_baked=round(net_ms / f_ms, 1),
                                          psnr_vs_network_exact_bender_db=round(psnr(exact, ref), 2),
                                          psnr_vs_network_warp32_db=round(psnr(fused()["rgb_map"], ref), 2),
                                          psnr_vs_network_warp64_db=round(psnr(F.render_baked(rec, warps[64], rays, N_samples=SAMPLES)["rgb_map"], ref), 2))),
                          flush=True)
                    del rec, exact
            del base
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
