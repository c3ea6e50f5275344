#!/usr/bin/env python
"""One 512 x 384 frame of the fitted checkpoint (tests/golden/fitted_latest.tar, frame 3 of the example sequence) rendered from baked
canonical volumes -- ``field.render_volume``: ``nrnerf_sample_depths_points`` -> ``nrnerf_bend_points`` -> ``nrnerf_volume_render``, 192 samples
per ray -- next to the same frame through the networks (``Model.render``, bf16, 64 + 128), in one process on one device:
    * bakes of 128^3 and 256^3 over the box of the resolution series (tests/volume_reference.py), float32 and float16 storage;
    * medians of device-event timings of the bender launch alone, the volume kernel alone (on the bent points of that launch) and the whole
      ``render_volume`` call, each alone on the stream after a warm-up, and of the network frame;
    * the volume kernel's achieved bytes/s, counted from shapes: per sample 16 B of bent point read and, for the samples inside the box,
      eight corners of 16 / 8 B gathered (cache hits included: this is the gather rate, not HBM traffic), plus the three maps;
    * PSNR of every image against the network frame.
    python tools/volume_render_bench.py [repeats]          (default 20)
One JSON line per volume and one for the network frame.  The script has no time limit of its own: run it under one, ``timeout -k 10 600
python tools/volume_render_bench.py``."""
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


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    gold = os.path.join(REPO, "tests", "golden")
    ck = load_checkpoint(os.path.join(gold, "fitted_latest.tar"), N_samples=64, N_importance=128, device=dev)
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
    lat = code.expand(n, -1)
    net = ck.network_fine if ck.network_fine is not None else ck.network_fn
    with torch.no_grad():
        model = R.get_model(ck.network_fn, ck.network_fine, precision="bf16", device=dev)
        frame = lambda: model.render(rays, lat, 64, 128)
        ref = frame()["rgb_map"]
        net_ms, net_min = event_ms(frame, repeats)
        print(json.dumps(dict(what="network frame", route="Model.render bf16 64 + 128", rays=n, height=h, width=WIDTH, repeats=repeats,
                              ms=round(net_ms, 4), min_ms=round(net_min, 4))), flush=True)
        bender = R.get_model(net, None, precision="bf16", device=dev)
        knobs = R._query_knobs(net)
        zs, pts = F.sample_rays(rays, SAMPLES)
        bend = lambda: bender.bend_points(pts, lat, rigidity_cutoff=knobs["rigidity_cutoff"], test_time_scaling=knobs["test_time_scaling"])
        bent4 = bend()
        bend_ms, bend_min = event_ms(bend, repeats)
        sample_ms, _ = event_ms(lambda: F.sample_rays(rays, SAMPLES), repeats)
        for res in (128, 256):
            base = F.bake(ck.render_kwargs_test, None, BOX[0], BOX[1], res, precision="bf16")
            for dtype in (torch.float32, torch.float16):
                vol = dict(base, raw=base["raw"].to(dtype))
                kernel = lambda: F.volume_render(vol, rays, N_samples=SAMPLES, z_vals=zs, points4=bent4)
                whole = lambda: F.render_volume(vol, rays, network=net, latents=code, N_samples=SAMPLES, precision="bf16")
                out = whole()
                raw = F.volume_render(vol, rays, N_samples=SAMPLES, z_vals=zs, points4=bent4, composite=False)["raw"]
                inside = int((raw != 0).any(-1).sum())
                k_ms, k_min = event_ms(kernel, repeats)
                w_ms, w_min = event_ms(whole, repeats)
                vertex = 16 if dtype == torch.float32 else 8
                nbytes = n * SAMPLES * (16 + 4) + inside * 8 * vertex + n * 20
                print(json.dumps(dict(what="baked volume", resolution=res, dtype=str(dtype).replace("torch.", ""), volume_mib=round(res ** 3 * vertex / 2 ** 20, 1),
                                      rays=n, samples=SAMPLES, samples_inside_share=round(inside / (n * SAMPLES), 4), repeats=repeats,
                                      sample_points_ms=round(sample_ms, 4), bender_ms=round(bend_ms, 4), bender_min_ms=round(bend_min, 4),
                                      volume_kernel_ms=round(k_ms, 4), volume_kernel_min_ms=round(k_min, 4),
                                      volume_kernel_gather_bytes=nbytes, volume_kernel_tb_per_s=round(nbytes / (k_ms * 1e-3) / 1e12, 3),
                                      render_volume_ms=round(w_ms, 4), render_volume_min_ms=round(w_min, 4),
                                      network_frame_over_render_volume=round(net_ms / w_ms, 2),
                                      psnr_vs_network_frame_db=round(psnr(out["rgb_map"], ref), 2))), flush=True)


if __name__ == "__main__":
    main()
