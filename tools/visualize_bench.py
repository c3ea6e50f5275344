#!/usr/bin/env python
"""Cost of free_viewpoint_rendering.py's per-frame images on the device (nonrigid_nerf_amd.visualize):

1. device ms per frame for the full set -- disp, disp_jet, disp_phong, correspondences, rigidity, rigidity_jet, PSNR / SSIM with both
   error maps, one background-stability accumulate -- at 512 x 384 and 1920 x 1080 (HIP events around the launches, mean of the reps);
2. driver.render_path frames/s on synthetic weights (bf16, 64 + 128 samples) without and with visualizations="all", metrics=True,
   stability=True (wall clock, the copies to pinned host memory included).

    python tools/visualize_bench.py [frames] [H] [W]          (defaults: 24 384 512)
Prints one JSON line."""
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nonrigid_nerf_amd import render as R
from nonrigid_nerf_amd import visualize as V
from nonrigid_nerf_amd.driver import render_path
from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_scene

DEV = "cuda:0"


def maps_ms(H, W, reps=20):
    g = torch.Generator(device=DEV).manual_seed(0)
    disp = 0.05 + torch.rand(1, H, W, device=DEV, generator=g)
    rgb = torch.rand(1, H, W, 3, device=DEV, generator=g)
    gt = torch.rand(1, H, W, 3, device=DEV, generator=g)
    pts = torch.randn(1, H, W, 3, device=DEV, generator=g)
    rig = torch.rand(1, H, W, device=DEV, generator=g)
    st = V.BackgroundStability()

    def once():
        V.disparity_maps(disp)
        V.correspondence_rgb(pts, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
        V.rigidity_maps(rig)
        V.metrics_on_device(gt, rgb, mask_ref=gt[0], error_maps=True)
        st.add(rgb)
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def render_fps(frames, H, W):
    cfg = SceneConfig()
    scene = make_scene(cfg, 0)
    rb, coarse, fine = build_modules(scene, device=DEV)
    R.set_precision("bf16")
    poses, intr = [], []
    for k in range(frames):
        a = 0.02 * k - 0.4
        poses.append(torch.tensor([[math.cos(a), 0.0, math.sin(a), 0.1 * math.sin(a)], [0.0, 1.0, 0.0, 0.0],
                                   [-math.sin(a), 0.0, math.cos(a), 0.15]]))
        intr.append(dict(height=H, width=W, focal_x=256.6 * W / 512, focal_y=256.6 * H / 384, center_x=W / 2, center_y=H / 2))
    codes = torch.randn(frames, 32, generator=torch.Generator().manual_seed(1)).cuda() * 0.1
    gt = [torch.rand(H, W, 3, generator=torch.Generator().manual_seed(k)).numpy() for k in range(frames)]
    kw = dict(network_fn=coarse, network_fine=fine, network_query_fn=None, N_samples=64, N_importance=128, perturb=False,
              raw_noise_std=0.0, white_bkgd=False, lindisp=False, ndc=False, use_viewdirs=False, ray_bender=rb, near=cfg.near, far=cfg.far)
    extra = dict(visualizations="all", volume_extent=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), metrics=True, stability=True, gt_imgs=gt)
    res = {}
    for label, ex in (("plain", {}), ("visualized", extra)):
        render_path(poses[:2], intr[:2], 32768, kw, codes[:2], rgb_dtype="uint8", **({**ex, "gt_imgs": gt[:2]} if ex else {}))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        render_path(poses, intr, 32768, kw, codes, rgb_dtype="uint8", **ex)
        torch.cuda.synchronize()
        res[label] = frames / (time.perf_counter() - t0)
    R.set_precision("bf16")
    return res


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 384
    W = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    out = {"maps_ms_512x384": round(maps_ms(384, 512), 4), "maps_ms_1920x1080": round(maps_ms(1080, 1920), 4)}
    fps = render_fps(frames, H, W)
    out.update({"render_path_fps_plain": round(fps["plain"], 3), "render_path_fps_visualized": round(fps["visualized"], 3),
                "fps_kept": round(fps["visualized"] / fps["plain"], 4), "frames": frames, "height": H, "width": W,
                "device": torch.cuda.get_device_name(0)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
