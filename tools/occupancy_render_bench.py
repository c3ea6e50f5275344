#!/usr/bin/env python
"""What an occupancy mask is worth on one 512 x 384 frame of the view-dependent fitted checkpoint (tests/golden/fitted_config4.tar, frame 3 of
the example sequence), 192 samples per ray, rendered from half bakes of 128^3 and 256^3 at degrees 0 / 1 / 2 through the 32^3 half warp --
``field.render_baked`` with and without ``occupancy=`` -- in one process on one device:
    * the share of empty blocks of the exact mask (threshold 0) at blocks of 4 / 8 / 16 cells, and the share of the frame's in-box samples
      that fall in an empty block of each size (counted from the lookup kernel's own ``raw``: an in-box sample the mask skipped is all zero);
    * medians of device-event timings of the whole ``render_baked`` call, each alone on the stream after a warm-up: through the EXISTING
      entry point (the baseline), with an all-ones mask (the price of the bit lookup), with the exact mask at blocks of 4 / 8 / 16, and with
      lossy masks (threshold > 0, block 8) next to their PSNR against the unmasked frame;
    * the mask's own build time and the volume bytes it streams per second;
    * ``==`` of the exact mask's rgb / disp / acc with the unmasked frame's (NaN equal to NaN), once per row.
    python tools/occupancy_render_bench.py [repeats]          (default 20)
One JSON line per (volume, degree).  The script has no time limit of its own: run it under one, ``timeout -k 10 900 python
tools/occupancy_render_bench.py``."""
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
THRESHOLDS = (0.5, 2.0, 5.0)


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
    return statistics.median(ms)


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


def empty_share(mask):
    """The share of a mask's blocks whose bit is clear."""
    n = 1
    for g in mask["grid"]:
        n *= -(-(int(g) - 1) // mask["block"])
    words = mask["bits"].cpu().numpy().view(np.uint32)
    return 1.0 - sum(bin(int(w)).count("1") for w in words) / n


def same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


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
        warp = F.bake_warp(net, code, BOX[0], BOX[1], 32, dtype=torch.float16, precision="bf16")
        for res in (128, 256):
            base = F.bake({"network_fn": net}, None, BOX[0], BOX[1], res, precision="bf16", sh_degree=2)
            sigma = base["raw"][..., 3].half().float()
            for degree in (0, 1, 2):
                rec = of_degree(base, degree, torch.float16)
                render = lambda occupancy=None: F.render_baked(rec, warp, rays, N_samples=SAMPLES, occupancy=occupancy)
                exact = {b: F.build_occupancy(rec, block=b) for b in (4, 8, 16)}
                ones = dict(exact[8], bits=torch.full_like(exact[8]["bits"], -1))
                # in-box samples and the ones the block-8 mask skips, from the lookup kernels' own raw (degree-0 lookup: raw alone)
                plain = {k: rec[k] for k in ("raw", "min_point", "max_point")}
                pts = F.warped_volume_render(plain, warp, rays, N_samples=SAMPLES, composite=False, return_points=True)["points4"][..., :3]
                lo, hi = (torch.tensor(v, device=dev) for v in BOX)
                inside = ((pts >= lo) & (pts <= hi)).all(-1)
                n_inside = max(1, int(inside.sum()))
                skipped = {}
                for b, m in exact.items():
                    kept = F.warped_volume_render(plain, warp, rays, N_samples=SAMPLES, composite=False, occupancy=m)["raw"]
                    skipped[str(b)] = round(int((inside & (kept == 0).all(-1)).sum()) / n_inside, 4)
                    del kept
                del pts
                want = render()
                got = render(exact[8])
                bit_identical = all(same(got[k], want[k]) for k in ("rgb_map", "disp_map", "acc_map"))
                row = dict(what="occupancy", volume=res, storage="float16", degree=degree, rays=n, samples=SAMPLES, repeats=repeats,
                           sigma_logit_positive_share=round(float((sigma > 0).float().mean()), 4),
                           empty_blocks_share={str(b): round(empty_share(m), 4) for b, m in exact.items()},
                           in_box_samples_share=round(float(inside.float().mean()), 4),
                           skipped_of_in_box_samples=skipped,
                           exact_mask_is_bit_identical=bit_identical,
                           unmasked_ms=round(event_ms(render, repeats), 4),
                           all_ones_mask_ms=round(event_ms(lambda: render(ones), repeats), 4),
                           exact_mask_ms={str(b): round(event_ms(lambda m=m: render(m), repeats), 4) for b, m in exact.items()})
                build_ms = event_ms(lambda: F.build_occupancy(plain, block=8), repeats)          # (`raw` alone: no finiteness pass over `sh`)
                row.update(build_block8_ms=round(build_ms, 4),
                           build_volume_gb_per_s=round(rec["raw"].numel() * rec["raw"].element_size() / build_ms / 1e6, 1))
                lossy = {}
                for thr in THRESHOLDS:
                    m = F.build_occupancy(rec, block=8, threshold=thr)
                    lossy[str(thr)] = dict(empty_blocks_share=round(empty_share(m), 4), ms=round(event_ms(lambda m=m: render(m), repeats), 4),
                                           psnr_vs_unmasked_db=round(psnr(render(m)["rgb_map"], want["rgb_map"]), 2))
                row["lossy_block8"] = lossy
                print(json.dumps(row), flush=True)
                del rec, want, got
            del base
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
