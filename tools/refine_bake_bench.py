#!/usr/bin/env python
"""What the gradient of the grid lookup buys, and what it costs, in one process on one device.

A. The refinement series.  ``fitted_latest`` (tests/golden), frames of the example sequence at 48 x 36 rays, 192 samples of the coarse spacing,
   every sample bent EXACTLY (``nrnerf_bend_points``, float32).  The 96^3 float32 canonical bake is refined with Adam (lr 2e-2) on the mean
   squared error against the fine network's renders (64 + 128 samples, float32) of the eight frames 0, 5, ..., 35, all eight in every
   iteration; frame 3 is held out.  One iteration is ``field.grid_lookup`` (forward: the lookup kernel, backward:
   ``nrnerf_grid_lookup_backward``) + the compositing kernels of the training step + torch's Adam.  PSNR of both sets at 0 / 60 / 120 / 240
   iterations, and the median time of an iteration (host clock around a synchronise).
B. The backward call by itself.  Straight samples ``o + d z`` of frame 3's camera (1024 rays x 192 and 512 x 384 rays x 192) through the box
   of the series, grids of 96^3 and 256^3 in float32 and half: medians of device-event timings of ``nrnerf_grid_lookup_backward`` with both
   outputs (d_grid accumulating into a zeroed buffer), d_grid alone and d_points alone, next to ``torch.nn.functional.grid_sample``'s backward
   (``align_corners=True``, trilinear, zeros padding; the gradients of input and grid, timed as ``torch.autograd.grad`` on a graph built outside
   the window) and next to the same ``torch.autograd.grad`` through ``field.grid_lookup`` (the entry point + the zeroing + the cast).
    python tools/refine_bake_bench.py [iterations] [repeats]          (defaults 240, 20)
One JSON line per measurement.  The script has no time limit of its own: run it under one, ``timeout -k 10 900 python
tools/refine_bake_bench.py``."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nonrigid_nerf_amd import _lib  # noqa: E402
from nonrigid_nerf_amd import field as F  # noqa: E402
from nonrigid_nerf_amd import render as R  # noqa: E402
from nonrigid_nerf_amd.checkpoint import load_checkpoint  # noqa: E402
from nonrigid_nerf_amd.driver import generate_rays  # noqa: E402
from nonrigid_nerf_amd.training import _Composite  # noqa: E402

BOX = ((-0.8, -0.9, -1.4), (1.25, 0.8, 0.0))
TRAIN_FRAMES, HELD_OUT, WIDTH, SAMPLES, VOLUME, LR = tuple(range(0, 40, 5)), 3, 48, 192, 96, 2e-2
REPORT_AT = (0, 60, 120, 240)


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * float(np.log10(mse))


def camera(z, width):
    s = width / float(z["hwf"][1])
    h = int(round(float(z["hwf"][0]) * s))
    return dict(height=h, width=width, focal_x=float(z["hwf"][2]) * s, focal_y=float(z["hwf"][2]) * s, center_x=width / 2, center_y=h / 2)


def event_ms(fn, repeats, before=None):
    for _ in range(3):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4), round(min(ms), 4)


def refinement_series(ck, z, dev, iterations):
    near, far = float(z["bds"].min()) * 0.9, float(z["bds"].max())
    intrin = camera(z, WIDTH)
    model = R.get_model(ck.network_fine, None, precision="f32", device=dev)
    sets = {}
    R.set_precision("f32")
    try:
        with torch.no_grad():
            for name, frames in (("train", TRAIN_FRAMES), ("held_out", (HELD_OUT,))):
                rays, p4, zs, target = [], [], [], []
                for f in frames:
                    r = generate_rays(torch.from_numpy(z["poses"][f]), intrin, near, far, False, dev)
                    code = ck.latents[f].detach().to(dev).reshape(1, -1).float()
                    n = int(r.shape[0])
                    net = R.batchify_rays(r, {"ray_bending_latents": code.expand(n, -1)}, network_fn=ck.network_fn, network_fine=ck.network_fine,
                                          N_samples=64, N_importance=128)
                    zz, pts = F.sample_rays(r, SAMPLES)
                    rays.append(r), zs.append(zz), target.append(net["rgb_map"])
                    p4.append(model.bend_points(pts, code.expand(n, -1).contiguous()))
                sets[name] = tuple(torch.cat(t, 0).contiguous() for t in (rays, p4, zs, target))
    finally:
        R.set_precision("bf16")
    lo, hi = BOX
    bake = F.bake({"network_fn": ck.network_fn, "network_fine": ck.network_fine}, None, lo, hi, VOLUME, precision="f32")
    raw = bake["raw"].detach().clone().requires_grad_(True)

    def render(name):
        rays, p4, zs, _ = sets[name]
        logits = F.grid_lookup(raw, lo, hi, p4[..., :3])
        return _Composite.apply(logits, rays, zs, None, False, 0, None)[0]

    def report(it):
        with torch.no_grad():
            row = {name: round(psnr(render(name), sets[name][3]), 2) for name in sets}
        print(json.dumps(dict(what="refinement series", volume=VOLUME, iterations=it, lr=LR, rays_per_iteration=int(sets["train"][0].shape[0]),
                              samples=SAMPLES, psnr_held_out_db=row["held_out"], psnr_train_db=row["train"])), flush=True)

    opt = torch.optim.Adam([raw], lr=LR)
    report(0)
    times = []
    for it in range(1, iterations + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = ((render("train") - sets["train"][3]) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        if it in REPORT_AT or it == iterations:
            report(it)
    if times:
        print(json.dumps(dict(what="refinement iteration", ms_median=round(statistics.median(times[3:] or times), 3),
                              ms_min=round(min(times), 3), iterations=len(times))), flush=True)


def backward_call(grid, lo, hi, pts4, cot, d_grid, d_points):
    a = _lib.GridLookupBackwardArgs()
    a.struct_size = C.sizeof(a)
    a.grid, a.grid_dtype = grid.data_ptr(), _lib.VOLUME_F16 if grid.dtype == torch.float16 else _lib.VOLUME_F32
    a.g[:] = (grid.shape[2], grid.shape[1], grid.shape[0])
    a.min_point[:], a.max_point[:] = lo, hi
    a.n_points, a.points, a.point_stride, a.g_value = int(pts4.shape[0]), pts4.data_ptr(), 4, cot.data_ptr()
    a.d_grid = None if d_grid is None else d_grid.data_ptr()
    a.d_points = None if d_points is None else d_points.data_ptr()
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(grid.device).cuda_stream)
    return lambda: _lib.check(lib.nrnerf_grid_lookup_backward(C.byref(a), stream), "nrnerf_grid_lookup_backward")


def backward_timings(z, dev, repeats):
    near, far = float(z["bds"].min()) * 0.9, float(z["bds"].max())
    full = generate_rays(torch.from_numpy(z["poses"][HELD_OUT]), camera(z, 512), near, far, False, dev)
    pick = torch.randperm(int(full.shape[0]), generator=torch.Generator().manual_seed(0))[:1024].to(dev)
    lo, hi = BOX
    lo_t, hi_t = torch.tensor(lo, device=dev), torch.tensor(hi, device=dev)
    for rays in (full[pick].contiguous(), full):
        with torch.no_grad():
            _, pts = F.sample_rays(rays, SAMPLES)
        pts = pts.reshape(-1, 3)
        m = int(pts.shape[0])
        inside = float(((pts >= lo_t) & (pts <= hi_t)).all(-1).float().mean())
        pts4 = torch.cat([pts, torch.zeros_like(pts[:, :1])], -1).contiguous()
        cot = torch.randn(m, 4, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        norm = ((pts - lo_t) / (hi_t - lo_t) * 2 - 1).reshape(1, 1, 1, m, 3)             # grid_sample's coordinates: (x, y, z) in -1 .. 1
        for res in (96, 256):
            base = torch.randn(res, res, res, 4, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
            for dtype in (torch.float32, torch.float16):
                grid = base.to(dtype)
                d_grid, d_points = torch.zeros(grid.shape, dtype=torch.float32, device=dev), torch.empty(m, 3, device=dev)
                both = event_ms(backward_call(grid, lo, hi, pts4, cot, d_grid, d_points), repeats)
                only_g = event_ms(backward_call(grid, lo, hi, pts4, cot, d_grid, None), repeats)
                only_p = event_ms(backward_call(grid, lo, hi, pts4, cot, None, d_points), repeats)
                del d_grid, d_points
                # the same gradients through autograd: ours, and grid_sample's on a channels-first copy of the grid
                held = {}

                def ours_graph():
                    g, p = grid.detach().requires_grad_(True), pts.detach().requires_grad_(True)
                    held["ours"] = (F.grid_lookup(g, lo, hi, p), g, p)

                def ours_backward():
                    v, g, p = held["ours"]
                    torch.autograd.grad(v, (g, p), cot)

                ours = event_ms(ours_backward, repeats, before=ours_graph)
                held.clear()
                vol5 = grid.permute(3, 0, 1, 2)[None].contiguous()
                cot5 = cot.t().reshape(1, 4, 1, 1, m).to(dtype).contiguous()

                def torch_graph():
                    g, p = vol5.detach().requires_grad_(True), norm.to(dtype).requires_grad_(True)
                    held["torch"] = (torch.nn.functional.grid_sample(g, p, mode="bilinear", padding_mode="zeros", align_corners=True), g, p)

                def torch_backward():
                    v, g, p = held["torch"]
                    torch.autograd.grad(v, (g, p), cot5)

                theirs = event_ms(torch_backward, repeats, before=torch_graph)
                held.clear()
                del vol5, cot5
                print(json.dumps(dict(what="lookup backward", points=m, inside_share=round(inside, 3), grid=res,
                                      grid_dtype=str(dtype).replace("torch.", ""), repeats=repeats,
                                      entry_point_both_ms=both[0], entry_point_both_min_ms=both[1], entry_point_d_grid_ms=only_g[0],
                                      entry_point_d_points_ms=only_p[0], grid_lookup_autograd_ms=ours[0], grid_lookup_autograd_min_ms=ours[1],
                                      grid_sample_backward_ms=theirs[0], grid_sample_backward_min_ms=theirs[1],
                                      grid_sample_over_entry_point=round(theirs[0] / both[0], 2),
                                      grid_sample_over_grid_lookup_autograd=round(theirs[0] / ours[0], 2))), flush=True)
            del base


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    gold = os.path.join(REPO, "tests", "golden")
    ck = load_checkpoint(os.path.join(gold, "fitted_latest.tar"), N_samples=64, N_importance=128, device=dev)
    for m in (ck.ray_bender, ck.network_fn, ck.network_fine):
        if m is not None:
            m.requires_grad_(False)
    z = np.load(os.path.join(gold, "example_sequence_96x72.npz"))
    if iterations > 0:
        refinement_series(ck, z, dev, iterations)
    if repeats > 0:
        backward_timings(z, dev, repeats)


if __name__ == "__main__":
    main()
