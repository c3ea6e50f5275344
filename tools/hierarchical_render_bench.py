#!/usr/bin/env python
"""One 512 x 384 frame of the fitted checkpoint (tests/golden/fitted_latest.tar, frame 3 of the example sequence) rendered from a 256^3 half bake
and a 32^3 half warp with hierarchical sampling -- ``field.render_baked(N_importance=...)`` -- in one process on one device:
    * 64 + 64 and 64 + 128 samples through the fused kernel (``nrnerf_hierarchical_volume_render``: one launch) and through the composed route
      (``nrnerf_warped_volume_render`` -> ``nrnerf_composite_forward`` -> ``nrnerf_warped_volume_render``: three launches, ``raw`` and the merged
      depths through memory), next to 128 and 192 uniform samples (``nrnerf_warped_volume_render``: one launch);
    * KERNEL time: the entry points alone on prepared records and preallocated outputs; CALL time: the whole ``render_baked`` call, allocations
      included.  Device-event timings; the variants of a row take turns, round by round, and the medians and minima over the rounds are reported;
    * PSNR of each image against the network's own frame (``render.batchify_rays``, 64 + 128, bf16), and a check that the two routes return
      the same bits;
    * the kernel times of both routes over the lane-width classes of the fused kernel (rows "kernel sweep").
    python tools/hierarchical_render_bench.py [rounds]          (default 20)
One JSON line per row, also written to profiles/hierarchical_render_bench.txt.  The script has no time limit of its own: run it under one,
``timeout -k 10 600 python tools/hierarchical_render_bench.py``."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nonrigid_nerf_amd import _lib  # noqa: E402
from nonrigid_nerf_amd import field as F  # noqa: E402
from nonrigid_nerf_amd import render as R  # noqa: E402
from nonrigid_nerf_amd.checkpoint import load_checkpoint  # noqa: E402
from nonrigid_nerf_amd.driver import generate_rays  # noqa: E402

BOX = ((-0.8, -0.9, -1.4), (1.25, 0.8, 0.0))
FRAME, WIDTH = 3, 512
VOLUME, WARP = 256, 32


def interleaved_ms(fns, rounds):
    """``{name: (median, min)}`` of device-event timings; the variants take turns within every round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v)) for k, v in ms.items()}


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * float(np.log10(mse))


def grids_into(a, vol, wrp):
    v, w = vol["raw"], wrp["warp"]
    a.volume, a.volume_dtype = v.data_ptr(), F._VOLUME_DTYPES[v.dtype]
    a.g[:] = (v.shape[2], v.shape[1], v.shape[0])
    a.min_point[:], a.max_point[:] = F.grid_extent(vol["min_point"], vol["max_point"])[0].tolist(), F.grid_extent(vol["min_point"], vol["max_point"])[1].tolist()
    a.warp, a.warp_dtype = w.data_ptr(), F._VOLUME_DTYPES[w.dtype]
    a.warp_g[:] = (w.shape[2], w.shape[1], w.shape[0])
    a.warp_min_point[:], a.warp_max_point[:] = F.grid_extent(wrp["min_point"], wrp["max_point"])[0].tolist(), F.grid_extent(wrp["min_point"], wrp["max_point"])[1].tolist()


def kernel_launchers(vol, wrp, rays, S, I):
    """``(fused, composed, uniform, keep)``: closures that launch the entry points alone on records prepared here, outputs preallocated."""
    dev, n = rays.device, int(rays.shape[0])
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    keep = dict(rgb=new(n, 3), disp=new(n), acc=new(n), rgb0=new(n, 3), disp0=new(n), acc0=new(n), z_std=new(n), z=new(n, S + I), raw=new(n, S, 4))
    h = _lib.HierarchicalVolumeRenderArgs()
    h.struct_size, h.n_rays, h.n_samples, h.n_importance = C.sizeof(h), n, S, I
    h.rays, h.ray_stride = rays.data_ptr(), int(rays.shape[1])
    grids_into(h, vol, wrp)
    h.rgb, h.disp, h.acc = keep["rgb"].data_ptr(), keep["disp"].data_ptr(), keep["acc"].data_ptr()
    h.rgb0, h.disp0, h.acc0 = keep["rgb0"].data_ptr(), keep["disp0"].data_ptr(), keep["acc0"].data_ptr()
    h.z_std, h.z_vals = keep["z_std"].data_ptr(), keep["z"].data_ptr()

    def warped(samples, z, raw, maps):
        w = _lib.WarpedVolumeRenderArgs()
        w.struct_size, w.n_rays, w.n_samples = C.sizeof(w), n, samples
        w.rays, w.ray_stride = rays.data_ptr(), int(rays.shape[1])
        grids_into(w, vol, wrp)
        w.z = z.data_ptr() if z is not None else None
        w.raw = raw.data_ptr() if raw is not None else None
        w.rgb, w.disp, w.acc = (keep[k].data_ptr() for k in maps)
        return w
    wa, wc, wu = warped(S, None, keep["raw"], ("rgb0", "disp0", "acc0")), warped(S + I, keep["z"], None, ("rgb", "disp", "acc")), \
        warped(S + I, None, None, ("rgb", "disp", "acc"))
    b = _lib.CompositeArgs()
    b.struct_size, b.n_rays, b.n_samples, b.n_importance = C.sizeof(b), n, S, I
    b.rays, b.ray_stride, b.raw4 = rays.data_ptr(), int(rays.shape[1]), keep["raw"].data_ptr()
    b.rgb, b.disp, b.acc = keep["rgb0"].data_ptr(), keep["disp0"].data_ptr(), keep["acc0"].data_ptr()
    b.z_std, b.z_merged = keep["z_std"].data_ptr(), keep["z"].data_ptr()

    def fused():
        _lib.check(lib.nrnerf_hierarchical_volume_render(C.byref(h), stream), "nrnerf_hierarchical_volume_render")

    def composed():
        _lib.check(lib.nrnerf_warped_volume_render(C.byref(wa), stream), "nrnerf_warped_volume_render")
        _lib.check(lib.nrnerf_composite_forward(C.byref(b), stream), "nrnerf_composite_forward")
        _lib.check(lib.nrnerf_warped_volume_render(C.byref(wc), stream), "nrnerf_warped_volume_render")

    def uniform():
        _lib.check(lib.nrnerf_warped_volume_render(C.byref(wu), stream), "nrnerf_warped_volume_render")
    return fused, composed, uniform, keep


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
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
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    R.set_precision("bf16")
    with torch.no_grad():
        ref = R.batchify_rays(rays, {"ray_bending_latents": code.expand(n, -1)}, network_fn=ck.network_fn, network_fine=ck.network_fine,
                              N_samples=64, N_importance=128)["rgb_map"]
        base = F.bake(ck.render_kwargs_test, None, BOX[0], BOX[1], VOLUME, precision="bf16")
        vol = dict(base, raw=base["raw"].to(torch.float16))
        wrp = F.bake_warp(ck.render_kwargs_test, code, BOX[0], BOX[1], WARP, dtype=torch.float16, precision="bf16")
        common = dict(what="hierarchical baked render", device=torch.cuda.get_device_name(0), volume=VOLUME, warp=WARP, dtype="float16", rays=n,
                      rounds=rounds)
        for S, I in ((64, 64), (64, 128)):
            fused_k, composed_k, uniform_k, keep = kernel_launchers(vol, wrp, rays, S, I)
            kernel = interleaved_ms(dict(fused=fused_k, composed=composed_k, uniform=uniform_k), rounds)
            call = interleaved_ms(dict(fused=lambda: F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, fused=True),
                                       composed=lambda: F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, fused=False),
                                       uniform=lambda: F.render_baked(vol, wrp, rays, N_samples=S + I)), rounds)
            a = F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, fused=True)
            b = F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, fused=False)
            u = F.render_baked(vol, wrp, rays, N_samples=S + I)
            same = all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
            ms = lambda t: dict(median_ms=round(t[0], 4), min_ms=round(t[1], 4))
            emit(**common, coarse=S, importance=I, uniform=S + I, routes_same_bits=same,
                 kernel_fused=ms(kernel["fused"]), kernel_composed=ms(kernel["composed"]), kernel_uniform=ms(kernel["uniform"]),
                 call_fused=ms(call["fused"]), call_composed=ms(call["composed"]), call_uniform=ms(call["uniform"]),
                 composed_over_fused_kernel=round(kernel["composed"][0] / kernel["fused"][0], 3),
                 composed_over_fused_call=round(call["composed"][0] / call["fused"][0], 3),
                 psnr_hierarchical_vs_network_db=round(psnr(a["rgb_map"], ref), 2), psnr_coarse_vs_network_db=round(psnr(a["rgb0"], ref), 2),
                 psnr_uniform_vs_network_db=round(psnr(u["rgb_map"], ref), 2), mean_z_std=round(float(a["z_std"].mean()), 5))
            del keep
        # the kernels alone over the lane-width classes: where the fused route pays (what ``fused=None`` resolves to, field._use_fused)
        for S, I in ((32, 32), (48, 80), (64, 128), (64, 192), (128, 128), (128, 256), (192, 64), (256, 256)):
            fused_k, composed_k, uniform_k, keep = kernel_launchers(vol, wrp, rays, S, I)
            kernel = interleaved_ms(dict(fused=fused_k, composed=composed_k, uniform=uniform_k), max(5, rounds // 2))
            emit(what="kernel sweep", coarse=S, importance=I, fused_median_ms=round(kernel["fused"][0], 4),
                 composed_median_ms=round(kernel["composed"][0], 4), uniform_median_ms=round(kernel["uniform"][0], 4),
                 composed_over_fused=round(kernel["composed"][0] / kernel["fused"][0], 3))
            del keep
    out = os.path.join(REPO, "profiles", "hierarchical_render_bench.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
