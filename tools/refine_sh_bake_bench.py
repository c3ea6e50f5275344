#!/usr/bin/env python
"""What the gradient of the spherical-harmonic colour sum buys, and what it costs, in one process on one device.

A. The refinement series.  ``fitted_config4`` (tests/golden: a view-dependent head behind a 7-layer bender), frames of the example sequence at
   48 x 36 rays, 192 samples of the coarse spacing, every sample bent EXACTLY (``nrnerf_bend_points``, float32).  The 128^3 degree-2 float32
   bake (``raw`` and ``sh``) is refined with Adam (lr 2e-2) on the mean squared error against the fine network's renders (the same 192
   samples, float32) of the eight frames 0, 5, ..., 35, all eight in every iteration; frame 3 is held out.  One iteration is
   ``field.sh_lookup`` (forward: the lookup kernel of ``nrnerf_sh_volume_render``; backward: ``nrnerf_grid_lookup_backward`` +
   ``nrnerf_sh_lookup_backward``; a sample's direction from the differences of the bent points) + the compositing kernels of the training
   step + torch's Adam.  PSNR of both sets at 0 / 60 / 120 / 240 iterations, and the median time of an iteration (host clock around a
   synchronise).
B. The backward call by itself.  Straight samples ``o + d z`` of frame 3's camera (1024 rays x 192 and 512 x 384 rays x 192) through the box of
   the series, degrees 1 and 2, 128^3 coefficients in float32 and half: medians of device-event timings of ``nrnerf_sh_lookup_backward`` under
   the RAY rule with all three outputs (d_sh accumulating into a zeroed buffer) and with each output alone, all three under DIFFERENCES, next
   to the float32 backward of the same function composed from ``torch.nn.functional.grid_sample`` (``align_corners=True``, trilinear, zeros
   padding) on the 12 L-channel grid plus ``field.sh_basis`` (the gradients of grid, input and directions, timed as ``torch.autograd.grad`` on
   a graph built outside the window).
C. The lane mappings of the scatter kernel.  ``--lanes DIR``: the libraries ``DIR/libnrnerf_sh_grad_l{8,16,32,64}.so`` -- nrnerf_sh_grad.hip built
   with ``-DNRN_SH_SCATTER_LANES=8 / 16 / 32 / 64`` (degree 1 takes at most 32) and linked with nrnerf_sh_grad_api.o alone (``--build-lanes`` builds them there first) -- are
   loaded side by side and d_sh alone is timed through each on the inputs of B, medians of 10.
    python tools/refine_sh_bake_bench.py [iterations] [repeats] [--lanes DIR] [--build-lanes]          (defaults 240, 10)
One JSON line per measurement.  The script has no time limit of its own: run it under one, ``timeout -k 10 900 python
tools/refine_sh_bake_bench.py``."""
import ctypes as C
import json
import os
import statistics
import subprocess
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
TRAIN_FRAMES, HELD_OUT, WIDTH, SAMPLES, VOLUME, DEGREE, LR = tuple(range(0, 40, 5)), 3, 48, 192, 128, 2, 2e-2
REPORT_AT = (0, 60, 120, 240)
LANES = (8, 16, 32, 64)


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
    net = ck.network_fine if ck.network_fine is not None else ck.network_fn
    model = R.get_model(net, None, precision="f32", device=dev)
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
                    out = R.batchify_rays(r, {"ray_bending_latents": code.expand(n, -1)}, network_fn=net, network_fine=None,
                                          N_samples=SAMPLES, N_importance=0)
                    zz, pts = F.sample_rays(r, SAMPLES)
                    rays.append(r), zs.append(zz), target.append(out["rgb_map"])
                    p4.append(model.bend_points(pts, code.expand(n, -1).contiguous()))
                sets[name] = tuple(torch.cat(t, 0).contiguous() for t in (rays, p4, zs, target))
        lo, hi = BOX
        bake = F.bake({"network_fn": net}, None, lo, hi, VOLUME, precision="f32", sh_degree=DEGREE)
    finally:
        R.set_precision("bf16")
    raw = bake["raw"].detach().clone().requires_grad_(True)
    sh = bake["sh"].detach().clone().requires_grad_(True)
    rec = dict(bake, raw=raw, sh=sh)

    def render(name):
        rays, p4, zs, _ = sets[name]
        logits = F.sh_lookup(rec, p4[..., :3])
        return _Composite.apply(logits, rays, zs, None, False, 0, None)[0]

    def report(it):
        with torch.no_grad():
            row = {name: round(psnr(render(name), sets[name][3]), 2) for name in sets}
        print(json.dumps(dict(what="sh refinement series", volume=VOLUME, degree=DEGREE, iterations=it, lr=LR,
                              rays_per_iteration=int(sets["train"][0].shape[0]), samples=SAMPLES, psnr_held_out_db=row["held_out"],
                              psnr_train_db=row["train"])), flush=True)

    opt = torch.optim.Adam([raw, sh], lr=LR)
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
        print(json.dumps(dict(what="sh refinement iteration", ms_median=round(statistics.median(times[3:] or times), 3),
                              ms_min=round(min(times), 3), iterations=len(times))), flush=True)


def backward_call(lib, sh, degree, lo, hi, rays, p4, cot, mode, d_sh, d_points, d_dirs):
    a = _lib.ShLookupBackwardArgs()
    a.struct_size = C.sizeof(a)
    a.n_rays, a.n_samples = int(p4.shape[0]), int(p4.shape[1])
    a.rays, a.ray_stride = rays.data_ptr(), int(rays.shape[1])
    a.points4, a.direction_mode = p4.data_ptr(), mode
    a.sh, a.sh_dtype, a.sh_degree = sh.data_ptr(), _lib.VOLUME_F16 if sh.dtype == torch.float16 else _lib.VOLUME_F32, degree
    a.g[:] = (sh.shape[2], sh.shape[1], sh.shape[0])
    a.min_point[:], a.max_point[:] = lo, hi
    a.g_raw = cot.data_ptr()
    a.d_sh = None if d_sh is None else d_sh.data_ptr()
    a.d_points = None if d_points is None else d_points.data_ptr()
    a.d_dirs = None if d_dirs is None else d_dirs.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream(sh.device).cuda_stream)
    return lambda: _lib.check(lib.nrnerf_sh_lookup_backward(C.byref(a), stream), "nrnerf_sh_lookup_backward")


def lane_library(directory, lanes, build):
    path = os.path.join(directory, f"libnrnerf_sh_grad_l{lanes}.so")
    if build and not os.path.exists(path):
        csrc = os.path.join(REPO, "nonrigid_nerf_amd", "csrc")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        flags = ["-O3", "-std=c++17", "-fPIC", f"-I{REPO}/include", f"-I{csrc}", "--offload-arch=gfx950", "-Wno-unused-result"]
        os.makedirs(directory, exist_ok=True)
        subprocess.run([hipcc] + flags + [f"-DNRN_SH_SCATTER_LANES={lanes}", "-shared", os.path.join(csrc, "nrnerf_sh_grad.hip"), "-x", "hip",
                                          os.path.join(csrc, "nrnerf_sh_grad_api.cpp"), "-o", path], check=True)
    lib = C.CDLL(path)
    lib.nrnerf_sh_lookup_backward.restype = C.c_int
    lib.nrnerf_sh_lookup_backward.argtypes = [C.POINTER(_lib.ShLookupBackwardArgs), C.c_void_p]
    return lib


def backward_timings(z, dev, repeats, lane_dir, build_lanes):
    near, far = float(z["bds"].min()) * 0.9, float(z["bds"].max())
    full = generate_rays(torch.from_numpy(z["poses"][HELD_OUT]), camera(z, 512), near, far, False, dev)
    pick = torch.randperm(int(full.shape[0]), generator=torch.Generator().manual_seed(0))[:1024].to(dev)
    lo, hi = BOX
    lo_t, hi_t = torch.tensor(lo, device=dev), torch.tensor(hi, device=dev)
    lane_libs = {lanes: lane_library(lane_dir, lanes, build_lanes) for lanes in LANES} if lane_dir else {}
    lib = _lib.load()
    DIFF, RAY = _lib.SH_DIRECTION_DIFFERENCES, _lib.SH_DIRECTION_RAY
    for rays in (full[pick].contiguous(), full):
        with torch.no_grad():
            _, pts = F.sample_rays(rays, SAMPLES)
        n, s = int(pts.shape[0]), int(pts.shape[1])
        m = n * s
        inside = float(((pts >= lo_t) & (pts <= hi_t)).all(-1).float().mean())
        p4 = torch.cat([pts, torch.zeros_like(pts[..., :1])], -1).contiguous()
        cot = torch.randn(n, s, 4, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        dirs = (rays[:, 3:6] / rays[:, 3:6].norm(dim=-1, keepdim=True))[:, None].expand(n, s, 3).reshape(m, 3).contiguous()
        norm = ((pts.reshape(m, 3) - lo_t) / (hi_t - lo_t) * 2 - 1).reshape(1, 1, 1, m, 3)       # grid_sample's coordinates: (x, y, z) in -1 .. 1
        for degree in (1, 2):
            ch, k1 = 12 * degree, (degree + 1) ** 2 - 1
            base = torch.randn(VOLUME, VOLUME, VOLUME, ch, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
            for dtype in (torch.float32, torch.float16):
                sh = base.to(dtype)
                d_sh = torch.zeros(sh.shape, dtype=torch.float32, device=dev)
                d_points, d_dirs = torch.empty(n, s, 3, device=dev), torch.empty(n, s, 3, device=dev)
                call = lambda mode, *outs, use=lib: backward_call(use, sh, degree, lo, hi, rays, p4, cot, mode, *outs)
                row = dict(what="sh lookup backward", samples=m, inside_share=round(inside, 3), grid=VOLUME, degree=degree,
                           sh_dtype=str(dtype).replace("torch.", ""), repeats=repeats)
                row["ray_all_ms"], row["ray_all_min_ms"] = event_ms(call(RAY, d_sh, d_points, d_dirs), repeats)
                row["ray_d_sh_ms"] = event_ms(call(RAY, d_sh, None, None), repeats)[0]
                row["ray_d_points_ms"] = event_ms(call(RAY, None, d_points, None), repeats)[0]
                row["ray_d_dirs_ms"] = event_ms(call(RAY, None, None, d_dirs), repeats)[0]
                row["differences_all_ms"] = event_ms(call(DIFF, d_sh, d_points, d_dirs), repeats)[0]
                row["differences_d_points_d_dirs_ms"] = event_ms(call(DIFF, None, d_points, d_dirs), repeats)[0]
                added = m * inside * 8 * 3 * k1 * 4
                row["d_sh_added_tb_per_s"] = round(added / (row["ray_d_sh_ms"] * 1e-3) / 1e12, 3)
                for lanes, other in lane_libs.items():
                    ms = event_ms(call(RAY, d_sh, None, None, use=other), repeats)
                    row[f"d_sh_lanes_{lanes}_ms"], row[f"d_sh_lanes_{lanes}_tb_per_s"] = ms[0], round(added / (ms[0] * 1e-3) / 1e12, 3)
                del d_sh, d_points, d_dirs
                if dtype == torch.float32:
                    # the same gradients through autograd: grid_sample on a channels-first copy of the coefficients, then the colour sum
                    held = {}
                    vol5 = sh.permute(3, 0, 1, 2)[None].contiguous()
                    cot3 = cot.reshape(m, 4)[:, :3].contiguous()

                    def torch_graph():
                        g, p, d = vol5.detach().requires_grad_(True), norm.detach().requires_grad_(True), dirs.detach().requires_grad_(True)
                        v = torch.nn.functional.grid_sample(g, p, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(ch, m)
                        Y = F.sh_basis(d, degree)
                        held["torch"] = ((Y[:, 1:, None] * v[:3 * k1].t().reshape(m, k1, 3)).sum(1), g, p, d)

                    def torch_backward():
                        v, g, p, d = held["torch"]
                        torch.autograd.grad(v, (g, p, d), cot3)

                    theirs = event_ms(torch_backward, repeats, before=torch_graph)
                    held.clear()
                    del vol5, cot3
                    row.update(grid_sample_backward_ms=theirs[0], grid_sample_backward_min_ms=theirs[1],
                               grid_sample_over_entry_point=round(theirs[0] / row["ray_all_ms"], 2))
                print(json.dumps(row), flush=True)
                del sh
                torch.cuda.empty_cache()
            del base


def main():
    argv = list(sys.argv[1:])
    build_lanes = "--build-lanes" in argv
    if build_lanes:
        argv.remove("--build-lanes")
    lane_dir = None
    if "--lanes" in argv:
        at = argv.index("--lanes")
        lane_dir = argv[at + 1]
        del argv[at:at + 2]
    iterations = int(argv[0]) if len(argv) > 0 else 240
    repeats = int(argv[1]) if len(argv) > 1 else 10
    dev = torch.device("cuda:0")
    gold = os.path.join(REPO, "tests", "golden")
    z = np.load(os.path.join(gold, "example_sequence_96x72.npz"))
    if iterations > 0:
        ck = load_checkpoint(os.path.join(gold, "fitted_config4.tar"), N_samples=64, N_importance=128, device=dev)
        for m in (ck.ray_bender, ck.network_fn, ck.network_fine):
            if m is not None:
                m.requires_grad_(False)
        refinement_series(ck, z, dev, iterations)
        del ck
        torch.cuda.empty_cache()
    if repeats > 0:
        backward_timings(z, dev, repeats, lane_dir, build_lanes)


if __name__ == "__main__":
    main()
