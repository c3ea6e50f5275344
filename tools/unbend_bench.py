#!/usr/bin/env python
"""Throughput of the inverse bender (``field.unbend_points`` -> ``nrnerf_bender_inverse``) on the fitted checkpoint
(tests/golden/fitted_latest.tar, code 3, tol 1e-6, 64 evaluations, omega 1):
    * 2^20 uniform random points in the cube of half the far bound;
    * the vertices of the canonical 128^3 mesh (``extract_mesh(..., with_bending=False)``, level = median of the positive densities);
each with the blocks handed out by the work counter and with fixed shares, next to
    * ONE evaluation of the same points (``max_iters=1``: the cost of the fp32 bender inside the loop), and
    * what a caller could do without the kernel: a Python loop of ``query_points(..., detailed_output=True)`` per iteration at the same
      tolerance, every point evaluated as often as the slowest one, the trunk evaluated as well, one host read per iteration for the vote.
    python tools/unbend_bench.py [repeats]          (default 5)
One JSON line per point set; times are medians over the repeats of each call alone on the stream, by device events -- the same number of
repeats for the kernel and for the loop of launches.  The script has no time limit of its own: run it under one, ``timeout -k 10 600 python
tools/unbend_bench.py``."""
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nonrigid_nerf_amd import _lib, field as F  # noqa: E402
from nonrigid_nerf_amd import render as R  # noqa: E402
from nonrigid_nerf_amd.checkpoint import load_checkpoint  # noqa: E402

TOL, MAX_ITERS, OMEGA = 1e-6, 64, 1.0


def event_ms(fn, repeats):
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


def host_loop(net, c, code):
    """The iteration as a loop of launches: the same updates and stopping rule, all points evaluated until the last one is done."""
    x = c.clone()
    done = torch.zeros(c.shape[0], dtype=torch.bool, device=c.device)
    tol = float(np.float32(TOL))
    evaluations = 0
    for k in range(MAX_ITERS):
        bent = R.query_points(x, net, code, detailed_output=True, precision="f32")[1]["input_pts"]
        evaluations += 1
        d = bent - c
        done = done | (d.abs().max(-1).values <= tol)
        if bool(done.all()) or k == MAX_ITERS - 1:          # the host read
            break
        x = torch.where(done[:, None], x, x - OMEGA * d)
    return x, evaluations


def measure(label, net, pts, code, repeats):
    with torch.no_grad():
        sol = F.unbend_points(net, pts, code, tol=TOL, relaxation=OMEGA, max_iters=MAX_ITERS)
        its = sol["iterations"].float()
        n = int(pts.shape[0])
        pad = (-n) % 32
        per_block = torch.cat([its, its.new_zeros(pad)]).reshape(-1, 32).max(-1).values       # flat points: rows of 64 = two blocks of 32 in order
        dyn_ms, dyn_min = event_ms(lambda: F.unbend_points(net, pts, code, tol=TOL, relaxation=OMEGA, max_iters=MAX_ITERS), repeats)
        fix_ms, fix_min = event_ms(lambda: F.unbend_points(net, pts, code, tol=TOL, relaxation=OMEGA, max_iters=MAX_ITERS, flags=_lib.RENDER_FIXED_SHARES), repeats)
        one_ms, one_min = event_ms(lambda: F.unbend_points(net, pts, code, tol=TOL, relaxation=OMEGA, max_iters=1), repeats)
        _, loop_evals = host_loop(net, pts, code)
        loop_ms, _ = event_ms(lambda: host_loop(net, pts, code), repeats)
    print(json.dumps(dict(points=label, n=n, repeats=repeats, relaxation=OMEGA, converged=float(sol["converged"].float().mean()),
                          evaluations_per_point_mean=float(its.mean()), evaluations_per_point_max=int(its.max()),
                          evaluations_per_block_mean=float(per_block.mean()),
                          dynamic_ms=round(dyn_ms, 4), dynamic_min_ms=round(dyn_min, 4), dynamic_points_per_s=n / (dyn_ms * 1e-3),
                          fixed_ms=round(fix_ms, 4), fixed_min_ms=round(fix_min, 4), fixed_points_per_s=n / (fix_ms * 1e-3),
                          one_evaluation_ms=round(one_ms, 4), one_evaluation_min_ms=round(one_min, 4),
                          ms_per_block_evaluation_sweep=dyn_ms / float(per_block.mean()),
                          host_loop_ms=round(loop_ms, 3), host_loop_evaluations=loop_evals, host_loop_over_kernel=loop_ms / dyn_ms)), flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    gold = os.path.join(REPO, "tests", "golden")
    ck = load_checkpoint(os.path.join(gold, "fitted_latest.tar"), N_samples=64, N_importance=128, device=dev)
    for m in (ck.ray_bender, ck.network_fn, ck.network_fine):
        if m is not None:
            m.requires_grad_(False)
    far = float(np.load(os.path.join(gold, "example_sequence_96x72.npz"))["bds"].max())
    lo, hi = np.full(3, -0.5 * far, dtype=np.float32), np.full(3, 0.5 * far, dtype=np.float32)
    code = ck.latents[3].reshape(1, -1)
    net = ck.network_fine if ck.network_fine is not None else ck.network_fn
    g = torch.Generator().manual_seed(0)
    pts = ((torch.rand(1 << 20, 3, generator=g) * 2 - 1) * (0.5 * far)).to(dev)
    measure("2^20 uniform in the cube of half the far bound", net, pts, code, repeats)
    with torch.no_grad():
        sigma = F.sample_grid(ck.render_kwargs_test, None, lo, hi, 128, fine=True, with_bending=False, precision="bf16")["sigma"]
        positive = sigma[sigma > 0]
        level = float(positive.median()) if positive.numel() else 0.5
        mesh = F.extract_mesh(ck.render_kwargs_test, None, level, lo, hi, 128, fine=True, with_bending=False, colors=False, rigidity=False,
                              precision="bf16")
    measure("vertices of the canonical 128^3 mesh", net, mesh["vertices"].contiguous(), code, repeats)


if __name__ == "__main__":
    main()
