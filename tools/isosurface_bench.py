#!/usr/bin/env python
"""Throughput of the iso-surface extraction (``nrnerf_isosurface_count`` + ``_emit``) on the density of the fitted checkpoint
(tests/golden/fitted_latest.tar, bf16 ``sample_grid``), for a 128^3 and a 256^3 grid: cells/s, the achieved bytes/s against the passes'
BY-DESIGN bytes, and -- beside it -- the time of copying the same volume to the host, which any host extractor pays before it starts.
    python tools/isosurface_bench.py [repeats] [grid ...]          (defaults 20, 128 256)

By-design bytes of a grid of n vertices (nb = ceil(n / 256) blocks) and a mesh of V vertices, T triangles:
    count  4 n (each value once from memory; its seven re-reads are cache hits by design) + 1 n (corner byte) + 4 n (offset word) + 8 nb (sums)
    scan   8 nb read + 16 nb written
    emit   1 n + 4 n (corner byte, offset word) + 16 nb (bases) + V (12 + 12) (positions, normals) + 12 T (faces)
           (the reads behind an active edge or a crossed cell -- two values and two gradients per vertex, 5 bytes + a base per face index -- scale
           with the surface, not the volume, and are left out: they are the reason "achieved" sits below the memory rate on a dense surface)
One JSON line per grid; times are medians over the repeats of each call alone on the stream, by device events."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nonrigid_nerf_amd import _lib, field as F  # noqa: E402
from nonrigid_nerf_amd.checkpoint import load_checkpoint  # noqa: E402


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


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    grids = [int(v) for v in sys.argv[2:]] or [128, 256]
    dev = torch.device("cuda:0")
    gold = os.path.join(REPO, "tests", "golden")
    ck = load_checkpoint(os.path.join(gold, "fitted_latest.tar"), N_samples=64, N_importance=128, device=dev)
    far = float(np.load(os.path.join(gold, "example_sequence_96x72.npz"))["bds"].max())
    lo, hi = np.full(3, -0.5 * far, dtype=np.float32), np.full(3, 0.5 * far, dtype=np.float32)
    lib = _lib.load()
    for g in grids:
        with torch.no_grad():
            sigma = F.sample_grid(ck.render_kwargs_test, ck.latents[3], lo, hi, g, fine=True, precision="bf16")["sigma"]
        positive = sigma[sigma > 0]
        level = float(positive.median()) if positive.numel() else 0.5
        n, nb = g ** 3, (g ** 3 + _lib.ISO_BLOCK - 1) // _lib.ISO_BLOCK
        a = _lib.IsosurfaceArgs()
        a.struct_size = C.sizeof(_lib.IsosurfaceArgs)
        a.value, a.gx, a.gy, a.gz, a.level = sigma.data_ptr(), g, g, g, level
        a.min_point[:], a.max_point[:] = lo.tolist(), hi.tolist()
        need = lib.nrnerf_isosurface_workspace_bytes(g, g, g)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        a.workspace, a.workspace_bytes, a.totals = ws.data_ptr(), need, totals.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        count = lambda: _lib.check(lib.nrnerf_isosurface_count(C.byref(a), stream), "count")
        count_ms, count_min = event_ms(count, repeats)
        n_v, n_t = totals.tolist()
        verts = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
        norms = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((n_t, 3), dtype=torch.int32, device=dev)
        a.vertices, a.normals, a.faces, a.n_vertices, a.n_triangles = verts.data_ptr() or None, norms.data_ptr() or None, faces.data_ptr() or None, n_v, n_t
        emit = lambda: _lib.check(lib.nrnerf_isosurface_emit(C.byref(a), stream), "emit")
        emit_ms, emit_min = event_ms(emit, repeats)
        whole_ms, _ = event_ms(lambda: F.isosurface(sigma, level, lo, hi), max(3, repeats // 4))      # with the host read and the allocations
        pinned = torch.empty(sigma.shape, dtype=torch.float32, pin_memory=True)
        copy_ms, _ = event_ms(lambda: pinned.copy_(sigma, non_blocking=True), max(3, repeats // 4))
        pageable_ms, _ = event_ms(lambda: sigma.cpu(), max(3, repeats // 4))
        count_bytes = 4 * n + n + 4 * n + 8 * nb + 8 * nb + 16 * nb
        emit_bytes = n + 4 * n + 16 * nb + 24 * n_v + 12 * n_t
        cells = (g - 1) ** 3
        print(json.dumps(dict(grid=g, level=round(level, 4), vertices=n_v, triangles=n_t,
                              count_ms=round(count_ms, 4), count_min_ms=round(count_min, 4), emit_ms=round(emit_ms, 4), emit_min_ms=round(emit_min, 4),
                              cells_per_s=cells / ((count_ms + emit_ms) * 1e-3),
                              count_design_bytes=count_bytes, count_design_bytes_per_s=count_bytes / (count_ms * 1e-3),
                              emit_design_bytes=emit_bytes, emit_design_bytes_per_s=emit_bytes / (emit_ms * 1e-3),
                              isosurface_call_ms=round(whole_ms, 4),
                              volume_to_pinned_host_ms=round(copy_ms, 4), volume_to_pageable_host_ms=round(pageable_ms, 4),
                              volume_bytes=4 * n)))


if __name__ == "__main__":
    main()
