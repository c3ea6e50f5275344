"""Baked warps, the parts that need no GPU: the record layout of nrnerf_warped_volume_render_args, what the entry point answers before its first
HIP call (in the order include/nrnerf.h states), the float64 reference of tests/warp_reference.py itself, and the accuracy series on the
fitted checkpoint -- what a warp grid of 8^3 .. 64^3 costs against the exact bender -- that tests/test_warp.py repeats on the device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd.synthetic import SceneConfig, make_scene
from oracle import nrnerf_oracle as O
from tests import volume_reference as V
from tests import warp_reference as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. record layout ----------------------------------------------------------------------------------------------------------------------------
def _offsets_by_c_program(tmp_path, record, fields, extra=()):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nrnerf.h"\nint main(void) {\n'
                     f'printf("%d %zu\\n", NRNERF_ABI_VERSION, sizeof({record}));\n'
                     + "".join(f'printf("%zu\\n", offsetof({record}, {f}));\n' for f in fields)
                     + "".join(f'printf("%ld\\n", (long)({e}));\n' for e in extra) + 'return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), str(probe), "-o", str(exe)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


def test_warped_volume_render_record_matches_ctypes(tmp_path):
    fields = ["n_rays", "n_samples", "rays", "ray_stride", "lindisp", "z", "volume", "volume_dtype", "g", "min_point", "max_point",
              "warp", "warp_dtype", "warp_g", "warp_min_point", "warp_max_point", "has_rigidity_cutoff", "rigidity_cutoff",
              "has_test_time_scaling", "test_time_scaling", "white_bkgd", "has_removal_threshold", "removal_threshold", "rgb", "disp", "acc",
              "raw", "weights", "alpha", "surface_pts", "surface_rigidity", "median_index", "points4"]
    WA = _lib.WarpedVolumeRenderArgs
    assert ["struct_size"] + fields == [f[0] for f in WA._fields_]
    got = _offsets_by_c_program(tmp_path, "nrnerf_warped_volume_render_args", fields,
                                ("NRNERF_VOLUME_F32", "NRNERF_VOLUME_F16", "NRNERF_MAX_SAMPLES", "sizeof(nrnerf_volume_render_args)"))
    assert got == [_lib.ABI_VERSION, C.sizeof(WA)] + [getattr(WA, f).offset for f in fields] + [_lib.VOLUME_F32, _lib.VOLUME_F16, _lib.MAX_SAMPLES,
                                                                                                 C.sizeof(_lib.VolumeRenderArgs)]
    assert _lib.ABI_VERSION == 10
    assert C.sizeof(WA) != C.sizeof(_lib.VolumeRenderArgs)          # (a record of the other call is told apart by its struct_size)


# ---- 2. status table: what the entry point answers before its first HIP call ---------------------------------------------------------------------
OK, INVALID, UNSUPPORTED = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
_HOST = (C.c_char * 4096)()
H = (C.addressof(_HOST) + 255) & ~255      # a non-null pointer, never dereferenced by these cases
STREAM = C.c_void_p(0)
_ARRAYS = ("g", "min_point", "max_point", "warp_g", "warp_min_point", "warp_max_point")


def warp_args(**kw):
    a = _lib.WarpedVolumeRenderArgs()
    a.struct_size = C.sizeof(_lib.WarpedVolumeRenderArgs)
    a.n_rays, a.n_samples, a.ray_stride = 3, 5, 8
    a.rays, a.volume, a.volume_dtype, a.warp, a.warp_dtype = H, H, _lib.VOLUME_F32, H, _lib.VOLUME_F32
    a.g[:], a.warp_g[:] = (4, 3, 2), (3, 2, 5)
    a.min_point[:], a.max_point[:] = (-1.0, -1.0, -1.0), (1.0, 2.0, 3.0)
    a.warp_min_point[:], a.warp_max_point[:] = (-2.0, 0.0, -1.0), (0.5, 2.5, 1.0)
    a.rgb, a.disp, a.acc = H, H, H
    for k, v in kw.items():
        if k in _ARRAYS:
            getattr(a, k)[:] = v
        else:
            setattr(a, k, v)
    return a


ZERO = dict(n_rays=0)      # a valid record answers OK here, so INVALID next to it is the named check's
NAN = float("nan")
NO_MAPS = dict(rgb=None, disp=None, acc=None)
WARP_TABLE = [
    ("null args", None, INVALID),
    ("zero rays", ZERO, OK),
    ("zero rays, null pointers", dict(ZERO, rays=None, volume=None, warp=None, rgb=None, disp=None, acc=None), OK),
    ("struct_size 0", dict(ZERO, struct_size=0), INVALID),
    ("struct_size of nrnerf_volume_render_args", dict(ZERO, struct_size=C.sizeof(_lib.VolumeRenderArgs)), INVALID),
    ("struct_size of another record", dict(ZERO, struct_size=C.sizeof(_lib.WarpedVolumeRenderArgs) - 8), INVALID),
    ("negative rays", dict(n_rays=-1), INVALID),
    ("n_samples 0", dict(ZERO, n_samples=0), INVALID),
    ("n_samples 1", dict(ZERO, n_samples=1), OK),
    ("n_samples NRNERF_MAX_SAMPLES", dict(ZERO, n_samples=_lib.MAX_SAMPLES), OK),
    ("n_samples beyond NRNERF_MAX_SAMPLES", dict(ZERO, n_samples=_lib.MAX_SAMPLES + 1), INVALID),
    ("ray_stride 7", dict(ZERO, ray_stride=7), INVALID),
    ("ray_stride 11", dict(ZERO, ray_stride=11), OK),
    ("gx 1", dict(ZERO, g=(1, 3, 2)), INVALID),
    ("gz 0", dict(ZERO, g=(4, 3, 0)), INVALID),
    ("the smallest grids", dict(ZERO, g=(2, 2, 2), warp_g=(2, 2, 2)), OK),
    ("max == min on x", dict(ZERO, max_point=(-1.0, 2.0, 3.0)), INVALID),
    ("NaN min", dict(ZERO, min_point=(-1.0, NAN, -1.0)), INVALID),
    ("unknown volume dtype", dict(ZERO, volume_dtype=2), INVALID),
    ("half volume", dict(ZERO, volume_dtype=_lib.VOLUME_F16), OK),
    ("warp gx 1", dict(ZERO, warp_g=(1, 2, 5)), INVALID),
    ("warp gy 1", dict(ZERO, warp_g=(3, 1, 5)), INVALID),
    ("warp gz -1", dict(ZERO, warp_g=(3, 2, -1)), INVALID),
    ("warp max == min on y", dict(ZERO, warp_max_point=(0.5, 0.0, 1.0)), INVALID),
    ("warp max < min on z", dict(ZERO, warp_max_point=(0.5, 2.5, -3.0)), INVALID),
    ("warp NaN min", dict(ZERO, warp_min_point=(NAN, 0.0, -1.0)), INVALID),
    ("warp NaN max", dict(ZERO, warp_max_point=(0.5, 2.5, NAN)), INVALID),
    ("unknown warp dtype", dict(ZERO, warp_dtype=2), INVALID),
    ("negative warp dtype", dict(ZERO, warp_dtype=-1), INVALID),
    ("half warp", dict(ZERO, warp_dtype=_lib.VOLUME_F16), OK),
    ("both half", dict(ZERO, warp_dtype=_lib.VOLUME_F16, volume_dtype=_lib.VOLUME_F16), OK),
    ("2^30 vertices in both", dict(ZERO, g=(1024, 1024, 1024), warp_g=(1024, 1024, 1024)), OK),
    ("volume beyond 2^30 vertices", dict(ZERO, g=(1024, 1024, 1025)), UNSUPPORTED),
    ("warp beyond 2^30 vertices", dict(ZERO, warp_g=(1025, 1024, 1024)), UNSUPPORTED),
    ("warp far beyond 2^30 vertices", dict(ZERO, warp_g=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), UNSUPPORTED),
    ("a bad warp grid comes before a volume that is too large", dict(ZERO, g=(1024, 1024, 1025), warp_g=(1, 2, 5)), INVALID),
    ("2^31 samples", dict(n_rays=2 ** 21, n_samples=1024), UNSUPPORTED),
    ("null rays", dict(rays=None), INVALID),
    ("null volume", dict(volume=None), INVALID),
    ("null warp", dict(warp=None), INVALID),
    ("rgb without disp", dict(disp=None), INVALID),
    ("acc alone", dict(rgb=None, disp=None), INVALID),
    ("nothing to write", NO_MAPS, INVALID),
    ("weights without the maps", dict(NO_MAPS, raw=H, weights=H), INVALID),
    ("alpha without the maps", dict(NO_MAPS, points4=H, alpha=H), INVALID),
    ("surface_pts without the maps", dict(NO_MAPS, raw=H, surface_pts=H), INVALID),
    ("surface_rigidity without the maps", dict(NO_MAPS, raw=H, points4=H, surface_rigidity=H), INVALID),
    ("median_index without the maps", dict(NO_MAPS, points4=H, median_index=H), INVALID),
]


@pytest.mark.parametrize("case,kw,want", WARP_TABLE, ids=[c[0] for c in WARP_TABLE])
def test_warped_volume_render_status_table(case, kw, want):
    lib = _lib.load()
    args = None if kw is None else C.byref(warp_args(**kw))
    assert lib.nrnerf_warped_volume_render(args, STREAM) == want


@pytest.mark.parametrize("kw", [dict(), dict(NO_MAPS, raw=H), dict(NO_MAPS, points4=H), dict(surface_pts=H, has_removal_threshold=1)],
                         ids=["maps", "raw alone", "points4 alone", "surface and removal need no input points"])
def test_a_record_that_passes_every_host_check_is_stopped_by_the_device_check(kw):
    """Host memory as the output: every check that needs no HIP call has passed when the ownership check answers INVALID (without a device,
    too: the query itself fails)."""
    assert _lib.load().nrnerf_warped_volume_render(C.byref(warp_args(**kw)), STREAM) == INVALID


# ---- 3. the reference itself ---------------------------------------------------------------------------------------------------------------------
LO, HI = (-0.5, 0.25, 1.0), (1.5, 1.0, 4.0)                 # the volume's box (tests/test_volume.py)
WLO, WHI = (-0.1, 0.4, 0.5), (1.1, 1.3, 3.2)                # the warp's: partly overlapping


def some_rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.5, 0.6, 0.0]) + 0.05 * torch.randn(n, 3, generator=g)
    d = torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(n, 3, generator=g)
    return torch.cat([o, d, torch.full((n, 1), 0.5), torch.full((n, 1), 5.0)], -1)


def same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_a_zero_warp_or_scaling_zero_is_the_straight_render():
    vol, warp = V.smooth_volume(9, 8, 7, seed=2), W.smooth_warp(5, 4, 3, seed=1)
    rays = some_rays(11, 5)
    z = V.coarse_depths(rays, 33)
    straight = V.render_reference(vol, LO, HI, rays, z, white_bkgd=True)
    for w, kw in ((torch.zeros_like(warp), {}), (warp, dict(test_time_scaling=0.0))):
        got = W.render_reference(vol, LO, HI, w, WLO, WHI, rays, z, white_bkgd=True, **kw)
        assert torch.equal(got["points4"][..., :3], got["points"])
        for k in ("rgb_map", "disp_map", "acc_map", "raw", "weights", "alpha", "median_index"):
            assert same(got[k], straight[k]), k
    moved = W.render_reference(vol, LO, HI, warp, WLO, WHI, rays, z, white_bkgd=True)
    assert not torch.equal(moved["raw"], straight["raw"]) and float(straight["acc_map"].max()) > 0.5


def test_a_point_on_a_warp_vertex_is_moved_by_the_stored_values():
    g = (5, 4, 3)
    warp = W.smooth_warp(*g, seed=3)
    lo, hi = (0.0, 0.0, 0.0), (g[0] - 1.0, g[1] - 1.0, g[2] - 1.0)                # unit spacing: a vertex IS its index
    verts = W.grid_vertices(lo, hi, g)
    for dtype in (torch.float64, torch.float32):
        w = warp.to(dtype)
        for store in (warp, warp.half()):
            ws = store.to(dtype)
            got = W.bend_reference(store, lo, hi, verts, dtype=dtype)
            assert torch.equal(got[..., :3], verts.to(dtype) + ws[..., 3:] * ws[..., :3]) and torch.equal(got[..., 3], ws[..., 3])
        got = W.bend_reference(warp, lo, hi, verts, test_time_scaling=1.5, rigidity_cutoff=0.5, dtype=dtype)
        m = torch.where(w[..., 3:] <= 0.5, torch.zeros_like(w[..., 3:]), w[..., 3:])
        assert torch.equal(got[..., :3], verts.to(dtype) + m * w[..., :3] * 1.5) and torch.equal(got[..., 3:], m)
    # outside the warp, or NaN: not bent, rigidity 0
    out = torch.tensor([[-0.01, 1.0, 1.0], [1.0, g[1] - 1 + 0.01, 1.0], [NAN, 1.0, 1.0], [float("inf"), 1.0, 1.0]])
    got = W.bend_reference(warp, lo, hi, out)
    assert same(got[..., :3], out.double()) and not bool(got[..., 3].any())


def test_cutoff_scaling_and_removal_are_the_benders_on_a_tiny_module():
    """A warp that holds a small bender's values at its vertices: at the vertices the rule with the knobs on is the oracle's bender with the
    same knobs (rnh:563-570), and the removal knob zeroes the sigma logits where the oracle's mask is at or above the threshold (rnh:308-311)."""
    cfg = SceneConfig(N_importance=0, bend_depth=5)
    scene = make_scene(cfg, 3)
    code = torch.randn(1, cfg.latent_size, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    g = (6, 5, 4)
    lo, hi = (0.0, 0.0, 0.0), (g[0] - 1.0, g[1] - 1.0, g[2] - 1.0)
    warp = W.bake_warp_reference(scene, code, g, lo, hi)                            # float64: the stored values ARE the bender's
    verts = W.grid_vertices(lo, hi, g).reshape(-1, 3)
    lat = code.expand(verts.shape[0], -1)
    mask = O.bend_points(verts, lat, scene.bender)[1]["rigidity_mask"][:, 0]
    cut, thr = float(np.float32(mask.median())), float(np.float32(mask.quantile(0.75)))      # (the record carries the knobs as float32)
    for knobs in (O.Knobs(), O.Knobs(rigidity_test_time_cutoff=cut), O.Knobs(test_time_scaling=2.5), O.Knobs(cut, 0.25)):
        bent, det = O.bend_points(verts, lat, scene.bender, knobs)
        got = W.bend_reference(warp, lo, hi, verts, rigidity_cutoff=knobs.rigidity_test_time_cutoff, test_time_scaling=knobs.test_time_scaling)
        assert torch.equal(got[:, :3], bent) and torch.equal(got[:, 3:], det["rigidity_mask"])
        if knobs.rigidity_test_time_cutoff is not None:
            frozen = mask <= cut
            assert bool(frozen.any()) and bool((~frozen).any()) and torch.equal(got[frozen, :3], verts[frozen]) and not bool(got[frozen, 3].any())
    # removal: rays along the grid's x-rows, one sample per vertex (o = (0, iy, iz), d = +x, z = ix)
    gx, gy, gz = g
    iz, iy = torch.meshgrid(torch.arange(gz, dtype=torch.float64), torch.arange(gy, dtype=torch.float64), indexing="ij")
    n = gy * gz
    rays = torch.cat([torch.zeros(n, 1, dtype=torch.float64), iy.reshape(n, 1), iz.reshape(n, 1), torch.ones(n, 1, dtype=torch.float64),
                      torch.zeros(n, 2, dtype=torch.float64), torch.zeros(n, 1, dtype=torch.float64), torch.full((n, 1), gx - 1.0, dtype=torch.float64)], -1)
    z = torch.arange(gx, dtype=torch.float64).expand(n, gx)
    vol = V.smooth_volume(7, 6, 5, seed=1)
    vlo, vhi = (-1.0, -1.0, -1.0), (6.0, 5.0, 4.0)
    kept = W.render_reference(vol, vlo, vhi, warp, lo, hi, rays, z)
    gone = W.render_reference(vol, vlo, vhi, warp, lo, hi, rays, z, removal_threshold=thr)
    assert torch.equal(kept["points"].reshape(-1, 3), verts)
    kill = (mask >= float(np.float32(thr))).reshape(n, gx)
    assert bool(kill.any()) and bool((~kill).any())
    assert bool((gone["raw"][..., 3][kill] == 0).all()) and torch.equal(gone["raw"][..., 3][~kill], kept["raw"][..., 3][~kill])
    assert torch.equal(gone["raw"][..., :3], kept["raw"][..., :3]) and torch.equal(gone["points4"], kept["points4"])


# ---- 4. the accuracy series on the fitted checkpoint, in float64 -----------------------------------------------------------------------------------
# PSNR of rgb_map rendered through a warp grid of 8^3 / 16^3 / 32^3 / 64^3 against the render whose samples the oracle's bender bent exactly,
# both on the float64 canonical bake at 96^3 (fitted_latest, frame 3, 48 x 36 rays, 192 samples): measured here, asserted to 0.01 dB, repeated on
# the device by tests/test_warp.py and quoted in DESIGN.md section 3.14
SERIES_PSNR = {8: 30.036, 16: 34.005, 32: 42.382, 64: 51.156}
_series = {}


def series_reference():
    """``{resolution: (psnr rgb_map, psnr acc_map, max |bent - exact bent|)}``; computed once and shared."""
    if not _series:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
        ck, scene, rays, code = V.series_setup()
        n = rays.shape[0]
        with torch.no_grad():
            z = V.coarse_depths(rays, V.SERIES_SAMPLES)
            pts = W.sample_points(rays, z)
            bent, det = O.bend_points(pts.reshape(-1, 3), code.double().expand(n * V.SERIES_SAMPLES, -1), scene.bender)
            p4 = torch.cat([bent, det["rigidity_mask"]], -1).reshape(n, -1, 4)
            vol = V.bake_reference(scene, W.SERIES_VOLUME)
            exact = V.render_reference(vol, V.SERIES_BOX[0], V.SERIES_BOX[1], rays, z, p4)
            inside = ((pts >= torch.tensor(W.SERIES_WARP_BOX[0], dtype=torch.float64)) & (pts <= torch.tensor(W.SERIES_WARP_BOX[1], dtype=torch.float64))).all(-1)
            for res in W.SERIES_WARPS:
                warp = W.bake_warp_reference(scene, code, res)
                out = W.render_reference(vol, V.SERIES_BOX[0], V.SERIES_BOX[1], warp, W.SERIES_WARP_BOX[0], W.SERIES_WARP_BOX[1], rays, z)
                gap = float((out["points4"][..., :3] - p4[..., :3])[inside].abs().max())
                _series[res] = (V.psnr(out["rgb_map"], exact["rgb_map"]), V.psnr(out["acc_map"], exact["acc_map"]), gap)
    return _series


def test_accuracy_series_of_the_warp_grid_in_float64():
    s = series_reference()
    print(f"[fitted_latest, frame {V.SERIES_FRAME}, {V.SERIES_WIDTH} wide, S {V.SERIES_SAMPLES}, canonical bake {W.SERIES_VOLUME}^3 float64]")
    for res in W.SERIES_WARPS:
        print(f"  warp {res}^3: PSNR rgb_map {s[res][0]:.3f} dB, acc_map {s[res][1]:.3f} dB against the exactly bent render; "
              f"largest displacement error inside the warp's box {s[res][2]:.3e}")
    for res in W.SERIES_WARPS:
        assert abs(s[res][0] - SERIES_PSNR[res]) <= 0.01, (res, s[res][0])


# ---- 5. the code object ----------------------------------------------------------------------------------------------------------------------------
BUILD = os.path.join(REPO, "nonrigid_nerf_amd", "csrc", "build")


def warp_kernel_resources():
    """``{(kind, EPL, volume half, warp half): resources}`` of the kernels of nrnerf_warp.o, from the code object's metadata; None: not built."""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_isa
    obj = os.path.join(BUILD, "nrnerf_warp.o")
    if not os.path.exists(obj):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        co = check_isa.device_code_object(obj, tmp)
        assert co is not None
        notes = subprocess.run([f"{check_isa.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    seen = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or "warped_" not in name.group(1):
            continue
        num = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
        kind = re.search(r"warped_(render|lookup)_kernelI(?:Li(\d+)E)?Lb([01])ELb([01])E", name.group(1))
        assert kind is not None, name.group(1)
        seen[(kind.group(1), int(kind.group(2) or 0), int(kind.group(3)), int(kind.group(4)))] = dict(
            vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), vgpr_spill=num("vgpr_spill_count"), scratch=num("private_segment_fixed_size"))
    return seen


@pytest.mark.skipif(not os.path.isdir(BUILD) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="no build directory / no llvm-readelf")
def test_warp_kernels_use_no_scratch():
    seen = warp_kernel_resources()
    if seen is None:
        pytest.skip("csrc/build/nrnerf_warp.o not built")
    for key in sorted(seen):
        print(key, seen[key])
    halves = [(v, w) for v in (0, 1) for w in (0, 1)]
    assert sorted(seen) == sorted([("render", e, v, w) for e in (1, 2, 3, 4, 6, 8, 12, 16) for v, w in halves] + [("lookup", 0, v, w) for v, w in halves])
    for key, r in seen.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (key, r)
        assert r["vgpr"] <= 256, (key, r)          # (within the architectural VGPRs: nothing is parked in AGPRs either)
