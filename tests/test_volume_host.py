"""Baked volumes, the parts that need no GPU: the record layouts of nrnerf_volume_render_args / nrnerf_bend_points_args, what the two entry
points answer before their first HIP call (in the order include/nrnerf.h states), the float64 reference of tests/volume_reference.py itself,
and the resolution series on the fitted checkpoint that tests/test_volume.py repeats on the device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import _lib
from oracle import nrnerf_oracle as O
from tests import volume_reference as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. record layouts ---------------------------------------------------------------------------------------------------------------------------
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


def test_volume_render_record_matches_ctypes(tmp_path):
    fields = ["n_rays", "n_samples", "rays", "ray_stride", "lindisp", "z", "points4", "volume", "volume_dtype", "g", "min_point", "max_point",
              "white_bkgd", "has_removal_threshold", "removal_threshold", "rgb", "disp", "acc", "raw", "weights", "alpha", "surface_pts",
              "surface_rigidity", "median_index"]
    VA = _lib.VolumeRenderArgs
    assert ["struct_size"] + fields == [f[0] for f in VA._fields_]
    got = _offsets_by_c_program(tmp_path, "nrnerf_volume_render_args", fields, ("NRNERF_VOLUME_F32", "NRNERF_VOLUME_F16", "NRNERF_MAX_SAMPLES"))
    assert got == [_lib.ABI_VERSION, C.sizeof(VA)] + [getattr(VA, f).offset for f in fields] + [_lib.VOLUME_F32, _lib.VOLUME_F16, _lib.MAX_SAMPLES]
    assert _lib.ABI_VERSION == 10


def test_bend_points_record_matches_ctypes(tmp_path):
    fields = ["n_rows", "n_samples", "points", "point_stride", "latent_stride", "latents", "has_rigidity_cutoff", "rigidity_cutoff",
              "has_test_time_scaling", "test_time_scaling", "flags", "bent4", "workspace", "workspace_bytes"]
    BA = _lib.BendPointsArgs
    assert ["struct_size"] + fields == [f[0] for f in BA._fields_]
    got = _offsets_by_c_program(tmp_path, "nrnerf_bend_points_args", fields,
                                ("NRNERF_RENDER_NO_X16 | NRNERF_RENDER_BENDER_32X32 | NRNERF_RENDER_FIXED_SHARES",))
    assert got == [_lib.ABI_VERSION, C.sizeof(BA)] + [getattr(BA, f).offset for f in fields] + [_lib.QUERY_FLAGS]
    assert _lib.ABI_VERSION == 10


# ---- 2. status tables: what the entry points answer before their first HIP call ------------------------------------------------------------------------
OK, INVALID, UNSUPPORTED = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
_HOST = (C.c_char * 4096)()
H = (C.addressof(_HOST) + 255) & ~255      # a non-null pointer, never dereferenced by these cases -- except as a MODEL: zeros, i.e. no ray bender
STREAM = C.c_void_p(0)


def volume_args(**kw):
    a = _lib.VolumeRenderArgs()
    a.struct_size = C.sizeof(_lib.VolumeRenderArgs)
    a.n_rays, a.n_samples, a.ray_stride = 3, 5, 8
    a.rays, a.volume, a.volume_dtype = H, H, _lib.VOLUME_F32
    a.g[:] = (4, 3, 2)
    a.min_point[:], a.max_point[:] = (-1.0, -1.0, -1.0), (1.0, 2.0, 3.0)
    a.rgb, a.disp, a.acc = H, H, H
    for k, v in kw.items():
        if k in ("g", "min_point", "max_point"):
            getattr(a, k)[:] = v
        else:
            setattr(a, k, v)
    return a


ZERO = dict(n_rays=0)      # a valid record answers OK here, so INVALID next to it is the named check's
NAN = float("nan")
VOLUME_TABLE = [
    ("null args", None, INVALID),
    ("zero rays", ZERO, OK),
    ("zero rays, null pointers", dict(ZERO, rays=None, volume=None, rgb=None, disp=None, acc=None), OK),
    ("struct_size 0", dict(ZERO, struct_size=0), INVALID),
    ("struct_size of another record", dict(ZERO, struct_size=C.sizeof(_lib.VolumeRenderArgs) - 8), INVALID),
    ("negative rays", dict(n_rays=-1), INVALID),
    ("n_samples 0", dict(ZERO, n_samples=0), INVALID),
    ("n_samples 1", dict(ZERO, n_samples=1), OK),
    ("n_samples NRNERF_MAX_SAMPLES", dict(ZERO, n_samples=_lib.MAX_SAMPLES), OK),
    ("n_samples beyond NRNERF_MAX_SAMPLES", dict(ZERO, n_samples=_lib.MAX_SAMPLES + 1), INVALID),
    ("ray_stride 7", dict(ZERO, ray_stride=7), INVALID),
    ("ray_stride 11", dict(ZERO, ray_stride=11), OK),
    ("gx 1", dict(ZERO, g=(1, 3, 2)), INVALID),
    ("gy 1", dict(ZERO, g=(4, 1, 2)), INVALID),
    ("gz 0", dict(ZERO, g=(4, 3, 0)), INVALID),
    ("the smallest grid", dict(ZERO, g=(2, 2, 2)), OK),
    ("max == min on x", dict(ZERO, max_point=(-1.0, 2.0, 3.0)), INVALID),
    ("max < min on z", dict(ZERO, max_point=(1.0, 2.0, -3.0)), INVALID),
    ("NaN min", dict(ZERO, min_point=(-1.0, NAN, -1.0)), INVALID),
    ("NaN max", dict(ZERO, max_point=(1.0, 2.0, NAN)), INVALID),
    ("unknown dtype", dict(ZERO, volume_dtype=2), INVALID),
    ("half storage", dict(ZERO, volume_dtype=_lib.VOLUME_F16), OK),
    ("2^30 vertices", dict(ZERO, g=(1024, 1024, 1024)), OK),
    ("beyond 2^30 vertices", dict(ZERO, g=(1024, 1024, 1025)), UNSUPPORTED),
    ("far beyond 2^30 vertices", dict(ZERO, g=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), UNSUPPORTED),
    ("2^31 samples", dict(n_rays=2 ** 21, n_samples=1024), UNSUPPORTED),
    ("null rays", dict(rays=None), INVALID),
    ("null volume", dict(volume=None), INVALID),
    ("rgb without disp", dict(disp=None), INVALID),
    ("acc alone", dict(rgb=None, disp=None), INVALID),
    ("nothing to write", dict(rgb=None, disp=None, acc=None), INVALID),
    ("weights without the maps", dict(rgb=None, disp=None, acc=None, raw=H, weights=H), INVALID),
    ("alpha without the maps", dict(rgb=None, disp=None, acc=None, raw=H, alpha=H), INVALID),
    ("a surface output without the maps", dict(rgb=None, disp=None, acc=None, raw=H, points4=H, median_index=H), INVALID),
    ("removal without points4", dict(has_removal_threshold=1, removal_threshold=0.5), INVALID),
    ("surface_pts without points4", dict(surface_pts=H), INVALID),
    ("surface_rigidity without points4", dict(surface_rigidity=H), INVALID),
    ("median_index without points4", dict(median_index=H), INVALID),
]


@pytest.mark.parametrize("case,kw,want", VOLUME_TABLE, ids=[c[0] for c in VOLUME_TABLE])
def test_volume_render_status_table(case, kw, want):
    lib = _lib.load()
    args = None if kw is None else C.byref(volume_args(**kw))
    assert lib.nrnerf_volume_render(args, STREAM) == want


def bend_args(**kw):
    a = _lib.BendPointsArgs()
    a.struct_size = C.sizeof(_lib.BendPointsArgs)
    a.n_rows, a.n_samples, a.point_stride, a.latent_stride = 3, 5, 3, 32
    a.points, a.latents, a.bent4, a.workspace, a.workspace_bytes = H, H, H, H, _lib.BEND_POINTS_WORKSPACE_BYTES
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ROWS0 = dict(n_rows=0)
BEND_TABLE = [
    ("null model", None, dict(), INVALID),
    ("null args", H, None, INVALID),
    ("zero rows", H, ROWS0, OK),
    ("zero rows, null pointers", H, dict(ROWS0, points=None, latents=None, bent4=None, workspace=None, workspace_bytes=0), OK),
    ("struct_size 0", H, dict(ROWS0, struct_size=0), INVALID),
    ("struct_size of another record", H, dict(ROWS0, struct_size=C.sizeof(_lib.BendPointsArgs) - 8), INVALID),
    ("negative rows", H, dict(n_rows=-1), INVALID),
    ("n_samples 0", H, dict(ROWS0, n_samples=0), INVALID),
    ("n_samples beyond NRNERF_MAX_SAMPLES", H, dict(ROWS0, n_samples=_lib.MAX_SAMPLES + 1), INVALID),
    ("point_stride 2", H, dict(ROWS0, point_stride=2), INVALID),
    ("point_stride 4", H, dict(ROWS0, point_stride=4), OK),
    ("negative latent stride", H, dict(ROWS0, latent_stride=-1), INVALID),
    ("one code for the call", H, dict(ROWS0, latent_stride=0), OK),
    ("unknown flag bit", H, dict(ROWS0, flags=1 << 20), INVALID),
    ("a render flag the query does not honour", H, dict(ROWS0, flags=_lib.RENDER_SPLIT_COARSE), INVALID),
    ("the query's flags", H, dict(ROWS0, flags=_lib.QUERY_FLAGS), OK),
    ("null points", H, dict(points=None), INVALID),
    ("null latents", H, dict(latents=None), INVALID),
    ("null bent4", H, dict(bent4=None), INVALID),
    ("a model without ray bender", H, dict(), INVALID),
]


@pytest.mark.parametrize("case,model,kw,want", BEND_TABLE, ids=[c[0] for c in BEND_TABLE])
def test_bend_points_status_table(case, model, kw, want):
    lib = _lib.load()
    args = None if kw is None else C.byref(bend_args(**kw))
    assert lib.nrnerf_bend_points(C.c_void_p(model), args, STREAM) == want


def test_bend_points_workspace_bytes_of_nothing_is_zero():
    lib = _lib.load()
    assert lib.nrnerf_bend_points_workspace_bytes(None) == 0
    assert lib.nrnerf_bend_points_workspace_bytes(C.c_void_p(H)) == 0          # (zeros: a model without ray bender)


# ---- 3. the reference itself ---------------------------------------------------------------------------------------------------------------------
LO, HI = (-0.5, 0.25, 1.0), (1.5, 1.0, 4.0)


def test_reference_reproduces_an_affine_volume():
    gx, gy, gz = 7, 5, 6
    A = torch.tensor([[0.3, -1.2, 0.7], [2.0, 0.1, -0.4], [-0.9, 0.8, 0.05], [1.1, 1.3, -2.2]], dtype=torch.float64)
    b = torch.tensor([0.2, -0.7, 1.5, 3.0], dtype=torch.float64)
    lo, hi = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (LO, HI))
    ax = [torch.as_tensor(lo[c] + np.arange(n) * ((hi[c] - lo[c]) / (n - 1))) for c, n in enumerate((gx, gy, gz))]
    zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    vol = torch.stack([xx, yy, zz], -1) @ A.t() + b
    pts = V.interior_points((500,), LO, HI, seed=3, outside_share=0.0)
    got = V.lookup_reference(vol, LO, HI, pts)
    want = pts.double() @ A.t() + b
    assert float((got - want).abs().max()) <= 64 * 2.0 ** -52 * float(want.abs().max())


def test_reference_returns_stored_values_at_the_vertices_and_zeros_outside():
    gx, gy, gz = 5, 4, 3
    vol = V.smooth_volume(gx, gy, gz, seed=1)
    lo, hi = (0.0, 0.0, 0.0), (gx - 1.0, gy - 1.0, gz - 1.0)                      # unit spacing: a vertex IS its index
    zz, yy, xx = torch.meshgrid(torch.arange(gz), torch.arange(gy), torch.arange(gx), indexing="ij")
    verts = torch.stack([xx, yy, zz], -1).float()
    for dtype in (torch.float64, torch.float32):
        assert torch.equal(V.lookup_reference(vol, lo, hi, verts, dtype), vol.to(dtype))
    half = vol.half()
    assert torch.equal(V.lookup_reference(half, lo, hi, verts), half.double())
    outside = torch.tensor([[-0.01, 1.0, 1.0], [1.0, gy - 1 + 0.01, 1.0], [1.0, 1.0, gz - 1 + 1e-3], [NAN, 1.0, 1.0], [1.0, 1.0, NAN],
                            [float("inf"), 1.0, 1.0], [1.0, float("-inf"), 1.0]])
    assert torch.equal(V.lookup_reference(vol, lo, hi, outside), torch.zeros(outside.shape[0], 4, dtype=torch.float64))
    # the faces themselves are inside
    faces = torch.tensor([[0.0, 0.0, 0.0], [gx - 1.0, gy - 1.0, gz - 1.0], [0.0, gy - 1.0, 0.5]])
    got = V.lookup_reference(vol, lo, hi, faces)
    assert torch.equal(got[0], vol[0, 0, 0].double()) and torch.equal(got[1], vol[-1, -1, -1].double())
    assert torch.equal(got[2], 0.5 * vol[0, -1, 0].double() + (vol[1, -1, 0].double() - 0.5 * vol[1, -1, 0].double()))


def test_reference_compositing_is_the_oracles():
    vol = V.smooth_volume(9, 8, 7, seed=2)
    g = torch.Generator().manual_seed(5)
    n, s = 11, 33
    o = torch.tensor([0.5, 0.6, 0.0]) + 0.05 * torch.randn(n, 3, generator=g)
    d = torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(n, 3, generator=g)
    rays = torch.cat([o, d, torch.full((n, 1), 0.5), torch.full((n, 1), 5.0)], -1)
    for lindisp in (False, True):
        z = V.coarse_depths(rays, s, lindisp)
        ref = V.render_reference(vol, LO, HI, rays, z, white_bkgd=True)
        pts = rays[:, None, :3].double() + rays[:, None, 3:6].double() * z[..., None]
        raw = V.lookup_reference(vol, LO, HI, pts)
        rgb, disp, acc, alpha, weights, _ = O.composite(raw, z, rays[:, 3:6].double(), True)
        same_disp = (ref["disp_map"] == disp) | (torch.isnan(ref["disp_map"]) & torch.isnan(disp))         # (a ray that misses: 0 / 0, train.py:781-784)
        assert torch.equal(ref["rgb_map"], rgb) and bool(same_disp.all()) and torch.equal(ref["acc_map"], acc)
        assert torch.equal(ref["weights"], weights) and torch.equal(ref["alpha"], alpha) and torch.equal(ref["raw"], raw)
        assert float(ref["acc_map"].max()) > 0.5                                    # (the rays do cross the box)
        idx, _, _ = O.surface_from_details(weights, pts)
        assert torch.equal(ref["median_index"], idx)
    # the removal knob: sigma logits times 0 where the rigidity is at or above the threshold
    p4 = torch.cat([pts, torch.rand(n, s, 1, generator=g, dtype=torch.float64)], -1).float()
    cut = V.render_reference(vol, LO, HI, rays, z, p4, removal_threshold=0.5)
    kept = V.render_reference(vol, LO, HI, rays, z, p4)
    kill = p4[..., 3] >= 0.5
    assert bool((cut["raw"][..., 3][kill] == 0).all()) and torch.equal(cut["raw"][..., 3][~kill], kept["raw"][..., 3][~kill])
    assert torch.equal(cut["raw"][..., :3], kept["raw"][..., :3])


# ---- 4. the resolution series on the fitted checkpoint, in float64 ---------------------------------------------------------------------------------
_series = {}


def series_reference():
    """``(psnr of rgb_map per resolution, psnr of acc_map per resolution, box of the bent samples)`` for 24^3 / 48^3 / 96^3 bakes against the oracle's
    64 + 128 network render; computed once and shared."""
    if not _series:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
        ck, scene, rays, code = V.series_setup()
        n = rays.shape[0]
        with torch.no_grad():
            net = O.batchify_rays(rays.double(), code.double().expand(n, -1), scene, dtype=torch.float64)
            z = V.coarse_depths(rays, V.SERIES_SAMPLES)
            pts = rays[:, None, :3].double() + rays[:, None, 3:6].double() * z[..., None]
            bent = O.bend_points(pts.reshape(-1, 3), code.double().expand(n * V.SERIES_SAMPLES, -1), scene.bender)[0].reshape(n, -1, 3)
            p4 = torch.cat([bent, torch.zeros_like(bent[..., :1])], -1)
            _series["box"] = (bent.reshape(-1, 3).min(0).values, bent.reshape(-1, 3).max(0).values)
            for res in (24, 48, 96):
                vol = V.bake_reference(scene, res)
                out = V.render_reference(vol, V.SERIES_BOX[0], V.SERIES_BOX[1], rays, z, p4)
                _series[res] = (V.psnr(out["rgb_map"], net["rgb_map"]), V.psnr(out["acc_map"], net["acc_map"]))
    return _series


def test_resolution_series_gains_a_decibel_per_doubling_in_float64():
    s = series_reference()
    lo, hi = s["box"]
    print(f"[fitted_latest, frame {V.SERIES_FRAME}, {V.SERIES_WIDTH} wide, S {V.SERIES_SAMPLES}] bent samples within {lo.tolist()} .. {hi.tolist()}")
    for res in (24, 48, 96):
        print(f"  {res}^3: PSNR rgb_map {s[res][0]:.2f} dB, acc_map {s[res][1]:.2f} dB against the oracle's 64 + 128 render")
    box_lo, box_hi = (torch.tensor(v, dtype=torch.float64) for v in V.SERIES_BOX)
    assert bool((lo > box_lo).all()) and bool((hi < box_hi).all())              # no sample is lost to the box
    assert s[48][0] >= s[24][0] + 1.0
    assert s[96][0] >= s[48][0] + 1.0


# ---- 5. the code object ----------------------------------------------------------------------------------------------------------------------------
BUILD = os.path.join(REPO, "nonrigid_nerf_amd", "csrc", "build")


@pytest.mark.skipif(not os.path.isdir(BUILD) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="no build directory / no llvm-readelf")
def test_volume_kernels_use_no_scratch():
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_isa
    obj = os.path.join(BUILD, "nrnerf_volume.o")
    if not os.path.exists(obj):
        pytest.skip("csrc/build/nrnerf_volume.o not built")
    with tempfile.TemporaryDirectory() as tmp:
        co = check_isa.device_code_object(obj, tmp)
        assert co is not None
        notes = subprocess.run([f"{check_isa.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    seen = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or "volume_" not in name.group(1):
            continue
        num = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
        kind = re.search(r"volume_(render|lookup)_kernelI(?:Li(\d+)E)?Lb([01])E", name.group(1))
        assert kind is not None, name.group(1)
        seen[(kind.group(1), int(kind.group(2) or 0), int(kind.group(3)))] = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"),
                                                                                 vgpr_spill=num("vgpr_spill_count"), scratch=num("private_segment_fixed_size"))
    print(seen)
    # every samples-per-lane class of composite_kernel's dispatch in both storage types, and the lookup kernel in both
    assert sorted(seen) == sorted([("render", e, h) for e in (1, 2, 3, 4, 6, 8, 12, 16) for h in (0, 1)] + [("lookup", 0, 0), ("lookup", 0, 1)])
    for key, r in seen.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (key, r)          # (the gathered logits stay in registers: no dynamic indexing)
        assert r["vgpr"] <= 256, (key, r)
