"""Hierarchical sampling of a baked scene, the parts that need no GPU: the record layout of nrnerf_hierarchical_volume_render_args and what the
entry point answers before its first HIP call, in the order include/nrnerf.h states."""
import ctypes as C
import os

import pytest

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd import field as F
from tests.test_warp_host import _offsets_by_c_program


# ---- 1. record layout ----------------------------------------------------------------------------------------------------------------------------
def test_hierarchical_volume_render_record_matches_ctypes(tmp_path):
    fields = ["n_rays", "n_samples", "n_importance", "rays", "ray_stride", "lindisp", "z", "u", "volume", "volume_dtype", "g", "min_point",
              "max_point", "warp", "warp_dtype", "warp_g", "warp_min_point", "warp_max_point", "has_rigidity_cutoff", "rigidity_cutoff",
              "has_test_time_scaling", "test_time_scaling", "white_bkgd", "has_removal_threshold", "removal_threshold", "rgb", "disp", "acc",
              "rgb0", "disp0", "acc0", "z_std", "z_vals", "raw", "weights", "alpha", "surface_pts", "surface_rigidity", "median_index", "points4"]
    HA = _lib.HierarchicalVolumeRenderArgs
    assert ["struct_size"] + fields == [f[0] for f in HA._fields_]
    got = _offsets_by_c_program(tmp_path, "nrnerf_hierarchical_volume_render_args", fields, ("sizeof(nrnerf_warped_volume_render_args)",))
    assert got == [_lib.ABI_VERSION, C.sizeof(HA)] + [getattr(HA, f).offset for f in fields] + [C.sizeof(_lib.WarpedVolumeRenderArgs)]
    assert _lib.ABI_VERSION == 10                                   # an addition: the version number does not change
    assert C.sizeof(HA) != C.sizeof(_lib.WarpedVolumeRenderArgs)    # (a record of the other call is told apart by its struct_size)


def test_the_fused_shapes_python_knows_are_the_entry_points():
    assert (_lib.HIER_MAX_COARSE, _lib.HIER_MAX_MERGED) == (256, 512)
    for s, i, want in ((3, 1, True), (2, 5, False), (64, 0, False), (256, 256, True), (257, 10, False), (64, 448, True), (64, 449, False)):
        assert F.hierarchical_fused_shape(s, i) is want, (s, i)


# ---- the thin-shell scene of tests/test_hierarchical.py, in float64 ----------------------------------------------------------------------------------
def test_the_float64_model_shows_importance_sampling_at_work_on_the_thin_shell():
    """The scene was chosen so that the float64 model itself shows a factor 2 or more on both maps (measured: 31.4 on acc_map, 6.3 on rgb_map);
    the device test asserts the strict inequality alone."""
    import torch
    from tests import hierarchical_reference as H
    from tests import volume_reference as V
    with torch.no_grad():
        vol, rays = H.shell_volume(), H.shell_rays()
        lo, hi = H.SHELL_BOX
        truth = V.render_reference(vol, lo, hi, rays, V.coarse_depths(rays, 1024))
        uniform = V.render_reference(vol, lo, hi, rays, V.coarse_depths(rays, 64))
        fine, _, z_vals = H.hierarchical_reference(vol, lo, hi, rays, 32, 32)
    eu, eh = H.mean_abs_errors(uniform, truth), H.mean_abs_errors(fine, truth)
    print(f"acc_map: 64 uniform {eu[0]:.3e}, 32 + 32 {eh[0]:.3e}, factor {eu[0] / eh[0]:.2f}; rgb_map: {eu[1]:.3e}, {eh[1]:.3e}, factor {eu[1] / eh[1]:.2f}")
    assert tuple(z_vals.shape) == (rays.shape[0], 64)
    assert eu[0] >= 2 * eh[0] and eu[1] >= 2 * eh[1]


# ---- 2. status table: what the entry point answers before its first HIP call ---------------------------------------------------------------------
OK, INVALID, UNSUPPORTED = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
_HOST = (C.c_char * 4096)()
H = (C.addressof(_HOST) + 255) & ~255      # a non-null pointer, never dereferenced by these cases
STREAM = C.c_void_p(0)
_ARRAYS = ("g", "min_point", "max_point", "warp_g", "warp_min_point", "warp_max_point")


def hier_args(**kw):
    a = _lib.HierarchicalVolumeRenderArgs()
    a.struct_size = C.sizeof(_lib.HierarchicalVolumeRenderArgs)
    a.n_rays, a.n_samples, a.n_importance, a.ray_stride = 3, 5, 4, 8
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


ZERO = dict(n_rays=0)      # a valid record answers OK here, so INVALID / UNSUPPORTED next to it is the named check's
NAN = float("nan")
NO_WARP = dict(warp=None, warp_g=(0, 0, 0), warp_dtype=7, warp_min_point=(0.0, 0.0, 0.0), warp_max_point=(0.0, 0.0, 0.0))
HIER_TABLE = [
    ("null args", None, INVALID),
    ("zero rays", ZERO, OK),
    ("zero rays, null pointers", dict(ZERO, rays=None, volume=None, warp=None, rgb=None, disp=None, acc=None), OK),
    ("struct_size 0", dict(ZERO, struct_size=0), INVALID),
    ("struct_size of nrnerf_warped_volume_render_args", dict(ZERO, struct_size=C.sizeof(_lib.WarpedVolumeRenderArgs)), INVALID),
    ("negative rays", dict(n_rays=-1), INVALID),
    ("n_samples 2", dict(ZERO, n_samples=2), INVALID),
    ("n_samples 3", dict(ZERO, n_samples=3), OK),
    ("n_importance 0", dict(ZERO, n_importance=0), INVALID),
    ("n_importance 1", dict(ZERO, n_importance=1), OK),
    ("ray_stride 7", dict(ZERO, ray_stride=7), INVALID),
    ("ray_stride 11", dict(ZERO, ray_stride=11), OK),
    ("gx 1", dict(ZERO, g=(1, 3, 2)), INVALID),
    ("max == min on x", dict(ZERO, max_point=(-1.0, 2.0, 3.0)), INVALID),
    ("NaN min", dict(ZERO, min_point=(-1.0, NAN, -1.0)), INVALID),
    ("unknown volume dtype", dict(ZERO, volume_dtype=2), INVALID),
    ("warp gy 1", dict(ZERO, warp_g=(3, 1, 5)), INVALID),
    ("warp max < min on z", dict(ZERO, warp_max_point=(0.5, 2.5, -3.0)), INVALID),
    ("unknown warp dtype", dict(ZERO, warp_dtype=2), INVALID),
    ("no warp: its grid record is not read", dict(ZERO, **NO_WARP), OK),
    ("both half", dict(ZERO, warp_dtype=_lib.VOLUME_F16, volume_dtype=_lib.VOLUME_F16), OK),
    ("256 + 256", dict(ZERO, n_samples=256, n_importance=256), OK),
    ("64 + 448", dict(ZERO, n_samples=64, n_importance=448), OK),
    ("257 + 10", dict(ZERO, n_samples=257, n_importance=10), UNSUPPORTED),
    ("64 + 449", dict(ZERO, n_samples=64, n_importance=449), UNSUPPORTED),
    ("3 + 2^31 - 1", dict(ZERO, n_samples=3, n_importance=2 ** 31 - 1), UNSUPPORTED),
    ("a bad grid comes before a shape that is too large", dict(ZERO, n_samples=257, n_importance=10, g=(1, 3, 2)), INVALID),
    ("n_samples 2 comes before a shape that is too large", dict(ZERO, n_samples=2, n_importance=600), INVALID),
    ("volume beyond 2^30 vertices", dict(ZERO, g=(1024, 1024, 1025)), UNSUPPORTED),
    ("warp beyond 2^30 vertices", dict(ZERO, warp_g=(1025, 1024, 1024)), UNSUPPORTED),
    ("2^31 samples", dict(n_rays=2 ** 22, n_samples=256, n_importance=256), UNSUPPORTED),
    ("null rays", dict(rays=None), INVALID),
    ("null volume", dict(volume=None), INVALID),
    ("rgb without disp", dict(disp=None), INVALID),
    ("no fine maps", dict(rgb=None, disp=None, acc=None, rgb0=H, disp0=H, acc0=H), INVALID),
    ("rgb0 without disp0", dict(rgb0=H, acc0=H), INVALID),
    ("acc0 alone", dict(acc0=H), INVALID),
]


@pytest.mark.parametrize("case,kw,want", HIER_TABLE, ids=[c[0] for c in HIER_TABLE])
def test_hierarchical_volume_render_status_table(case, kw, want):
    lib = _lib.load()
    args = None if kw is None else C.byref(hier_args(**kw))
    assert lib.nrnerf_hierarchical_volume_render(args, STREAM) == want


@pytest.mark.parametrize("kw", [dict(), dict(rgb0=H, disp0=H, acc0=H), dict(NO_WARP), dict(z_vals=H, z_std=H, raw=H, surface_pts=H)],
                         ids=["fine maps", "with the coarse maps", "no warp", "optional outputs"])
def test_a_record_that_passes_every_host_check_is_stopped_by_the_device_check(kw):
    """Host memory as the output: every check that needs no HIP call has passed when the ownership check answers INVALID (without a device,
    too: the query itself fails)."""
    assert _lib.load().nrnerf_hierarchical_volume_render(C.byref(hier_args(**kw)), STREAM) == INVALID


# ---- 3. the code objects ---------------------------------------------------------------------------------------------------------------------------
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "nonrigid_nerf_amd", "csrc", "build")


def hier_kernel_resources():
    """``{(EPL_C, EPL_F, volume half, warp half): resources}`` of the kernels of nrnerf_hier_volume_c*.o, from the code objects' metadata; None:
    not built."""
    import re
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_isa
    seen = {}
    for c in (1, 2, 3, 4):
        obj = os.path.join(BUILD, f"nrnerf_hier_volume_c{c}.o")
        if not os.path.exists(obj):
            return None
        with tempfile.TemporaryDirectory() as tmp:
            co = check_isa.device_code_object(obj, tmp)
            assert co is not None
            notes = subprocess.run([f"{check_isa.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            kind = re.search(r"hier_render_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E", name.group(1)) if name else None
            assert kind is not None and int(kind.group(1)) == c, name and name.group(1)
            num = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
            seen[tuple(int(v) for v in kind.groups())] = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), vgpr_spill=num("vgpr_spill_count"),
                                                             scratch=num("private_segment_fixed_size"), lds=num("group_segment_fixed_size"))
    return seen


@pytest.mark.skipif(not os.path.isdir(BUILD) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="no build directory / no llvm-readelf")
def test_hierarchical_kernels_use_no_scratch_and_at_most_16_kib_of_lds():
    seen = hier_kernel_resources()
    if seen is None:
        pytest.skip("csrc/build/nrnerf_hier_volume_c*.o not built")
    for key in sorted(seen):
        print(key, seen[key])
    halves = [(v, w) for v in (0, 1) for w in (0, 1)]
    assert sorted(seen) == sorted((c, f, v, w) for c in (1, 2, 3, 4) for f in (1, 2, 3, 4, 6, 8) if f >= c for v, w in halves)
    for (c, f, _, _), r in seen.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, ((c, f), r)
        assert r["lds"] == 4 * 4 * (64 * f + max(128 * c, 64 * f)) <= 16384, ((c, f), r)
