"""The adjoint of the spherical-harmonic colour sum, the parts that need no GPU: the record layout of nrnerf_sh_lookup_backward_args, what the
entry point answers before its first HIP call (in the order include/nrnerf.h states), the attached reference of tests/sh_grad_reference.py
itself (its forward IS tests/sh_reference.py's; its direction chain against finite differences), and the resources of the new code object."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from nonrigid_nerf_amd import _lib
from tests import sh_grad_reference as SG
from tests import sh_reference as SH
from tests import volume_reference as V
from tests import warp_reference as W
from tests.test_warp_host import _offsets_by_c_program

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. record layout ----------------------------------------------------------------------------------------------------------------------------
def test_sh_lookup_backward_record_matches_ctypes(tmp_path):
    fields = ["n_rays", "n_samples", "rays", "ray_stride", "points4", "direction_mode", "sh", "sh_dtype", "sh_degree", "g", "min_point",
              "max_point", "g_raw", "d_sh", "d_points", "d_dirs"]
    SA = _lib.ShLookupBackwardArgs
    assert ["struct_size"] + fields == [f[0] for f in SA._fields_]
    got = _offsets_by_c_program(tmp_path, "nrnerf_sh_lookup_backward_args", fields,
                                ("NRNERF_VOLUME_F32", "NRNERF_VOLUME_F16", "NRNERF_SH_DIRECTION_DIFFERENCES", "NRNERF_SH_DIRECTION_RAY",
                                 "NRNERF_MAX_SAMPLES", "sizeof(nrnerf_grid_lookup_backward_args)", "sizeof(nrnerf_sh_volume_render_args)"))
    assert got == [_lib.ABI_VERSION, C.sizeof(SA)] + [getattr(SA, f).offset for f in fields] + [
        _lib.VOLUME_F32, _lib.VOLUME_F16, _lib.SH_DIRECTION_DIFFERENCES, _lib.SH_DIRECTION_RAY, _lib.MAX_SAMPLES,
        C.sizeof(_lib.GridLookupBackwardArgs), C.sizeof(_lib.ShVolumeRenderArgs)]
    assert _lib.ABI_VERSION == 10                                   # (an addition: the other records and the version stay)
    assert C.sizeof(SA) not in (C.sizeof(_lib.GridLookupBackwardArgs), C.sizeof(_lib.ShVolumeRenderArgs))


# ---- 2. status table: what the entry point answers before its first HIP call ---------------------------------------------------------------------
OK, INVALID, UNSUPPORTED = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
DIFF, RAY = _lib.SH_DIRECTION_DIFFERENCES, _lib.SH_DIRECTION_RAY
_HOST = (C.c_char * 4096)()
H = (C.addressof(_HOST) + 255) & ~255      # a non-null pointer, never dereferenced by these cases
STREAM = C.c_void_p(0)
_ARRAYS = ("g", "min_point", "max_point")


def grad_args(**kw):
    a = _lib.ShLookupBackwardArgs()
    a.struct_size = C.sizeof(_lib.ShLookupBackwardArgs)
    a.n_rays, a.n_samples = 7, 5
    a.rays, a.ray_stride, a.points4, a.direction_mode = H, 8, H, DIFF
    a.sh, a.sh_dtype, a.sh_degree = H, _lib.VOLUME_F32, 2
    a.g[:] = (4, 3, 2)
    a.min_point[:], a.max_point[:] = (-1.0, -1.0, -1.0), (1.0, 2.0, 3.0)
    a.g_raw, a.d_sh, a.d_points, a.d_dirs = H, H, H, H
    for k, v in kw.items():
        if k in _ARRAYS:
            getattr(a, k)[:] = v
        else:
            setattr(a, k, v)
    return a


ZERO = dict(n_rays=0)        # a valid record answers OK here, so INVALID next to it is the named check's
NAN = float("nan")
GRAD_TABLE = [
    ("null args", None, INVALID),
    ("zero rays", ZERO, OK),
    ("zero rays, null pointers", dict(ZERO, rays=None, points4=None, sh=None, g_raw=None, d_sh=None, d_points=None, d_dirs=None), OK),
    ("struct_size 0", dict(ZERO, struct_size=0), INVALID),
    ("struct_size of nrnerf_grid_lookup_backward_args", dict(ZERO, struct_size=C.sizeof(_lib.GridLookupBackwardArgs)), INVALID),
    ("struct_size of another record", dict(ZERO, struct_size=C.sizeof(_lib.ShLookupBackwardArgs) - 8), INVALID),
    ("negative rays", dict(n_rays=-1), INVALID),
    ("zero samples", dict(ZERO, n_samples=0), INVALID),
    ("too many samples", dict(ZERO, n_samples=_lib.MAX_SAMPLES + 1), INVALID),
    ("the most samples", dict(ZERO, n_samples=_lib.MAX_SAMPLES), OK),
    ("sh_degree 0", dict(ZERO, sh_degree=0), INVALID),
    ("sh_degree 3", dict(ZERO, sh_degree=3), INVALID),
    ("sh_degree 1", dict(ZERO, sh_degree=1), OK),
    ("unknown direction mode", dict(ZERO, direction_mode=2), INVALID),
    ("negative direction mode", dict(ZERO, direction_mode=-1), INVALID),
    ("differences with one sample", dict(ZERO, n_samples=1), INVALID),
    ("the ray rule with one sample", dict(ZERO, n_samples=1, direction_mode=RAY), OK),
    ("the ray rule with ray_stride 5", dict(ZERO, direction_mode=RAY, ray_stride=5), INVALID),
    ("the ray rule with ray_stride 6", dict(ZERO, direction_mode=RAY, ray_stride=6), OK),
    ("differences do not read ray_stride", dict(ZERO, ray_stride=0), OK),
    ("gx 1", dict(ZERO, g=(1, 3, 2)), INVALID),
    ("gz -1", dict(ZERO, g=(4, 3, -1)), INVALID),
    ("the smallest grid", dict(ZERO, g=(2, 2, 2)), OK),
    ("max == min on x", dict(ZERO, max_point=(-1.0, 2.0, 3.0)), INVALID),
    ("NaN min", dict(ZERO, min_point=(-1.0, NAN, -1.0)), INVALID),
    ("NaN max", dict(ZERO, max_point=(1.0, 2.0, NAN)), INVALID),
    ("unknown sh dtype", dict(ZERO, sh_dtype=2), INVALID),
    ("half coefficients", dict(ZERO, sh_dtype=_lib.VOLUME_F16), OK),
    ("2^30 vertices", dict(ZERO, g=(1024, 1024, 1024)), OK),
    ("beyond 2^30 vertices", dict(ZERO, g=(1024, 1024, 1025)), UNSUPPORTED),
    ("a bad grid comes before one that is too large", dict(ZERO, g=(1024, 1024, 1025), sh_dtype=2), INVALID),
    ("too large comes before zero rays", dict(ZERO, g=(1025, 1024, 1024), points4=None), UNSUPPORTED),
    ("2^31 samples", dict(n_rays=2 ** 21, n_samples=1024), UNSUPPORTED),
    ("a bad degree comes before too many samples", dict(n_rays=2 ** 21, n_samples=1024, sh_degree=3), INVALID),
    ("null points4", dict(points4=None), INVALID),
    ("null g_raw", dict(g_raw=None), INVALID),
    ("the ray rule without rays", dict(direction_mode=RAY, rays=None), INVALID),
    ("nothing to write", dict(d_sh=None, d_points=None, d_dirs=None), INVALID),
    ("d_points without sh", dict(sh=None), INVALID),
    ("d_dirs alone without sh", dict(sh=None, d_sh=None, d_points=None), INVALID),
    ("differences: d_points without d_dirs", dict(d_dirs=None), INVALID),
    ("differences: d_points alone without d_dirs", dict(d_dirs=None, d_sh=None), INVALID),
]


@pytest.mark.parametrize("case,kw,want", GRAD_TABLE, ids=[c[0] for c in GRAD_TABLE])
def test_sh_lookup_backward_status_table(case, kw, want):
    lib = _lib.load()
    args = None if kw is None else C.byref(grad_args(**kw))
    assert lib.nrnerf_sh_lookup_backward(args, STREAM) == want


@pytest.mark.parametrize("kw", [dict(), dict(d_points=None, d_dirs=None), dict(d_points=None, d_dirs=None, sh=None), dict(d_sh=None),
                                dict(d_sh=None, d_points=None), dict(direction_mode=RAY, d_dirs=None), dict(rays=None)],
                         ids=["all", "d_sh alone", "d_sh alone needs no sh", "d_points and d_dirs", "d_dirs alone",
                              "the ray rule: d_points without d_dirs", "differences need no rays"])
def test_a_record_that_passes_every_host_check_is_stopped_by_the_device_check(kw):
    """Host memory as the output: every check that needs no HIP call has passed when the ownership check answers INVALID (without a device,
    too: the query itself fails)."""
    assert _lib.load().nrnerf_sh_lookup_backward(C.byref(grad_args(**kw)), STREAM) == INVALID


# ---- 3. the reference itself ---------------------------------------------------------------------------------------------------------------------
LO, HI = (-0.5, 0.25, 1.0), (1.5, 1.0, 4.0)                 # the box of tests/test_warp.py
WLO, WHI = (-0.1, 0.4, 0.5), (1.1, 1.3, 3.2)


def some_rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.5, 0.6, 0.0]) + 0.05 * torch.randn(n, 3, generator=g)
    d = torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(n, 3, generator=g)
    return torch.cat([o, d, torch.full((n, 1), 0.5), torch.full((n, 1), 5.0)], -1)


@pytest.mark.parametrize("degree", [1, 2])
def test_the_attached_reference_has_the_values_of_the_sh_reference(degree):
    """``lookup_channels``, ``basis``, ``directions`` and ``render`` of tests/sh_grad_reference.py: tests/sh_reference.py's, exactly."""
    g = (9, 8, 7)
    vol, sh, warp = V.smooth_volume(*g, seed=2), SH.smooth_sh(*g, degree, seed=4), W.smooth_warp(5, 4, 3, seed=1)
    rays = some_rays(11, 5)
    z = V.coarse_depths(rays, 33)
    for dtype in (torch.float64, torch.float32):
        pts = W.sample_points(rays, z, dtype)
        pts[3, 4] = NAN
        assert torch.equal(SG.lookup_channels(sh.to(dtype), LO, HI, pts), SH.lookup_channels(sh, LO, HI, pts, dtype))
        for ray_directions in (False, True):
            d = SG.directions(pts, rays, ray_directions)
            want = SH.directions(pts, rays, ray_directions, dtype)
            assert bool(((d == want) | (torch.isnan(d) & torch.isnan(want))).all())
        d = SG.directions(W.sample_points(rays, z, dtype), rays, False)
        assert torch.equal(SG.basis(d, degree), SH.basis(d, degree, dtype))
        for knobs in (dict(), dict(rigidity_cutoff=0.4, test_time_scaling=1.5, removal_threshold=0.6)):
            want = SH.render_reference(vol, sh, degree, LO, HI, rays, z, warp=warp, warp_min=WLO, warp_max=WHI, white_bkgd=True, dtype=dtype, **knobs)
            got = SG.render(vol.to(dtype), sh.to(dtype), degree, LO, HI, warp.to(dtype), WLO, WHI, rays, z, white_bkgd=True, **knobs)
            for k in ("raw", "rgb_map", "disp_map", "acc_map", "weights"):
                assert bool(((got[k] == want[k]) | (torch.isnan(got[k]) & torch.isnan(want[k]))).all()), (k, dtype, bool(knobs))
        want = SH.render_reference(vol, sh, degree, LO, HI, rays, z, dtype=dtype)
        got = SG.render(vol.to(dtype), sh.to(dtype), degree, LO, HI, None, None, None, rays, z)
        assert torch.equal(got["raw"], want["raw"]) and torch.equal(got["weights"], want["weights"]) and float(want["acc_map"].max()) > 0.5


@pytest.mark.parametrize("degree", [1, 2])
def test_the_direction_chain_is_the_derivative_of_the_colour_sum_along_a_ray(degree):
    """One ray of nine bent points, float64, DIFFERENCES: ``d_points`` (position part + chain) against central differences of ``sum <g, s>`` in
    every coordinate of every point -- the first point (whose direction is its neighbour's), the last one and an outside one included --
    ``d_dirs`` against central differences in the directions as free variables, ``d_sh`` by the linearity of the sum in the coefficients."""
    g = (5, 4, 3)
    sh = SH.smooth_sh(*g, degree, seed=3).double()
    gen = torch.Generator().manual_seed(9)
    base = torch.tensor([0.4, 0.5, 1.3], dtype=torch.float64)
    pts = (base + torch.arange(9, dtype=torch.float64)[:, None] * torch.tensor([0.03, 0.02, 0.3], dtype=torch.float64)
           + 0.02 * torch.randn(9, 3, generator=gen, dtype=torch.float64))[None]
    pts[0, 5] = torch.tensor([2.0, 0.5, 2.5], dtype=torch.float64)                        # outside the box, between two inside samples
    cot = torch.randn(1, 9, 3, generator=gen, dtype=torch.float64)
    d_sh, d_pts, d_dirs = SG.lookup_backward(sh, degree, LO, HI, pts, cot)
    inside = (SH.lookup_channels(sh, LO, HI, pts) != 0).any(-1)
    assert not bool(inside[0, 5]) and int(inside.sum()) == 8
    assert not bool(d_dirs[0, 5].any()) and bool(d_pts[0, 5].any())                       # an empty sample: the direction part alone

    def loss(p, d=None):
        d = SG.directions(p, None, False) if d is None else d
        return float((SG.colour_sum(sh, degree, LO, HI, p, d) * cot).sum())

    h = 1e-6
    scale = max(1.0, float(d_pts.abs().max()))
    for i in range(9):
        for c in range(3):
            e = torch.zeros_like(pts)
            e[0, i, c] = h
            fd = (loss(pts + e) - loss(pts - e)) / (2 * h)
            assert abs(fd - float(d_pts[0, i, c])) <= 1e-6 * scale, (i, c, fd, float(d_pts[0, i, c]))
    d0 = SG.directions(pts, None, False)
    for i in (0, 1, 8):
        for c in range(3):
            e = torch.zeros_like(d0)
            e[0, i, c] = h
            fd = (loss(pts, d0 + e) - loss(pts, d0 - e)) / (2 * h)
            assert abs(fd - float(d_dirs[0, i, c])) <= 1e-6 * max(1.0, float(d_dirs.abs().max()))
    assert abs(float((d_sh * sh).sum()) - loss(pts)) <= 1e-10 * float((d_sh * sh).abs().sum())
    if degree == 1:
        assert not bool(d_sh[..., 9:].any())


# ---- 4. the code object ----------------------------------------------------------------------------------------------------------------------------
BUILD = os.path.join(REPO, "nonrigid_nerf_amd", "csrc", "build")


def sh_grad_kernel_resources():
    """``{kernel: resources}`` of the kernels of nrnerf_sh_grad.o -- ``("scatter", degree)``, ``("point", degree, half)``, ``"chain"`` -- from the
    code object's metadata; None: not built."""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_isa
    obj = os.path.join(BUILD, "nrnerf_sh_grad.o")
    if not os.path.exists(obj):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        co = check_isa.device_code_object(obj, tmp)
        assert co is not None
        notes = subprocess.run([f"{check_isa.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    seen = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        assert name is not None
        n = name.group(1)
        scatter = re.search(r"sh_scatter_kernelILi([12])ELi(\d+)EE", n)
        point = re.search(r"sh_point_dir_grad_kernelILi([12])ELb([01])EE", n)
        if scatter:
            key = ("scatter", int(scatter.group(1)))
        elif point:
            key = ("point", int(point.group(1)), int(point.group(2)))
        else:
            assert "sh_direction_chain_kernelE" in n, n             # (the unit holds no other kernel)
            key = "chain"
        num = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
        assert key not in seen, key
        seen[key] = dict(vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), vgpr_spill=num("vgpr_spill_count"),
                         sgpr_spill=num("sgpr_spill_count"), scratch=num("private_segment_fixed_size"), lds=num("group_segment_fixed_size"))
    return seen


@pytest.mark.skipif(not os.path.isdir(BUILD) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="no build directory / no llvm-readelf")
def test_sh_grad_kernels_use_no_scratch():
    seen = sh_grad_kernel_resources()
    if seen is None:
        pytest.skip("csrc/build/nrnerf_sh_grad.o not built")
    for key in sorted(seen, key=str):
        print(key, seen[key])
    # the scatter does not read the coefficients: one kernel per degree whatever the storage; the point kernel: per degree and storage
    assert sorted(seen, key=str) == sorted([("scatter", 1), ("scatter", 2), ("point", 1, 0), ("point", 1, 1), ("point", 2, 0), ("point", 2, 1),
                                            "chain"], key=str)
    for key, r in seen.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, (key, r)
        assert r["vgpr"] <= 128, (key, r)                           # (at least four waves per SIMD)
