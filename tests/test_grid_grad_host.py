"""The adjoint of the grid lookup, the parts that need no GPU: the record layout of nrnerf_grid_lookup_backward_args, what the entry point answers
before its first HIP call (in the order include/nrnerf.h states), the differentiable reference of tests/grid_grad_reference.py itself, and the
resources of the new code object."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from nonrigid_nerf_amd import _lib
from tests import grid_grad_reference as G
from tests import volume_reference as V
from tests import warp_reference as W
from tests.test_warp_host import _offsets_by_c_program

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. record layout ----------------------------------------------------------------------------------------------------------------------------
def test_grid_lookup_backward_record_matches_ctypes(tmp_path):
    fields = ["grid", "grid_dtype", "g", "min_point", "max_point", "n_points", "points", "point_stride", "g_value", "d_grid", "d_points"]
    GA = _lib.GridLookupBackwardArgs
    assert ["struct_size"] + fields == [f[0] for f in GA._fields_]
    got = _offsets_by_c_program(tmp_path, "nrnerf_grid_lookup_backward_args", fields,
                                ("NRNERF_VOLUME_F32", "NRNERF_VOLUME_F16", "sizeof(((nrnerf_grid_lookup_backward_args*)0)->n_points)",
                                 "sizeof(nrnerf_volume_render_args)", "sizeof(nrnerf_warped_volume_render_args)"))
    assert got == [_lib.ABI_VERSION, C.sizeof(GA)] + [getattr(GA, f).offset for f in fields] + [
        _lib.VOLUME_F32, _lib.VOLUME_F16, 8, C.sizeof(_lib.VolumeRenderArgs), C.sizeof(_lib.WarpedVolumeRenderArgs)]
    assert _lib.ABI_VERSION == 10                                   # (an addition: the other records and the version stay)
    assert C.sizeof(GA) not in (C.sizeof(_lib.VolumeRenderArgs), C.sizeof(_lib.WarpedVolumeRenderArgs))


# ---- 2. status table: what the entry point answers before its first HIP call ---------------------------------------------------------------------
OK, INVALID, UNSUPPORTED = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
_HOST = (C.c_char * 4096)()
H = (C.addressof(_HOST) + 255) & ~255      # a non-null pointer, never dereferenced by these cases
STREAM = C.c_void_p(0)
_ARRAYS = ("g", "min_point", "max_point")


def grad_args(**kw):
    a = _lib.GridLookupBackwardArgs()
    a.struct_size = C.sizeof(_lib.GridLookupBackwardArgs)
    a.grid, a.grid_dtype = H, _lib.VOLUME_F32
    a.g[:] = (4, 3, 2)
    a.min_point[:], a.max_point[:] = (-1.0, -1.0, -1.0), (1.0, 2.0, 3.0)
    a.n_points, a.points, a.point_stride, a.g_value = 7, H, 3, H
    a.d_grid, a.d_points = H, H
    for k, v in kw.items():
        if k in _ARRAYS:
            getattr(a, k)[:] = v
        else:
            setattr(a, k, v)
    return a


ZERO = dict(n_points=0)      # a valid record answers OK here, so INVALID next to it is the named check's
NAN = float("nan")
GRAD_TABLE = [
    ("null args", None, INVALID),
    ("zero points", ZERO, OK),
    ("zero points, null pointers", dict(ZERO, grid=None, points=None, g_value=None, d_grid=None, d_points=None), OK),
    ("struct_size 0", dict(ZERO, struct_size=0), INVALID),
    ("struct_size of nrnerf_volume_render_args", dict(ZERO, struct_size=C.sizeof(_lib.VolumeRenderArgs)), INVALID),
    ("struct_size of another record", dict(ZERO, struct_size=C.sizeof(_lib.GridLookupBackwardArgs) - 8), INVALID),
    ("negative points", dict(n_points=-1), INVALID),
    ("point_stride 2", dict(ZERO, point_stride=2), INVALID),
    ("point_stride 3", dict(ZERO, point_stride=3), OK),
    ("point_stride 4", dict(ZERO, point_stride=4), OK),
    ("point_stride 11", dict(ZERO, point_stride=11), OK),
    ("gx 1", dict(ZERO, g=(1, 3, 2)), INVALID),
    ("gy 0", dict(ZERO, g=(4, 0, 2)), INVALID),
    ("gz -1", dict(ZERO, g=(4, 3, -1)), INVALID),
    ("the smallest grid", dict(ZERO, g=(2, 2, 2)), OK),
    ("max == min on x", dict(ZERO, max_point=(-1.0, 2.0, 3.0)), INVALID),
    ("max < min on z", dict(ZERO, max_point=(1.0, 2.0, -3.0)), INVALID),
    ("NaN min", dict(ZERO, min_point=(-1.0, NAN, -1.0)), INVALID),
    ("NaN max", dict(ZERO, max_point=(1.0, 2.0, NAN)), INVALID),
    ("unknown grid dtype", dict(ZERO, grid_dtype=2), INVALID),
    ("negative grid dtype", dict(ZERO, grid_dtype=-1), INVALID),
    ("half grid", dict(ZERO, grid_dtype=_lib.VOLUME_F16), OK),
    ("2^30 vertices", dict(ZERO, g=(1024, 1024, 1024)), OK),
    ("beyond 2^30 vertices", dict(ZERO, g=(1024, 1024, 1025)), UNSUPPORTED),
    ("far beyond 2^30 vertices", dict(ZERO, g=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), UNSUPPORTED),
    ("a bad grid comes before one that is too large", dict(ZERO, g=(1024, 1024, 1025), grid_dtype=2), INVALID),
    ("too large comes before zero points", dict(ZERO, g=(1025, 1024, 1024), points=None), UNSUPPORTED),
    ("null points", dict(points=None), INVALID),
    ("null g_value", dict(g_value=None), INVALID),
    ("nothing to write", dict(d_grid=None, d_points=None), INVALID),
    ("d_points without a grid", dict(grid=None), INVALID),
    ("d_points alone without a grid", dict(grid=None, d_grid=None), INVALID),
]


@pytest.mark.parametrize("case,kw,want", GRAD_TABLE, ids=[c[0] for c in GRAD_TABLE])
def test_grid_lookup_backward_status_table(case, kw, want):
    lib = _lib.load()
    args = None if kw is None else C.byref(grad_args(**kw))
    assert lib.nrnerf_grid_lookup_backward(args, STREAM) == want


@pytest.mark.parametrize("kw", [dict(), dict(d_points=None), dict(d_grid=None), dict(d_points=None, grid=None)],
                         ids=["both", "d_grid alone", "d_points alone", "d_grid alone needs no grid"])
def test_a_record_that_passes_every_host_check_is_stopped_by_the_device_check(kw):
    """Host memory as the output: every check that needs no HIP call has passed when the ownership check answers INVALID (without a device,
    too: the query itself fails)."""
    assert _lib.load().nrnerf_grid_lookup_backward(C.byref(grad_args(**kw)), STREAM) == INVALID


# ---- 3. the reference itself ---------------------------------------------------------------------------------------------------------------------
LO, HI = (-0.5, 0.25, 1.0), (1.5, 1.0, 4.0)                 # the box of tests/test_warp.py


def some_points(n, seed):
    pts = V.interior_points((n,), LO, HI, seed=seed)
    pts[n // 2] = NAN
    return pts


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("g", [(2, 2, 2), (5, 4, 3), (17, 9, 33)], ids=["2x2x2", "5x4x3", "17x9x33"])
def test_the_differentiable_lookup_has_the_values_of_the_volume_reference(g, dtype):
    for grid in (V.smooth_volume(*g, seed=sum(g)), V.smooth_volume(*g, seed=sum(g)).half()):
        pts = some_points(301, 7)
        got = G.lookup(grid.to(dtype), LO, HI, pts.to(dtype))
        assert torch.equal(got, V.lookup_reference(grid, LO, HI, pts, dtype))
        assert bool((got == 0).all(-1).any()) and bool((got != 0).any(-1).any())            # empty samples and others


def test_the_adjoint_is_the_derivative_of_the_value():
    """Central differences of the float64 value in the grid and in the points, away from cell faces (the value has a kink there)."""
    g = (5, 4, 3)
    grid = V.smooth_volume(*g, seed=3).double()
    pts = some_points(64, 11).double()
    cot = torch.randn(64, 4, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    val, d_grid, d_pts = G.lookup_backward(grid, LO, HI, pts, cot)
    top = torch.tensor([g[0] - 1.0, g[1] - 1.0, g[2] - 1.0], dtype=torch.float64)
    gc = (pts - torch.tensor(LO, dtype=torch.float64)) * (top / (torch.tensor(HI, dtype=torch.float64) - torch.tensor(LO, dtype=torch.float64)))
    inside = ((gc >= 0) & (gc <= top)).all(-1)
    h = 1e-6
    off_face = inside & (((gc - torch.floor(gc)) > 1e-3) & ((gc - torch.floor(gc)) < 1 - 1e-3)).all(-1)
    assert int(off_face.sum()) > 30 and int((~inside).sum()) > 5
    assert not bool(d_pts[~inside].any())                                               # outside, or NaN: exactly no gradient
    loss = lambda gr, p: (G.lookup(gr, LO, HI, p) * cot).sum(-1)
    for c in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[c] = h
        fd = (loss(grid, pts + e) - loss(grid, pts - e)) / (2 * h)
        assert float((fd - d_pts[:, c])[off_face].abs().max()) <= 1e-6 * max(1.0, float(d_pts.abs().max()))
    # the value is linear in the grid: the adjoint reproduces it, <d_grid, grid> = <cot, value>
    assert abs(float((d_grid * grid).sum()) - float((cot * val).sum())) <= 1e-10 * float((cot * val).abs().sum())
    # and every point spreads its cotangent with weights that sum to one
    assert float((d_grid.sum((0, 1, 2)) - cot[inside].sum(0)).abs().max()) <= 1e-12 * float(cot.abs().sum())


def test_on_a_face_the_derivative_is_the_one_of_the_cell_the_lookup_picks():
    """Unit spacing, a vertex IS its index: at an interior vertex the derivative along x is the difference to the NEXT vertex (the upper cell),
    on the top face the difference from the previous one (the last cell); the cotangent lands on that vertex alone."""
    g = (5, 4, 3)
    grid = V.smooth_volume(*g, seed=3).double()
    lo, hi = (0.0, 0.0, 0.0), (g[0] - 1.0, g[1] - 1.0, g[2] - 1.0)
    verts = W.grid_vertices(lo, hi, g)                                                  # [Gz, Gy, Gx, 3]
    cot = torch.randn(g[2], g[1], g[0], 4, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    val, d_grid, d_pts = G.lookup_backward(grid, lo, hi, verts, cot)
    assert torch.equal(val, grid) and torch.equal(d_grid, cot)
    fwd = grid[:, :, 1:] - grid[:, :, :-1]                                              # along x
    want = torch.cat([fwd, fwd[:, :, -1:]], 2)                                          # the top face: the last cell's
    assert torch.allclose(d_pts[..., 0], (cot * want).sum(-1), rtol=0, atol=1e-13)


def test_the_differentiable_render_has_the_values_of_the_warp_reference():
    vol, warp = V.smooth_volume(9, 8, 7, seed=2), W.smooth_warp(5, 4, 3, seed=1)
    wlo, whi = (-0.1, 0.4, 0.5), (1.1, 1.3, 3.2)
    g = torch.Generator().manual_seed(5)
    o = torch.tensor([0.5, 0.6, 0.0]) + 0.05 * torch.randn(11, 3, generator=g)
    d = torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(11, 3, generator=g)
    rays = torch.cat([o, d, torch.full((11, 1), 0.5), torch.full((11, 1), 5.0)], -1)
    z = V.coarse_depths(rays, 33)
    for knobs in (dict(), dict(rigidity_cutoff=0.4, test_time_scaling=1.5, removal_threshold=0.6)):
        for dtype in (torch.float64, torch.float32):
            want = W.render_reference(vol, LO, HI, warp, wlo, whi, rays, z, white_bkgd=True, dtype=dtype, **knobs)
            got = G.render(vol.to(dtype), LO, HI, warp.to(dtype), wlo, whi, rays, z, white_bkgd=True, **knobs)
            for k in ("rgb_map", "disp_map", "acc_map", "weights"):
                assert bool(((got[k] == want[k]) | (torch.isnan(got[k]) & torch.isnan(want[k]))).all()), (k, dtype)
    straight = G.render(vol.double(), LO, HI, None, None, None, rays, z)
    want = V.render_reference(vol, LO, HI, rays, z)
    assert torch.equal(straight["weights"], want["weights"]) and float(want["acc_map"].max()) > 0.5


# ---- 4. the code object ----------------------------------------------------------------------------------------------------------------------------
BUILD = os.path.join(REPO, "nonrigid_nerf_amd", "csrc", "build")


def grid_grad_kernel_resources():
    """``{kernel: resources}`` of the kernels of nrnerf_grid_grad.o -- ``"scatter"`` (d_grid), ``("point", grid half)`` (d_points) -- from the code
    object's metadata; None: not built."""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_isa
    obj = os.path.join(BUILD, "nrnerf_grid_grad.o")
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
        kind = re.search(r"grid_scatter_kernelE|grid_point_grad_kernelILb([01])EE", name.group(1))
        assert kind is not None, name.group(1)                      # (the unit holds no other kernel)
        num = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
        seen["scatter" if kind.group(1) is None else ("point", int(kind.group(1)))] = dict(
            vgpr=num("vgpr_count"), sgpr=num("sgpr_count"), vgpr_spill=num("vgpr_spill_count"), scratch=num("private_segment_fixed_size"),
            lds=num("group_segment_fixed_size"))
    return seen


@pytest.mark.skipif(not os.path.isdir(BUILD) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="no build directory / no llvm-readelf")
def test_grid_grad_kernels_use_no_scratch():
    seen = grid_grad_kernel_resources()
    if seen is None:
        pytest.skip("csrc/build/nrnerf_grid_grad.o not built")
    for key in sorted(seen, key=str):
        print(key, seen[key])
    # d_grid does not read the grid: one kernel whatever the storage; d_points: float32 and half storage
    assert sorted(seen, key=str) == [("point", 0), ("point", 1), "scatter"]
    for key, r in seen.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["lds"] == 0, (key, r)
        assert r["vgpr"] <= 128, (key, r)                           # (at least four waves per SIMD)
