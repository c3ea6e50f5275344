"""View-dependent bakes, the parts that need no GPU: the record layout of nrnerf_sh_volume_render_args, the basis and the 26-point rule, the
projection identities in float64, the old rule inside the new one, what the entry point answers before its first HIP call (in the order
include/nrnerf.h states), and the resources of the code objects."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import _lib, field
from tests import sh_reference as SH
from tests import volume_reference as V
from tests import warp_reference as W
from tests.test_warp_host import HI, LO, WHI, WLO, _offsets_by_c_program, same, some_rays

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. record layout ----------------------------------------------------------------------------------------------------------------------------
def test_sh_volume_render_record_matches_ctypes(tmp_path):
    SA = _lib.ShVolumeRenderArgs
    fields = [f[0] for f in SA._fields_][1:]
    assert fields[:-4] == [f[0] for f in _lib.WarpedVolumeRenderArgs._fields_][1:]           # the fields of the warped call, then the new ones
    assert fields[-4:] == ["sh", "sh_degree", "points4_in", "direction_mode"]
    got = _offsets_by_c_program(tmp_path, "nrnerf_sh_volume_render_args", fields,
                                ("NRNERF_SH_DIRECTION_DIFFERENCES", "NRNERF_SH_DIRECTION_RAY", "sizeof(nrnerf_warped_volume_render_args)",
                                 "sizeof(nrnerf_volume_render_args)"))
    assert got == [_lib.ABI_VERSION, C.sizeof(SA)] + [getattr(SA, f).offset for f in fields] + [
        _lib.SH_DIRECTION_DIFFERENCES, _lib.SH_DIRECTION_RAY, C.sizeof(_lib.WarpedVolumeRenderArgs), C.sizeof(_lib.VolumeRenderArgs)]
    assert _lib.ABI_VERSION == 10
    assert C.sizeof(SA) not in (C.sizeof(_lib.WarpedVolumeRenderArgs), C.sizeof(_lib.VolumeRenderArgs))      # told apart by struct_size


# ---- 2. the basis and the rule -------------------------------------------------------------------------------------------------------------------
def test_the_direction_table_is_the_26_point_rule():
    d, w = SH.lebedev_26()
    assert np.array_equal(field.SH_DIRECTIONS, d.numpy()) and np.array_equal(field.SH_WEIGHTS, w.numpy())
    assert abs(float(w.sum()) - 1.0) < 1e-15 and float((d.norm(dim=1) - 1).abs().max()) < 1e-15
    assert len({tuple(np.round(v, 9)) for v in d.numpy()}) == 26


def test_the_basis_is_orthonormal_under_the_rule():
    d, w = SH.lebedev_26()
    for degree in (0, 1, 2):
        Y = field.sh_basis(d, degree)
        assert Y.dtype == torch.float64 and tuple(Y.shape) == (26, (degree + 1) ** 2) and torch.equal(Y, SH.basis(d, degree))
        gram = 4.0 * np.pi * (Y * w[:, None]).T @ Y
        err = float((gram - torch.eye(Y.shape[1], dtype=torch.float64)).abs().max())
        print(f"degree {degree}: |4 pi sum w Y Y^T - I|_max = {err:.2e}")
        assert err <= 1e-13


def test_the_float32_basis_is_within_4_ulp_scale_of_float64():
    g = torch.Generator().manual_seed(7)
    d = torch.randn(4096, 3, generator=g)
    d = torch.cat([d / d.norm(dim=1, keepdim=True), SH.lebedev_26()[0].float()], 0)
    y32 = field.sh_basis(d, 2)
    assert y32.dtype == torch.float32
    err = (y32.double() - field.sh_basis(d.double(), 2)).abs().max(0).values
    scale = 2.0 ** -24 * SH.C2                                # an ulp-scale: half an ulp of the largest constant
    print("float32 basis, largest error per function in units of 2^-24 * 1.0925:", [round(float(e / scale), 2) for e in err])
    assert float(err.max()) <= 4 * scale


@pytest.mark.parametrize("bad", [3, -1])
def test_sh_basis_refuses_other_degrees(bad):
    with pytest.raises(ValueError):
        field.sh_basis(torch.zeros(1, 3), bad)


# ---- 3. projection identities, float64 -----------------------------------------------------------------------------------------------------------
def test_a_polynomial_of_degree_2_is_recovered():
    d, _ = SH.lebedev_26()
    g = torch.Generator().manual_seed(3)
    for degree in (0, 1, 2):
        c = torch.randn((degree + 1) ** 2, 5, generator=g, dtype=torch.float64)
        f = SH.basis(d, degree) @ c                                          # IS in the span
        assert float((SH.project(f, degree) - c).abs().max()) <= 1e-12
        if degree < 2:
            assert float(SH.project(f, 2)[c.shape[0]:].abs().max()) <= 1e-12               # and nothing above its degree


def test_the_residual_falls_with_the_degree_and_obeys_parseval():
    d, w = SH.lebedev_26()
    g = torch.Generator().manual_seed(4)
    f = torch.randn(26, 7, generator=g, dtype=torch.float64)
    norm = (w[:, None] * f * f).sum(0)
    before = None
    for degree in (0, 1, 2):
        c = SH.project(f, degree)
        res = (w[:, None] * (f - SH.basis(d, degree) @ c) ** 2).sum(0)
        assert float((res - (norm - (c * c).sum(0) / (4.0 * np.pi))).abs().max()) <= 1e-12
        if before is not None:
            assert bool((res <= before + 1e-15).all())
        before = res
    mean, sh = SH.bake_reference(f[:, :, None].expand(-1, -1, 3).contiguous(), 2)          # [26, 7, 3]: three equal colours
    assert float((mean - SH.C0 * SH.project(f, 0)[0][:, None]).abs().max()) <= 1e-15          # the mean IS Y0 times the coefficient of k = 0
    assert float((sh[:, 3 * 4 + 1] - SH.project(f, 2)[5]).abs().max()) == 0.0                 # channel 3 (k - 1) + c


# ---- 4. the new rule contains the old one ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2])
def test_with_zero_coefficients_the_reference_is_the_old_references(degree):
    vol, warp = V.smooth_volume(9, 8, 7, seed=2), W.smooth_warp(5, 4, 3, seed=1)
    zero = torch.zeros(7, 8, 9, 12 * degree)
    rays = some_rays(11, 5)
    z = V.coarse_depths(rays, 33)
    keys = ("rgb_map", "disp_map", "acc_map", "raw", "weights", "alpha", "median_index")
    for dtype in (torch.float64, torch.float32):
        old = W.render_reference(vol, LO, HI, warp, WLO, WHI, rays, z, white_bkgd=True, removal_threshold=0.6, rigidity_cutoff=0.2, dtype=dtype)
        new = SH.render_reference(vol, zero, degree, LO, HI, rays, z, warp=warp, warp_min=WLO, warp_max=WHI, white_bkgd=True,
                                  removal_threshold=0.6, rigidity_cutoff=0.2, dtype=dtype)
        for k in keys + ("points4", "surface_pts", "surface_rigidity"):
            assert same(new[k], old[k]), k
        again = SH.render_reference(vol, zero, degree, LO, HI, rays, z, points4=old["points4"], removal_threshold=0.6, white_bkgd=True, dtype=dtype)
        straight = SH.render_reference(vol, zero, degree, LO, HI, rays, z, dtype=dtype)
        plain = V.render_reference(vol, LO, HI, rays, z, dtype=dtype)
        for k in keys:
            assert same(again[k], old[k]) and same(straight[k], plain[k]), k
    # ... and coefficients that are not zero do change the colours, under either direction rule
    sh = SH.smooth_sh(9, 8, 7, degree, seed=3)
    a = SH.render_reference(vol, sh, degree, LO, HI, rays, z, warp=warp, warp_min=WLO, warp_max=WHI)
    b = SH.render_reference(vol, sh, degree, LO, HI, rays, z, warp=warp, warp_min=WLO, warp_max=WHI, ray_directions=True)
    assert not torch.equal(a["rgb_map"], old["rgb_map"].double()) and not torch.equal(a["rgb_map"], b["rgb_map"])
    assert torch.equal(a["raw"][..., 3], b["raw"][..., 3]) and torch.equal(a["dirs"][:, 0], a["dirs"][:, 1])


# ---- 5. status table: what the entry point answers before its first HIP call ---------------------------------------------------------------------
OK, INVALID, UNSUPPORTED = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
_HOST = (C.c_char * 4096)()
H = (C.addressof(_HOST) + 255) & ~255      # a non-null pointer, never dereferenced by these cases
STREAM = C.c_void_p(0)
_ARRAYS = ("g", "min_point", "max_point", "warp_g", "warp_min_point", "warp_max_point")
DIFF, RAY = _lib.SH_DIRECTION_DIFFERENCES, _lib.SH_DIRECTION_RAY


def sh_args(**kw):
    a = _lib.ShVolumeRenderArgs()
    a.struct_size = C.sizeof(_lib.ShVolumeRenderArgs)
    a.n_rays, a.n_samples, a.ray_stride = 3, 5, 8
    a.rays, a.volume, a.volume_dtype, a.warp, a.warp_dtype = H, H, _lib.VOLUME_F32, H, _lib.VOLUME_F32
    a.sh, a.sh_degree, a.direction_mode = H, 2, DIFF
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
NO_MAPS = dict(rgb=None, disp=None, acc=None)
NO_WARP = dict(warp=None, warp_g=(0, 0, 0), warp_dtype=7)          # without a warp its four fields are not read
SH_TABLE = [
    ("null args", None, INVALID),
    ("zero rays", ZERO, OK),
    ("zero rays, null pointers", dict(ZERO, rays=None, volume=None, sh=None, warp=None, rgb=None, disp=None, acc=None), OK),
    ("struct_size 0", dict(ZERO, struct_size=0), INVALID),
    ("struct_size of nrnerf_warped_volume_render_args", dict(ZERO, struct_size=C.sizeof(_lib.WarpedVolumeRenderArgs)), INVALID),
    ("negative rays", dict(n_rays=-1), INVALID),
    ("n_samples 0", dict(ZERO, n_samples=0), INVALID),
    ("n_samples NRNERF_MAX_SAMPLES", dict(ZERO, n_samples=_lib.MAX_SAMPLES), OK),
    ("n_samples beyond NRNERF_MAX_SAMPLES", dict(ZERO, n_samples=_lib.MAX_SAMPLES + 1), INVALID),
    ("ray_stride 7", dict(ZERO, ray_stride=7), INVALID),
    ("sh_degree 0", dict(ZERO, sh_degree=0), INVALID),
    ("sh_degree 1", dict(ZERO, sh_degree=1), OK),
    ("sh_degree 3", dict(ZERO, sh_degree=3), INVALID),
    ("unknown direction mode", dict(ZERO, direction_mode=2), INVALID),
    ("differences with one sample", dict(ZERO, n_samples=1), INVALID),
    ("the ray's direction with one sample", dict(ZERO, n_samples=1, direction_mode=RAY), OK),
    ("a warp together with points4_in", dict(ZERO, points4_in=H), INVALID),
    ("points4_in without a warp", dict(ZERO, points4_in=H, **NO_WARP), OK),
    ("straight rays", dict(ZERO, direction_mode=RAY, **NO_WARP), OK),
    ("gx 1", dict(ZERO, g=(1, 3, 2)), INVALID),
    ("unknown volume dtype", dict(ZERO, volume_dtype=2), INVALID),
    ("half volume", dict(ZERO, volume_dtype=_lib.VOLUME_F16), OK),
    ("warp gy 1", dict(ZERO, warp_g=(3, 1, 5)), INVALID),
    ("unknown warp dtype", dict(ZERO, warp_dtype=2), INVALID),
    ("volume beyond 2^30 vertices", dict(ZERO, g=(1024, 1024, 1025)), UNSUPPORTED),
    ("warp beyond 2^30 vertices", dict(ZERO, warp_g=(1025, 1024, 1024)), UNSUPPORTED),
    ("differences with one sample come before a volume that is too large", dict(ZERO, n_samples=1, g=(1024, 1024, 1025)), INVALID),
    ("2^31 samples", dict(n_rays=2 ** 21, n_samples=1024), UNSUPPORTED),
    ("null rays", dict(rays=None), INVALID),
    ("null volume", dict(volume=None), INVALID),
    ("null sh", dict(sh=None), INVALID),
    ("rgb without disp", dict(disp=None), INVALID),
    ("nothing to write", NO_MAPS, INVALID),
    ("weights without the maps", dict(NO_MAPS, raw=H, weights=H), INVALID),
    ("median_index without the maps", dict(NO_MAPS, points4=H, median_index=H), INVALID),
]


@pytest.mark.parametrize("case,kw,want", SH_TABLE, ids=[c[0] for c in SH_TABLE])
def test_sh_volume_render_status_table(case, kw, want):
    args = None if kw is None else C.byref(sh_args(**kw))
    assert _lib.load().nrnerf_sh_volume_render(args, STREAM) == want


@pytest.mark.parametrize("kw", [dict(), dict(NO_MAPS, raw=H), dict(NO_MAPS, points4=H), dict(NO_WARP, points4_in=H, surface_pts=H),
                                dict(NO_WARP, direction_mode=RAY, n_samples=1)],
                         ids=["maps", "raw alone", "points4 alone", "points4_in and a surface output", "straight rays, one sample"])
def test_a_record_that_passes_every_host_check_is_stopped_by_the_device_check(kw):
    """Host memory as the output: every check that needs no HIP call has passed when the ownership check answers INVALID (without a device,
    too: the query itself fails)."""
    assert _lib.load().nrnerf_sh_volume_render(C.byref(sh_args(**kw)), STREAM) == INVALID


# ---- 6. the python surface that needs no device ----------------------------------------------------------------------------------------------------
def test_sh_channels():
    assert field.sh_channels(1) == 12 and field.sh_channels(2) == 24
    for bad in (0, 3):
        with pytest.raises(ValueError):
            field.sh_channels(bad)


# ---- 7. the code objects ---------------------------------------------------------------------------------------------------------------------------
BUILD = os.path.join(REPO, "nonrigid_nerf_amd", "csrc", "build")


def sh_kernel_resources():
    """``{(kind, degree, EPL, volume half, warp half): resources}`` of the kernels of nrnerf_sh_volume_d1.o / _d2.o, from the code objects'
    metadata; None: not built."""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_isa
    seen = {}
    for degree in (1, 2):
        obj = os.path.join(BUILD, f"nrnerf_sh_volume_d{degree}.o")
        if not os.path.exists(obj):
            return None
        with tempfile.TemporaryDirectory() as tmp:
            co = check_isa.device_code_object(obj, tmp)
            assert co is not None
            notes = subprocess.run([f"{check_isa.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count", "\n" + notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or "sh_" not in name.group(1):
                continue
            num = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
            kind = re.search(r"sh_(render|lookup)_kernelILi(\d+)E(?:Li(\d+)E)?Lb([01])ELb([01])E", name.group(1))
            assert kind is not None, name.group(1)
            seen[(kind.group(1), int(kind.group(2)), int(kind.group(3) or 0), int(kind.group(4)), int(kind.group(5)))] = dict(
                agpr=int(re.match(r":\s+(\d+)", blk).group(1)), vgpr=num("vgpr_count"), sgpr=num("sgpr_count"),
                vgpr_spill=num("vgpr_spill_count"), scratch=num("private_segment_fixed_size"), lds=num("group_segment_fixed_size"))
    return seen


@pytest.mark.skipif(not os.path.isdir(BUILD) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="no build directory / no llvm-readelf")
def test_sh_kernels_stay_within_256_registers_with_nothing_in_scratch():
    seen = sh_kernel_resources()
    if seen is None:
        pytest.skip("csrc/build/nrnerf_sh_volume_d*.o not built")
    for key in sorted(seen):
        print(key, seen[key])
    halves = [(v, w) for v in (0, 1) for w in (0, 1)]
    assert sorted(seen) == sorted([("render", d, e, v, w) for d in (1, 2) for e in (1, 2, 3, 4, 6, 8, 12, 16) for v, w in halves]
                                  + [("lookup", d, 0, v, w) for d in (1, 2) for v, w in halves])
    for key, r in seen.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (key, r)
        assert r["vgpr"] <= 256 and r["agpr"] == 0, (key, r)          # (within the architectural VGPRs: nothing is parked in AGPRs either)
