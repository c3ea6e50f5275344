"""Occupancy masks, the parts that need no GPU: the record layouts against a C99 probe, the mask rule (tests/occupancy_reference.py) on
hand-made grids, what the two entry points answer before their first HIP call (in the order include/nrnerf.h states), the resources of the
code objects, and the criterion itself: the lerp of THE VALUE AT A POINT, emulated in numpy, never turns eight sigma logits <= 0 into a
positive one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import _lib
from tests import occupancy_reference as OC
from tests.test_warp_host import _offsets_by_c_program

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. record layouts ---------------------------------------------------------------------------------------------------------------------------
def test_culled_volume_render_record_matches_ctypes(tmp_path):
    CA = _lib.CulledVolumeRenderArgs
    fields = [f[0] for f in CA._fields_][1:]
    assert fields[:-3] == [f[0] for f in _lib.ShVolumeRenderArgs._fields_][1:]           # the fields of the sh call, then the new ones
    assert fields[-3:] == ["occupancy", "occupancy_log2_block", "occupancy_words"]
    got = _offsets_by_c_program(tmp_path, "nrnerf_culled_volume_render_args", fields,
                                ("sizeof(nrnerf_sh_volume_render_args)", "sizeof(nrnerf_warped_volume_render_args)",
                                 "sizeof(nrnerf_volume_render_args)"))
    assert got == [_lib.ABI_VERSION, C.sizeof(CA)] + [getattr(CA, f).offset for f in fields] + [
        C.sizeof(_lib.ShVolumeRenderArgs), C.sizeof(_lib.WarpedVolumeRenderArgs), C.sizeof(_lib.VolumeRenderArgs)]
    assert _lib.ABI_VERSION == 10                                                         # no existing record changed, the version stays
    assert C.sizeof(CA) not in (C.sizeof(_lib.ShVolumeRenderArgs), C.sizeof(_lib.WarpedVolumeRenderArgs), C.sizeof(_lib.VolumeRenderArgs))


def test_occupancy_build_record_matches_ctypes(tmp_path):
    OA = _lib.OccupancyBuildArgs
    fields = ["volume", "volume_dtype", "g", "log2_block", "threshold", "words", "n_words"]
    assert ["struct_size"] + fields == [f[0] for f in OA._fields_]
    got = _offsets_by_c_program(tmp_path, "nrnerf_occupancy_build_args", fields)
    assert got == [_lib.ABI_VERSION, C.sizeof(OA)] + [getattr(OA, f).offset for f in fields]


# ---- 2. the mask rule on hand-made grids ------------------------------------------------------------------------------------------------------------
def empty_grid(gx, gy, gz, dtype=np.float32):
    v = np.zeros((gz, gy, gx, 4), dtype=dtype)
    v[..., :3] = 1.5            # colours are not looked at
    v[..., 3] = -1.0
    return v


def test_block_counts_of_grids_that_are_no_multiple_of_the_block():
    # 9 x 10 x 11 vertices = 8 x 9 x 10 cells at block 4: 2 x 3 x 3 blocks; 6 x 5 x 4 vertices = 5 x 4 x 3 cells at block 2: 3 x 2 x 2
    assert OC.mask_reference(empty_grid(9, 10, 11), 4).shape == (3, 3, 2)
    assert OC.mask_reference(empty_grid(6, 5, 4), 2).shape == (2, 2, 3)
    for g, k, want in (((9, 10, 11), 2, 1), ((6, 5, 4), 1, 1), ((33, 33, 33), 2, 16), ((257, 257, 257), 3, 1024), ((2, 2, 2), 4, 1),
                       ((17, 17, 17), 4, 1), ((18, 17, 17), 4, 1), ((18, 17, 17), 1, 18)):
        assert _lib.occupancy_words(g, k) == want, (g, k)
        assert _lib.load().nrnerf_occupancy_words((C.c_int32 * 3)(*g), k) == want, (g, k)
    lib = _lib.load()
    assert lib.nrnerf_occupancy_words(None, 3) == 0 and lib.nrnerf_occupancy_words((C.c_int32 * 3)(1, 4, 4), 3) == 0
    assert lib.nrnerf_occupancy_words((C.c_int32 * 3)(4, 4, 4), 0) == 0 and lib.nrnerf_occupancy_words((C.c_int32 * 3)(4, 4, 4), 5) == 0


def test_an_all_empty_and_an_all_positive_grid():
    v = empty_grid(9, 10, 11)
    assert not OC.mask_reference(v, 4).any()
    v[..., 3] = 0.0                                                 # <= 0: still empty (relu(0) = 0)
    assert not OC.mask_reference(v, 4).any()
    v[..., 3] = -0.0
    assert not OC.mask_reference(v, 4).any()
    v[..., 3] = np.float32(1e-45)                                   # the smallest denormal is not <= 0
    assert OC.mask_reference(v, 4).all()
    assert not OC.mask_reference(v, 4, threshold=1.0).any()         # ... and is below a lossy threshold


def test_a_lone_positive_vertex_marks_every_block_that_shares_it():
    # inside block (1, 0, 2) of the 9 x 10 x 11 grid at block 4 (x 5, y 2, z 9): that block alone
    v = empty_grid(9, 10, 11)
    v[9, 2, 5, 3] = 0.25
    occ = OC.mask_reference(v, 4)
    assert occ.sum() == 1 and occ[2, 0, 1]
    # on the face x = 4 between blocks bx = 0 and 1: both
    v = empty_grid(9, 10, 11)
    v[9, 2, 4, 3] = 0.25
    occ = OC.mask_reference(v, 4)
    assert occ.sum() == 2 and occ[2, 0, 0] and occ[2, 0, 1]
    # on the corner (4, 4, 4): the eight blocks around it
    v = empty_grid(9, 10, 11)
    v[4, 4, 4, 3] = 0.25
    occ = OC.mask_reference(v, 4)
    assert occ.sum() == 8 and occ[:2, :2, :2].all()
    # the grid's last vertex (x 8, y 9, z 10): the last block alone, though 8 is a multiple of 4 (there is no block bx = 2)
    v = empty_grid(9, 10, 11)
    v[10, 9, 8, 3] = 0.25
    occ = OC.mask_reference(v, 4)
    assert occ.sum() == 1 and occ[2, 2, 1]
    # 6 x 5 x 4 at block 2: vertex (2, 2, 2) is the corner of eight blocks, of which bz = 1 is the last, thin one (cells 2 .. 2)
    v = empty_grid(6, 5, 4)
    v[2, 2, 2, 3] = 0.25
    occ = OC.mask_reference(v, 2)
    assert occ.shape == (2, 2, 3) and occ.sum() == 8 and occ[:2, :2, :2].all()


@pytest.mark.parametrize("channel,value", [(3, np.nan), (3, np.inf), (3, -np.inf), (0, np.nan), (1, np.inf), (2, -np.inf)],
                         ids=["sigma NaN", "sigma +inf", "sigma -inf", "red NaN", "green +inf", "blue -inf"])
def test_a_vertex_that_is_not_finite_marks_its_blocks(channel, value):
    for dtype in (np.float32, np.float16):
        v = empty_grid(9, 10, 11, dtype)
        v[5, 4, 2, channel] = value                                 # y = 4: on the face between by = 0 and 1
        occ = OC.mask_reference(torch.from_numpy(v), 4, threshold=3.0)
        assert occ.sum() == 2 and occ[1, 0, 0] and occ[1, 1, 0]


def test_unused_high_bits_are_zero_and_the_bit_order():
    v = empty_grid(9, 10, 11)
    v[..., 3] = 1.0
    words = OC.pack_bits(OC.mask_reference(v, 4))                   # 18 blocks: one word, bits 0 .. 17
    assert words.dtype == np.int32 and words.tolist() == [(1 << 18) - 1]
    v = empty_grid(9, 10, 11)
    v[9, 6, 5, 3] = 1.0                                             # block (bx 1, by 1, bz 2): index (2 * 3 + 1) * 2 + 1 = 15
    assert OC.pack_bits(OC.mask_reference(v, 4)).tolist() == [1 << 15]
    big = np.ones((5, 4, 3), dtype=bool)                            # 60 blocks: bit 31 of word 0 is the sign bit of an int32
    words = OC.pack_bits(big)
    assert words.tolist() == [-1, (1 << 28) - 1] and OC.unpack_bits(words, (5, 4, 3)).all()
    g = np.random.default_rng(0).random((5, 4, 3)) < 0.5
    assert np.array_equal(OC.unpack_bits(OC.pack_bits(g), g.shape), g)


# ---- 3. status tables: what the entry points answer before their first HIP call ----------------------------------------------------------------------
OK, INVALID, UNSUPPORTED = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
_HOST = (C.c_char * 4096)()
H = (C.addressof(_HOST) + 255) & ~255      # a non-null pointer, never dereferenced by these cases
STREAM = C.c_void_p(0)
_ARRAYS = ("g", "min_point", "max_point", "warp_g", "warp_min_point", "warp_max_point")
DIFF, RAY = _lib.SH_DIRECTION_DIFFERENCES, _lib.SH_DIRECTION_RAY
NAN = float("nan")


def culled_args(**kw):
    a = _lib.CulledVolumeRenderArgs()
    a.struct_size = C.sizeof(_lib.CulledVolumeRenderArgs)
    a.n_rays, a.n_samples, a.ray_stride = 3, 5, 8
    a.rays, a.volume, a.volume_dtype, a.warp, a.warp_dtype = H, H, _lib.VOLUME_F32, H, _lib.VOLUME_F32
    a.sh, a.sh_degree, a.direction_mode = H, 2, DIFF
    a.g[:], a.warp_g[:] = (4, 3, 2), (3, 2, 5)
    a.min_point[:], a.max_point[:] = (-1.0, -1.0, -1.0), (1.0, 2.0, 3.0)
    a.warp_min_point[:], a.warp_max_point[:] = (-2.0, 0.0, -1.0), (0.5, 2.5, 1.0)
    a.rgb, a.disp, a.acc = H, H, H
    a.occupancy, a.occupancy_log2_block, a.occupancy_words = H, 1, 1           # (4, 3, 2) vertices at block 2: 2 x 1 x 1 blocks, one word
    for k, v in kw.items():
        if k in _ARRAYS:
            getattr(a, k)[:] = v
        else:
            setattr(a, k, v)
    return a


ZERO = dict(n_rays=0)      # a valid record answers OK here, so INVALID next to it is the named check's
NO_MAPS = dict(rgb=None, disp=None, acc=None)
NO_WARP = dict(warp=None, warp_g=(0, 0, 0), warp_dtype=7)          # without a warp its four fields are not read
DEG0 = dict(sh=None, sh_degree=0)
CULLED_TABLE = [
    ("null args", None, INVALID),
    ("zero rays", ZERO, OK),
    ("zero rays, null pointers", dict(ZERO, rays=None, volume=None, sh=None, warp=None, rgb=None, disp=None, acc=None, occupancy=None), OK),
    ("struct_size 0", dict(ZERO, struct_size=0), INVALID),
    ("struct_size of nrnerf_sh_volume_render_args", dict(ZERO, struct_size=C.sizeof(_lib.ShVolumeRenderArgs)), INVALID),
    ("negative rays", dict(n_rays=-1), INVALID),
    ("n_samples 0", dict(ZERO, n_samples=0), INVALID),
    ("n_samples NRNERF_MAX_SAMPLES", dict(ZERO, n_samples=_lib.MAX_SAMPLES), OK),
    ("n_samples beyond NRNERF_MAX_SAMPLES", dict(ZERO, n_samples=_lib.MAX_SAMPLES + 1), INVALID),
    ("ray_stride 7", dict(ZERO, ray_stride=7), INVALID),
    ("sh_degree 0: the degree-0 record", dict(ZERO, **DEG0), OK),
    ("sh_degree 1", dict(ZERO, sh_degree=1), OK),
    ("sh_degree 3", dict(ZERO, sh_degree=3), INVALID),
    ("sh_degree -1", dict(ZERO, sh_degree=-1), INVALID),
    ("unknown direction mode", dict(ZERO, direction_mode=2), INVALID),
    ("unknown direction mode at degree 0", dict(ZERO, direction_mode=2, **DEG0), INVALID),
    ("differences with one sample", dict(ZERO, n_samples=1), INVALID),
    ("differences with one sample at degree 0: no direction is made", dict(ZERO, n_samples=1, **DEG0), OK),
    ("the ray's direction with one sample", dict(ZERO, n_samples=1, direction_mode=RAY), OK),
    ("a warp together with points4_in", dict(ZERO, points4_in=H), INVALID),
    ("points4_in without a warp", dict(ZERO, points4_in=H, **NO_WARP), OK),
    ("straight rays", dict(ZERO, direction_mode=RAY, **NO_WARP), OK),
    ("gx 1", dict(ZERO, g=(1, 3, 2)), INVALID),
    ("max not above min", dict(ZERO, max_point=(1.0, -1.0, 3.0)), INVALID),
    ("max NaN", dict(ZERO, max_point=(1.0, NAN, 3.0)), INVALID),
    ("unknown volume dtype", dict(ZERO, volume_dtype=2), INVALID),
    ("half volume", dict(ZERO, volume_dtype=_lib.VOLUME_F16), OK),
    ("warp gy 1", dict(ZERO, warp_g=(3, 1, 5)), INVALID),
    ("unknown warp dtype", dict(ZERO, warp_dtype=2), INVALID),
    ("log2_block 0", dict(ZERO, occupancy_log2_block=0), INVALID),
    ("log2_block 5", dict(ZERO, occupancy_log2_block=5), INVALID),
    ("log2_block 4", dict(ZERO, occupancy_log2_block=4), OK),
    ("log2_block out of range comes before a volume that is too large", dict(ZERO, occupancy_log2_block=0, g=(1024, 1024, 1025)), INVALID),
    ("volume beyond 2^30 vertices", dict(ZERO, g=(1024, 1024, 1025)), UNSUPPORTED),
    ("warp beyond 2^30 vertices", dict(ZERO, warp_g=(1025, 1024, 1024)), UNSUPPORTED),
    ("2^31 samples", dict(n_rays=2 ** 21, n_samples=1024), UNSUPPORTED),
    ("a volume that is too large comes before a wrong word count", dict(ZERO, g=(1024, 1024, 1025), occupancy_words=7), UNSUPPORTED),
    ("one word too many", dict(ZERO, occupancy_words=2), INVALID),
    ("no words", dict(ZERO, occupancy_words=0), INVALID),
    ("the word count of another block size", dict(ZERO, g=(33, 33, 33), occupancy_log2_block=2, occupancy_words=2), INVALID),
    ("33^3 at block 4: 512 blocks, 16 words", dict(ZERO, g=(33, 33, 33), occupancy_log2_block=2, occupancy_words=16), OK),
    ("a wrong word count comes before null pointers", dict(rays=None, occupancy_words=2), INVALID),
    ("null rays", dict(rays=None), INVALID),
    ("null volume", dict(volume=None), INVALID),
    ("null occupancy", dict(occupancy=None), INVALID),
    ("null occupancy at degree 0", dict(occupancy=None, **DEG0), INVALID),
    ("null sh at degree 2", dict(sh=None), INVALID),
    ("sh given at degree 0", dict(sh_degree=0), INVALID),
    ("rgb without disp", dict(disp=None), INVALID),
    ("nothing to write", NO_MAPS, INVALID),
    ("weights without the maps", dict(NO_MAPS, raw=H, weights=H), INVALID),
    ("median_index without the maps", dict(NO_MAPS, points4=H, median_index=H), INVALID),
]


@pytest.mark.parametrize("case,kw,want", CULLED_TABLE, ids=[c[0] for c in CULLED_TABLE])
def test_culled_volume_render_status_table(case, kw, want):
    args = None if kw is None else C.byref(culled_args(**kw))
    assert _lib.load().nrnerf_culled_volume_render(args, STREAM) == want


@pytest.mark.parametrize("kw", [dict(), dict(DEG0), dict(NO_MAPS, raw=H), dict(NO_MAPS, points4=H), dict(NO_WARP, points4_in=H, surface_pts=H),
                                dict(NO_WARP, direction_mode=RAY, n_samples=1), dict(NO_WARP, n_samples=1, **DEG0)],
                         ids=["maps", "degree 0", "raw alone", "points4 alone", "points4_in and a surface output", "straight rays, one sample",
                              "degree 0, straight rays, one sample"])
def test_a_culled_record_that_passes_every_host_check_is_stopped_by_the_device_check(kw):
    """Host memory as the output: every check that needs no HIP call has passed when the ownership check answers INVALID (without a device,
    too: the query itself fails)."""
    assert _lib.load().nrnerf_culled_volume_render(C.byref(culled_args(**kw)), STREAM) == INVALID


def test_the_record_has_no_noise_input():
    """Noise added to sigma voids the criterion.  The public record carries none (no field of that name), so no caller of the C ABI can hand
    one over.  (The kernels' launcher also refuses a compositing record that has one, csrc/nrnerf_culled_volume.h; no entry point can reach
    that branch, and no test here runs it.)"""
    assert not [f for f, _ in _lib.CulledVolumeRenderArgs._fields_ if "noise" in f]


def build_args(**kw):
    a = _lib.OccupancyBuildArgs()
    a.struct_size = C.sizeof(_lib.OccupancyBuildArgs)
    a.volume, a.volume_dtype, a.log2_block, a.threshold, a.words, a.n_words = H, _lib.VOLUME_F32, 2, 0.0, H, 1
    a.g[:] = (9, 10, 11)            # 2 x 3 x 3 blocks at block 4
    for k, v in kw.items():
        if k == "g":
            a.g[:] = v
        else:
            setattr(a, k, v)
    return a


BUILD_TABLE = [
    ("null args", None, INVALID),
    ("struct_size 0", dict(struct_size=0), INVALID),
    ("gz 1", dict(g=(9, 10, 1)), INVALID),
    ("unknown dtype", dict(volume_dtype=2), INVALID),
    ("log2_block 0", dict(log2_block=0), INVALID),
    ("log2_block 5", dict(log2_block=5), INVALID),
    ("negative threshold", dict(threshold=-1e-30), INVALID),
    ("NaN threshold", dict(threshold=NAN), INVALID),
    ("a negative threshold comes before a volume that is too large", dict(threshold=-1.0, g=(1024, 1024, 1025)), INVALID),
    ("beyond 2^30 vertices", dict(g=(1024, 1024, 1025), n_words=1), UNSUPPORTED),
    ("a wrong word count", dict(n_words=2), INVALID),
    ("a wrong word count comes before null pointers", dict(n_words=0, volume=None), INVALID),
    ("null volume", dict(volume=None), INVALID),
    ("null words", dict(words=None), INVALID),
    ("host memory: every host check passed, the device check stops it", dict(), INVALID),
    ("the same with half storage, block 16, a lossy threshold", dict(volume_dtype=_lib.VOLUME_F16, log2_block=4, threshold=2.5), INVALID),
]


@pytest.mark.parametrize("case,kw,want", BUILD_TABLE, ids=[c[0] for c in BUILD_TABLE])
def test_occupancy_build_status_table(case, kw, want):
    args = None if kw is None else C.byref(build_args(**kw))
    assert _lib.load().nrnerf_occupancy_build(args, STREAM) == want


# ---- 4. the code objects ---------------------------------------------------------------------------------------------------------------------------
BUILD = os.path.join(REPO, "nonrigid_nerf_amd", "csrc", "build")
# (the unmasked kernels, whose text the culled ones follow line by line, are held to the same bounds)
OBJECTS = ["nrnerf_culled_volume_d0.o", "nrnerf_culled_volume_d1.o", "nrnerf_culled_volume_d2.o", "nrnerf_occupancy.o",
           "nrnerf_warp.o", "nrnerf_sh_volume_d1.o", "nrnerf_sh_volume_d2.o"]


def occupancy_kernel_resources():
    """``{(object, kernel name): resources}`` of every kernel of the new objects, from the code objects' metadata; None: not built."""
    import re
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_isa
    seen = {}
    for o in OBJECTS:
        obj = os.path.join(BUILD, o)
        if not os.path.exists(obj):
            return None
        with tempfile.TemporaryDirectory() as tmp:
            co = check_isa.device_code_object(obj, tmp)
            assert co is not None
            notes = subprocess.run([f"{check_isa.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count", "\n" + notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            assert name is not None
            num = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
            seen[(o, name.group(1))] = dict(agpr=int(re.match(r":\s+(\d+)", blk).group(1)), vgpr=num("vgpr_count"), sgpr=num("sgpr_count"),
                                            vgpr_spill=num("vgpr_spill_count"), scratch=num("private_segment_fixed_size"),
                                            lds=num("group_segment_fixed_size"))
    return seen


@pytest.mark.skipif(not os.path.isdir(BUILD) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="no build directory / no llvm-readelf")
def test_every_kernel_of_the_new_objects_stays_within_256_registers_with_nothing_in_scratch():
    import re
    seen = occupancy_kernel_resources()
    if seen is None:
        pytest.skip("csrc/build/nrnerf_culled_volume_d*.o / nrnerf_occupancy.o not built")
    for key in sorted(seen):
        print(key, seen[key])
    halves = [(v, w) for v in (0, 1) for w in (0, 1)]
    epls = (1, 2, 3, 4, 6, 8, 12, 16)
    kinds = []
    for (o, name), r in seen.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (o, name, r)
        assert r["vgpr"] <= 256 and r["agpr"] == 0, (o, name, r)          # (within the architectural VGPRs: nothing is parked in AGPRs either)
        m = (re.search(r"culled_(render)_kernelILi(\d+)ELb([01])ELi([012])ELb([01])E", name) or re.search(r"culled_(sh_render)_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E", name)
             or re.search(r"culled_(lookup)_kernelILi(\d+)ELb([01])ELb([01])E", name) or re.search(r"(occupancy_build)_kernelILb([01])E", name)
             or re.search(r"(warped_render)_kernelILi(\d+)ELb([01])ELb([01])E", name) or re.search(r"(warped_lookup)_kernelILb([01])ELb([01])E", name)
             or re.search(r"(?<=\d)(sh_render)_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E", name)
             or re.search(r"(?<=\d)(sh_lookup)_kernelILi(\d+)ELb([01])ELb([01])E", name))
        assert m is not None, name
        kinds.append((o, m.group(1)) + tuple(int(v) for v in m.groups()[1:]))
    # degree 0: (EPL, volume half, source: 0 straight / 1 points4_in / 2 warp, warp half); without a warp its storage is no parameter
    want = [("nrnerf_culled_volume_d0.o", "render", e, v, 2, w) for e in epls for v, w in halves]
    want += [("nrnerf_culled_volume_d0.o", "render", e, v, s, 0) for e in epls for v in (0, 1) for s in (0, 1)]
    want += [(f"nrnerf_culled_volume_d{d}.o", "sh_render", d, e, v, w) for d in (1, 2) for e in epls for v, w in halves]
    want += [(f"nrnerf_culled_volume_d{d}.o", "lookup", d, v, w) for d in (0, 1, 2) for v, w in halves]
    want += [("nrnerf_occupancy.o", "occupancy_build", h) for h in (0, 1)]
    want += [("nrnerf_warp.o", "warped_render", e, v, w) for e in epls for v, w in halves] + [("nrnerf_warp.o", "warped_lookup", v, w) for v, w in halves]
    want += [(f"nrnerf_sh_volume_d{d}.o", "sh_render", d, e, v, w) for d in (1, 2) for e in epls for v, w in halves]
    want += [(f"nrnerf_sh_volume_d{d}.o", "sh_lookup", d, v, w) for d in (1, 2) for v, w in halves]
    assert sorted(kinds) == sorted(want)


# ---- 5. the criterion, emulated --------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fma(a, b, c) of float32 operands, rounded once: the product of two float32 is exact in float64 (48 bits of significand); its sum with a
    float32 is rounded to float64 first and to float32 second -- a double rounding that can differ from the single one only in the last place
    and NEVER in sign or across zero (both roundings are monotone and keep 0), which is all the criterion asks about."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def lerp32(a, b, f):
    """lerp4 of csrc/nrnerf_volume_lookup.h: fma(f, b, fma(-f, a, a))."""
    return fma32(f, b, fma32(-f, a, a))


def trilinear32(c, f):
    """grid_value's order: x, then y, then z.  ``c [n, 8]`` corners 000 100 010 110 001 101 011 111, ``f [n, 3]``."""
    x00, x10 = lerp32(c[:, 0], c[:, 1], f[:, 0]), lerp32(c[:, 2], c[:, 3], f[:, 0])
    x01, x11 = lerp32(c[:, 4], c[:, 5], f[:, 0]), lerp32(c[:, 6], c[:, 7], f[:, 0])
    return lerp32(lerp32(x00, x10, f[:, 1]), lerp32(x01, x11, f[:, 1]), f[:, 2])


def test_eight_corners_at_or_below_zero_never_interpolate_above_zero():
    rng = np.random.default_rng(17)
    n = 100_000
    c = -(100.0 * rng.random((n, 8)) ** 4).astype(np.float32)                    # [-100, 0], crowded towards 0
    f = rng.random((n, 3)).astype(np.float32)
    pick = rng.random((n, 3))
    f[pick < 0.1] = 0.0
    f[pick > 0.9] = 1.0
    f[(pick > 0.45) & (pick < 0.5)] = np.float32(1.0) - np.float32(2.0 ** -24)    # the largest float32 below 1
    f[(pick > 0.5) & (pick < 0.55)] = np.float32(1e-45)
    assert (f == 0).any() and (f == 1).any()
    # edge values among the corners: -0.0, +0.0, denormals, the smallest normal, next to ordinary ones
    edge = np.array([-0.0, 0.0, -1e-45, -1e-40, -1.1754944e-38, -100.0], dtype=np.float32)
    sel = rng.random((n, 8)) < 0.3
    c[sel] = edge[rng.integers(0, len(edge), int(sel.sum()))]
    c[:64] = np.array([[edge[(i >> (k % 6)) % len(edge)] for k in range(8)] for i in range(64)], dtype=np.float32)
    c[64:128] = np.float32(-0.0)
    c[128:192] = np.float32(-1e-45)
    assert (c <= 0).all() and c.min() >= -100.0
    v = trilinear32(c, f)
    worst = float(v.max())
    print(f"{n} cells, corners in [-100, 0]: the largest interpolated sigma is {worst!r}; {int((v == 0).sum())} are zero")
    assert not np.isnan(v).any() and (v <= 0).all()
    # ... and the weight: s = max(sigma, 0) is 0, alpha = 1 - exp(-s * dist) is exactly +0 for every distance
    s = np.maximum(v, np.float32(0.0))
    for dist in (np.float32(1e-3), np.float32(1.0), np.float32(1e10)):
        alpha = np.float32(1.0) - np.exp(-(s * dist), dtype=np.float32)
        assert (alpha == 0).all() and not np.signbit(alpha).any()
    # the criterion is sharp: one corner a denormal above zero can give a positive value
    c2 = c.copy()
    c2[:, 3] = np.float32(1e-45)
    f2 = np.tile(np.array([[1.0, 1.0, 0.0]], dtype=np.float32), (n, 1))          # AT that corner
    assert (trilinear32(c2, f2) > 0).all()
