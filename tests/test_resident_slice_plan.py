"""The resident slice of the 16x16x32 trunk kernel (csrc/nrnerf_net_x16.h ``RES``; table: ``ResX16``, csrc/nrnerf_plan.h), host side:
which fragments of the packed image (``nrnerf_pack_host`` which = 10) the kernel keeps in LDS, which ones the ring streams and from
where -- read from the library's own compile-time table (which = 15) and checked against the kernel's fragment order, restated here
from the plan's layer list.  No GPU needed.
"""
import ctypes as C

import numpy as np
import pytest

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd.render import build_model_desc
from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_scene

NFRAGS, NRES, NRING, NUNITS, UNIT_FRAGS, RING = 968, 72, 896, 56, 16, 4
LDS_MAX = 160 * 1024
# the 8 x 256 trunk as PlanX16 lists it: (k-steps, 16-row tiles, encoding k-steps in front) per layer; the skip layer is layer 5
LAYERS = [(2, 16, 2)] + [(8, 16, 0)] * 4 + [(10, 16, 2)] + [(8, 16, 0)] * 2 + [(8, 1, 0)]


def _pack(precision, which):
    """nrnerf_pack_host's size record and unit table for the default architecture (the entry tests/test_packing.py reads the image from)"""
    rb, coarse, fine = build_modules(make_scene(SceneConfig(N_importance=128), 3))
    desc, keep = build_model_desc(coarse, fine, precision, 0)
    lib = _lib.load()
    info = _lib.PackedInfo()
    null_u32, null_f = C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)()
    _lib.check(lib.nrnerf_pack_host(C.byref(desc), which, C.byref(info), None, 0, null_u32, null_f), "size query")
    units = np.zeros(info.n_units + 1, dtype=np.uint32)
    _lib.check(lib.nrnerf_pack_host(C.byref(desc), which, C.byref(info), None, 0, units.ctypes.data_as(C.POINTER(C.c_uint32)), null_f), "table")
    return info, units


def _table(precision):
    info, units = _pack(precision, 15)
    assert info.stream_bytes == 0
    u = [int(x) for x in units]
    nres = u[0]
    res = u[1:1 + nres]
    nunits, unit_frags = u[1 + nres], u[2 + nres]
    offs = u[3 + nres:]
    assert len(offs) == nunits and info.n_units + 1 == len(u)
    assert info.frag_bytes == 1024 and info.slot_bytes == unit_frags * 1024
    return res, nunits, unit_frags, offs


def _sequence():
    """(image fragment, resident?) in the order dense_x16 reads: layer by layer, tile pairs with their k-steps interleaved (SeqPos), a lone
    last tile alone; resident = the first layer, the skip layer's encoding k-steps, the head."""
    out, g = [], 0
    for li, (ns, nt, ne) in enumerate(LAYERS):
        npair = nt // 2
        for q in range(nt * ns):
            slab = (q % (2 * ns)) // 2 if q < npair * 2 * ns else q - npair * 2 * ns
            out.append((g, li == 0 or nt == 1 or slab < ne))
            g += 1
    return out


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_resident_and_ring_fragments_partition_the_image(precision):
    res, nunits, unit_frags, offs = _table(precision)
    assert (len(res), nunits, unit_frags) == (NRES, NUNITS, UNIT_FRAGS)
    assert nunits % RING == 0                                   # unit 0 lands in ring slot 0 every iteration without padding units
    assert all(o % 64 == 0 for o in offs)                       # offsets are in 16-byte words: whole 1 KiB fragments
    ring = [o // 64 + k for o in offs for k in range(unit_frags)]      # every unit: 16 consecutive image fragments
    assert len(ring) == NRING
    assert sorted(res + ring) == list(range(NFRAGS))            # each fragment of the image exactly once
    # the image holds them: 64 units of 16 fragments (the plain stream's padded length)
    info = _pack(precision, 10)[0]
    assert info.stream_bytes == 64 * 16 * 1024 and max(res + ring) < info.stream_bytes // 1024
    # the skip layer's units: eight runs of 16 at stride 20, offset 4, behind layer 0's 32 and layers 1-4's 512 fragments
    assert [o // 64 for o in offs[32:40]] == [544 + 20 * p + 4 for p in range(8)]
    assert [o // 64 for o in offs[:32]] == [32 + 16 * u for u in range(32)]
    assert [o // 64 for o in offs[40:]] == [704 + 16 * u for u in range(16)]


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_walking_the_layers_through_the_table_yields_the_plain_stream(precision):
    res, nunits, unit_frags, offs = _table(precision)
    seq = _sequence()
    assert [g for g, _ in seq] == list(range(NFRAGS))           # (the plain stream IS the image, front to back)
    slot_of = {g: r for r, g in enumerate(res)}
    n_ring, advances, got = 0, [], []
    for pos, (g, resident) in enumerate(seq):
        assert resident == (g in slot_of), (g, resident)
        if resident:
            got.append(res[slot_of[g]])                         # resident block, slot r: copied from image fragment res[r]
        else:
            u, k = divmod(n_ring, unit_frags)
            if k == 0:
                advances.append((u, pos))
            got.append(offs[u] // 64 + k)                       # ring slot u % RING, fragment k of the unit DMA'd from offs[u]
            n_ring += 1
    assert got == [g for g, _ in seq]
    assert n_ring == NRING and [u for u, _ in advances] == list(range(NUNITS))
    # resident slots are taken in image order, in runs of 4 consecutive fragments (one per wave of the copy)
    assert res == sorted(res) and all(res[4 * c + 3] == res[4 * c] + 3 for c in range(NRES // 4))
    # LAG = 2 slot reuse: between the first fragment of unit U and the last fragment of unit U - 2 lie at least 16 positions of the
    # sequence -- more than the 8 fragments the kernel requests ahead -- with or without resident fragments in between
    first = dict(advances)
    last = {}
    n = 0
    for pos, (g, resident) in enumerate(seq):
        if not resident:
            last[n // unit_frags] = pos
            n += 1
    assert all(first[u] - last[u - 2] > 16 for u in range(2, NUNITS))


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_lds_request_fits_the_headline_cases_and_not_256_fused_samples(precision):
    lib = _lib.load()
    prec = {"bf16": 1, "f16": 2}[precision]
    lds = lambda S, fused, resident: int(lib.nrnerf_trunk_kernel_lds_bytes(prec, S, int(fused), int(resident)))
    plain = lambda S, fused: 65536 + 129 * 64 + 128 + ((4 * (1 if (S + 15) // 16 % 4 == 0 else 2 if (S + 15) // 16 % 2 == 0 else 4) * ((S + 15) // 16) * 256 + 256) if fused else 0)
    for S, fused in ((64, False), (192, False), (192, True), (64, True), (85, True), (80, True), (256, True), (256, False)):
        assert lds(S, fused, False) == plain(S, fused)
        assert lds(S, fused, True) == plain(S, fused) + NRES * 1024
    # the headline render (64 + 128 samples): coarse pass raw-to-memory, fine pass with fused compositing -- and both raw-to-memory
    assert lds(64, False, True) <= LDS_MAX and lds(192, True, True) <= LDS_MAX and lds(192, False, True) <= LDS_MAX
    assert lds(85, True, True) <= LDS_MAX                       # two rays per wave group (6 blocks per ray)
    # the fallback is reachable: 256 fused samples, and a stage of four rays per wave (5 blocks per ray), keep the streaming kernel ...
    assert lds(256, True, True) > LDS_MAX and lds(80, True, True) > LDS_MAX
    assert lds(256, True, False) <= LDS_MAX and lds(80, True, False) <= LDS_MAX       # ... whose own request fits
    assert lib.nrnerf_trunk_kernel_lds_bytes(0, 64, 0, 1) == 0  # fp32: no such kernel


def test_no_table_for_the_other_instantiations():
    lib = _lib.load()
    for kw in (dict(netwidth=128, netwidth_fine=128), dict(use_viewdirs=True)):
        rb, coarse, fine = build_modules(make_scene(SceneConfig(N_importance=128, **kw), 3))
        desc, keep = build_model_desc(coarse, fine, "bf16", 0)
        info = _lib.PackedInfo()
        rc = lib.nrnerf_pack_host(C.byref(desc), 15, C.byref(info), None, 0, C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)())
        assert rc == _lib.ERR_UNSUPPORTED, kw
