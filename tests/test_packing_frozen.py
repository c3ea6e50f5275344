"""Frozen weight images: every image ``nrnerf_pack_host`` can produce (``which`` 0-14), pinned byte for byte.

``test_packing.py`` checks that an image MEANS the right network (it emulates the kernels' dataflow); this file checks that an
image does not CHANGE: per configuration and ``which`` the SHA-256 of the fragment stream, of the unit table and of the bias
table, the six ``nrnerf_packed_info`` fields, or -- where the library rejects the request -- the returned status.  The table
(``tests/golden/packed_images_frozen.json``) was recorded from the library as it stood before the packers moved out of
``nrnerf_api.cpp`` into ``nrnerf_pack.cpp``; re-record it (``python tests/test_packing_frozen.py --record``) only together with
a deliberate change of an image's contents.

Weights and biases come from an integer formula (below), not from a random generator, so the table does not depend on the
torch build: a multiplicative hash of the parameter's position in the flat parameter vector scaled into (-1, 1) -- values
with 24 significant bits, so neither f16 nor bf16 holds them and the split images' lo parts are exercised -- with every 97th
entry an exact zero and every 89th a multiple of 1/64 (exact in every format).

What ``nrnerf_pack_host`` does not show -- the source maps of the device-side refresh, and the training images of a
time-conditioned trunk (``which`` 4 / 5 reject it; only a model handle has them) -- is covered by the GPU tier's refresh tests.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd.render import build_model_desc
from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_scene

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_images_frozen.json")
WHICH = range(15)
INFO_FIELDS = ("stream_bytes", "n_units", "n_bias_tiles", "frag_bytes", "slot_bytes", "mfma_per_block")

_VIEWS = dict(use_viewdirs=True)
# name -> (SceneConfig keywords, model flags, precisions)
CONFIGS = {
    # compiled architectures 0 / 1 / 2 / 5, with and without bender (1 is a bender shape, 2 excludes a bender)
    "a0_bend": (dict(), 0, ("f32", "bf16", "f16")),
    "a0_nobend": (dict(ray_bending=False), 0, ("f32", "bf16", "f16")),
    "a1_bend": (dict(bend_depth=7), 0, ("f32", "bf16", "f16")),
    "a2_time_conditioned": (dict(ray_bending=False, time_conditioned_baseline=True), 0, ("f32", "bf16", "f16")),
    "a5_bend": (dict(netwidth=128), 0, ("f32", "bf16", "f16")),
    "a5_nobend": (dict(netwidth=128, ray_bending=False), 0, ("f32", "bf16", "f16")),
    "a0_coarse_only": (dict(N_importance=0), 0, ("bf16",)),
    # the view-dependent head: compiled (finite-difference and exact directions), width class, layer program
    "a0_views_bend": (dict(**_VIEWS), 0, ("f32", "bf16", "f16")),
    "a0_views_nobend": (dict(ray_bending=False, **_VIEWS), 0, ("f32", "bf16")),
    "a1_views_bend": (dict(bend_depth=7, **_VIEWS), 0, ("bf16",)),
    "a0_views_exact": (dict(approx_nonrigid_viewdirs=False, **_VIEWS), 0, ("f32", "bf16")),
    "w192_views": (dict(netwidth=192, netdepth=6, **_VIEWS), 0, ("f32", "bf16", "f16")),
    "w96_views_lv2": (dict(netwidth=96, netdepth=4, skips=(1,), multires_views=2, **_VIEWS), 0, ("bf16", "f16")),
    "views_96_160": (dict(netdepth=7, netwidth=96, netwidth_fine=160, multires=6, multires_views=2, **_VIEWS), 0, ("f32", "bf16", "f16")),
    "time_conditioned_448_views": (dict(netwidth=448, multires=12, latent_size=24, ray_bending=False, time_conditioned_baseline=True,
                                        multires_views=6, **_VIEWS), 0, ("f32", "bf16")),
    # NRNERF_MODEL_NO_X16_F16
    "a0_bend_no_x16_f16": (dict(), _lib.MODEL_NO_X16_F16, ("bf16", "f16")),
    "a0_views_no_x16_f16": (dict(**_VIEWS), _lib.MODEL_NO_X16_F16, ("f16",)),
    # generic shapes: those of test_packing.py, and widths that are no multiple of 32
    "w192_d6_l8": (dict(netwidth=192, netdepth=6, multires=8), 0, ("f32", "bf16", "f16")),
    "w320_d10": (dict(netwidth=320, netdepth=10), 0, ("f32", "bf16", "f16")),
    "w64_d3_noskip": (dict(netwidth=64, netdepth=3, skips=()), 0, ("f32", "bf16", "f16")),
    "192_320_latent16": (dict(netdepth=6, netwidth=192, netdepth_fine=10, netwidth_fine=320, multires=8, latent_size=16), 0, ("f32", "bf16", "f16")),
    "192_320_skip2_bwd": (dict(netdepth=6, netwidth=192, netdepth_fine=5, netwidth_fine=320, skips=(2,), multires=8, latent_size=16), 0, ("f32", "bf16")),
    "w72_d4_nobend": (dict(netdepth=4, netwidth=72, ray_bending=False), 0, ("f32", "bf16", "f16")),
    "w500_d5_skip1_l4": (dict(netwidth=500, netdepth=5, skips=(1,), multires=4), 0, ("bf16", "f16")),
    "w100_bend_hidden48": (dict(netwidth=100, netdepth=5, skips=(2,), bend_hidden=48, rigidity_hidden=24), 0, ("f32", "bf16")),
}
CASES = [(name, p) for name, (_, _, precs) in CONFIGS.items() for p in precs]


def formula_values(first, count):
    """Parameter values of flat positions first .. first + count - 1 (float32)."""
    i = np.arange(first, first + count, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    v = ((h >> np.uint64(8)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)      # 24-bit grid in [-1, 1)
    coarse_grid = np.round(v * 64.0) / 64.0
    v = np.where(i % np.uint64(89) == 0, coarse_grid.astype(np.float32), v)
    v = np.where(i % np.uint64(97) == 0, np.float32(0.0), v)
    return v


def fill_modules(rb, coarse, fine):
    """Overwrites every nn.Linear of the three modules, in the order of the flat parameter vector (include/nrnerf.h)."""
    at = [0]

    def fill(lin):
        for p in (lin.weight, lin.bias):
            if p is None:
                continue
            with torch.no_grad():
                p.copy_(torch.from_numpy(formula_values(at[0], p.numel()).reshape(tuple(p.shape))))
            at[0] += p.numel()

    if rb is not None:
        for lin in list(rb.network) + list(rb.rigidity_network):
            fill(lin)
    for net in (coarse, fine):
        if net is None:
            continue
        for lin in net.pts_linears:
            fill(lin)
        if net.use_viewdirs:
            for lin in (net.alpha_linear, net.feature_linear, net.views_linears[0], net.rgb_linear):
                fill(lin)
        else:
            fill(net.output_linear)
    return at[0]


def pack_all(name, precision):
    kw, flags, _ = CONFIGS[name]
    scene = make_scene(SceneConfig(**kw), 3)
    rb, coarse, fine = build_modules(scene)
    assert fill_modules(rb, coarse, fine) > 0
    desc, keep = build_model_desc(coarse, fine, precision, 0, flags=flags)
    lib = _lib.load()
    null_u32, null_f = C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)()
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    got = {}
    for which in WHICH:
        info = _lib.PackedInfo()
        rc = lib.nrnerf_pack_host(C.byref(desc), which, C.byref(info), None, 0, null_u32, null_f)
        if rc != _lib.OK:
            got[str(which)] = {"status": rc}
            continue
        stream = np.zeros(info.stream_bytes, dtype=np.uint8)
        units = np.zeros(info.n_units + 1, dtype=np.uint32)
        bias = np.zeros(info.n_bias_tiles * 32, dtype=np.float32)       # (16 rows per tile in the 16x16x32 images: the rest stays zero)
        rc = lib.nrnerf_pack_host(C.byref(desc), which, C.byref(info), stream.ctypes.data_as(C.c_void_p), stream.nbytes,
                                  units.ctypes.data_as(C.POINTER(C.c_uint32)), bias.ctypes.data_as(C.POINTER(C.c_float)))
        got[str(which)] = {"status": rc, "info": [int(getattr(info, f)) for f in INFO_FIELDS],
                           "stream": sha(stream), "units": sha(units), "bias": sha(bias)}
    del keep
    return got


def test_formula_exercises_zeros_and_the_lo_part():
    v = formula_values(0, 4096)
    assert v.dtype == np.float32 and np.abs(v).max() < 1.0 and (v == 0).sum() >= 4096 // 97
    assert (v.astype(np.float16).astype(np.float32) != v).mean() > 0.9          # not representable in f16: a non-zero lo part
    assert hashlib.sha256(v.tobytes()).hexdigest() == "1205ace7d4c89db5c815300648e06672a773441141d91f2c7409f50a6cf39af7"


@pytest.mark.parametrize("name,precision", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_every_image_is_byte_identical_to_the_recorded_one(name, precision):
    with open(TABLE) as f:
        want = json.load(f)[f"{name}-{precision}"]
    got = pack_all(name, precision)
    assert set(got) == set(want) == {str(w) for w in WHICH}
    for which in WHICH:
        assert got[str(which)] == want[str(which)], f"which = {which}"


def test_the_table_covers_every_kind_of_image():
    """Every ``which`` is accepted by some configuration and rejected by another (7, the coarse network's layer program, exists for
    every description, the compiled shapes included): no route goes unpinned."""
    with open(TABLE) as f:
        table = json.load(f)
    assert set(table) == {f"{n}-{p}" for n, p in CASES}
    for which in WHICH:
        statuses = {entry[str(which)]["status"] for entry in table.values()}
        assert _lib.OK in statuses, which
        if which != 7:
            assert statuses - {_lib.OK}, which


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: test_packing_frozen.py --record"
    table = {f"{n}-{p}": pack_all(n, p) for n, p in CASES}
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} configurations, {sum(e[str(w)]['status'] == 0 for e in table.values() for w in WHICH)} images recorded")
