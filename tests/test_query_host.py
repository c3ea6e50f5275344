"""CPU tier of the field query (nrnerf_query / query_points / sample_grid): nothing here needs a device.

* the oracle's ``query_network`` against the reference's own ``network_query_fn`` on non-collinear points
  (tests/golden/query/query_points.npz, tools/make_query_golden.py), at 1/50 of the GPU tolerances -- the rule of tests/test_oracle_golden.py;
* the ctypes records against the header as a C99 compiler sees it;
* a literal status table of the rejections the library decides before its first HIP call;
* the pure planners: the flat-point layout of ``query_points`` and the slabs / argument checks of ``sample_grid``.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd.synthetic import SceneConfig, make_scene
from oracle import nrnerf_oracle as O
from tests.helpers import compare_dict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_GOLDEN = os.path.join(REPO, "tests", "golden", "query", "query_points.npz")
sys.path.insert(0, os.path.join(REPO, "tools"))
from make_query_golden import CASES, N_ROWS, N_SAMPLES, SEED, case_inputs  # noqa: E402


def load_query_case(name):
    """(cfg, scene, knobs, points, latents, viewdirs | None, reference outputs) of one case of the fixture."""
    z = np.load(QUERY_GOLDEN)
    cfg_kw, knobs = CASES[name]
    cfg = SceneConfig(**cfg_kw)
    scene = make_scene(cfg, SEED)
    pts, lat, dirs = case_inputs(name, cfg)
    # the generator must still produce the inputs the reference was run on
    assert np.array_equal(pts.numpy(), z[f"{name}__points"]) and np.array_equal(lat.numpy(), z[f"{name}__latents"])
    assert np.array_equal(dirs.numpy(), z[f"{name}__viewdirs"])
    ref = {k[len(name) + 7:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "__out__")}
    return cfg, scene, knobs, pts, lat, (dirs if cfg.use_viewdirs else None), ref


def test_fixture_is_small_and_not_collinear():
    assert os.path.getsize(QUERY_GOLDEN) < 100 * 1024
    z = np.load(QUERY_GOLDEN)
    for name in CASES:
        p = z[f"{name}__points"].astype(np.float64)
        assert p.shape == (N_ROWS, N_SAMPLES, 3)
        # every row spans three dimensions: the singular values of the centred row are all far from zero
        for row in p:
            assert np.linalg.svd(row - row.mean(0), compute_uv=False).min() > 0.05


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_query_network_matches_the_reference(name):
    cfg, scene, knobs, pts, lat, dirs, ref = load_query_case(name)
    raw, details = O.query_network(pts, dirs, lat, scene.coarse, scene.bender, cfg, knobs=O.Knobs(**knobs), detailed=True)
    got = dict(details, raw=raw)
    assert set(got) == set(ref)
    fails = compare_dict(got, ref, tol_scale=0.02)       # 50x tighter than the GPU fp32 tolerance
    assert not fails, "\n".join(fails)


def test_abi10_records_match_ctypes(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    fields = ["which", "n_rows", "n_samples", "points", "point_stride", "latent_stride", "latents", "viewdirs", "has_rigidity_cutoff",
              "rigidity_cutoff", "has_test_time_scaling", "test_time_scaling", "has_removal_threshold", "removal_threshold", "detailed_output",
              "flags", "raw_ch", "raw", "details", "workspace", "workspace_bytes"]
    assert ["struct_size"] + fields == [f[0] for f in _lib.QueryArgs._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nrnerf.h"\nint main(void) {\n'
                     'printf("%d %zu %zu\\n", NRNERF_ABI_VERSION, sizeof(nrnerf_query_args), sizeof(nrnerf_sample_outputs));\n'
                     + "".join(f'printf("%zu\\n", offsetof(nrnerf_query_args, {f}));\n' for f in fields)
                     + 'printf("%u\\n", (unsigned)(NRNERF_RENDER_NO_X16 | NRNERF_RENDER_BENDER_32X32 | NRNERF_RENDER_FIXED_SHARES));\n'
                     'return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    QA = _lib.QueryArgs
    want = [_lib.ABI_VERSION, C.sizeof(QA), C.sizeof(_lib.SampleOutputs)] + [getattr(QA, f).offset for f in fields] + [_lib.QUERY_FLAGS]
    assert got == want
    assert _lib.ABI_VERSION == 10


# ---- status table: what nrnerf_query / nrnerf_grid_points / nrnerf_field_from_raw answer before their first HIP call ---------------------
OK, INVALID = _lib.OK, _lib.ERR_INVALID
_HOST = (C.c_char * 4096)()
H = (C.addressof(_HOST) + 255) & ~255      # a non-null pointer (never dereferenced by these cases); a non-null model is such an address too
STREAM = C.c_void_p(0)


def query_args(**kw):
    a = _lib.QueryArgs()
    a.struct_size = C.sizeof(_lib.QueryArgs)
    a.which, a.n_rows, a.n_samples, a.point_stride, a.latent_stride, a.raw_ch = 0, 3, 5, 3, 32, 4
    a.points, a.latents, a.raw, a.workspace, a.workspace_bytes = H, H, H, H, 1 << 20
    for k, v in kw.items():
        if k.startswith("details_"):
            setattr(a.details, k[len("details_"):], v)
        else:
            setattr(a, k, v)
    return a


QUERY_TABLE = [
    ("null model", None, dict(), INVALID),
    ("null args", H, None, INVALID),
    ("struct_size 0", H, dict(struct_size=0), INVALID),
    ("struct_size of another ABI", H, dict(struct_size=C.sizeof(_lib.QueryArgs) - 8), INVALID),
    ("struct_size wins over zero rows", H, dict(struct_size=4, n_rows=0), INVALID),
    ("which 2", H, dict(which=2), INVALID),
    ("negative rows", H, dict(n_rows=-1), INVALID),
    ("n_samples 0", H, dict(n_samples=0), INVALID),
    ("n_samples beyond NRNERF_MAX_SAMPLES", H, dict(n_samples=_lib.MAX_SAMPLES + 1), INVALID),
    ("n_samples wins over zero rows", H, dict(n_samples=0, n_rows=0), INVALID),
    ("point_stride 2", H, dict(point_stride=2), INVALID),
    ("point_stride wins over zero rows", H, dict(point_stride=0, n_rows=0), INVALID),
    ("negative latent stride", H, dict(latent_stride=-1), INVALID),
    ("unknown flag bit", H, dict(flags=1 << 20), INVALID),
    ("a render flag the query does not honour", H, dict(flags=_lib.RENDER_UNFUSED_COMPOSITE), INVALID),
    ("honoured flags, zero rows", H, dict(flags=_lib.QUERY_FLAGS, n_rows=0), OK),
    ("visibility_weights set", H, dict(details_visibility_weights=H), INVALID),
    ("opacity_alpha set", H, dict(details_opacity_alpha=H), INVALID),
    ("compositing pointer wins over zero rows", H, dict(details_opacity_alpha=H, n_rows=0), INVALID),
    ("zero rows", H, dict(n_rows=0), OK),
    ("zero rows, null pointers", H, dict(n_rows=0, points=None, raw=None, latents=None, workspace=None, workspace_bytes=0), OK),
    ("null points", H, dict(points=None), INVALID),
    ("null raw", H, dict(raw=None), INVALID),
]


@pytest.mark.parametrize("case,model,kw,want", QUERY_TABLE, ids=[c[0] for c in QUERY_TABLE])
def test_query_status_table(case, model, kw, want):
    lib = _lib.load()
    args = None if kw is None else C.byref(query_args(**kw))
    assert lib.nrnerf_query(C.c_void_p(model), args, STREAM) == want


def test_query_workspace_bytes_of_nothing_is_zero():
    lib = _lib.load()
    assert lib.nrnerf_query_workspace_bytes(None, 0, 4, 4) == 0
    for which, n, s in ((2, 4, 4), (0, 0, 4), (0, 4, 0), (0, 4, _lib.MAX_SAMPLES + 1)):
        assert lib.nrnerf_query_workspace_bytes(C.c_void_p(0), which, n, s) == 0


def _f3(*v):
    return (C.c_float * 3)(*v)


GRID_TABLE = [
    ("null min", (None, _f3(1, 1, 1), 4, 4, 4, 0, 4, H), INVALID),
    ("null max", (_f3(0, 0, 0), None, 4, 4, 4, 0, 4, H), INVALID),
    ("gx 0", (_f3(0, 0, 0), _f3(1, 1, 1), 0, 4, 4, 0, 4, H), INVALID),
    ("gz 0", (_f3(0, 0, 0), _f3(1, 1, 1), 4, 4, 0, 0, 0, H), INVALID),
    ("negative first row", (_f3(0, 0, 0), _f3(1, 1, 1), 4, 4, 4, -1, 4, H), INVALID),
    ("negative rows", (_f3(0, 0, 0), _f3(1, 1, 1), 4, 4, 4, 0, -1, H), INVALID),
    ("rows beyond the grid", (_f3(0, 0, 0), _f3(1, 1, 1), 4, 4, 4, 13, 4, H), INVALID),
    ("zero rows", (_f3(0, 0, 0), _f3(1, 1, 1), 4, 4, 4, 16, 0, None), OK),
    ("null output", (_f3(0, 0, 0), _f3(1, 1, 1), 4, 4, 4, 0, 4, None), INVALID),
    ("host output", (_f3(0, 0, 0), _f3(1, 1, 1), 4, 4, 4, 0, 4, H), INVALID),       # (the owner lookup: not device memory)
]


@pytest.mark.parametrize("case,args,want", GRID_TABLE, ids=[c[0] for c in GRID_TABLE])
def test_grid_points_status_table(case, args, want):
    lib = _lib.load()
    lo, hi, gx, gy, gz, first, n, out = args
    assert lib.nrnerf_grid_points(lo, hi, gx, gy, gz, first, n, C.c_void_p(out), STREAM) == want


FIELD_TABLE = [
    ("negative count", (H, 4, -1, H, H), INVALID),
    ("three channels", (H, 3, 8, H, H), INVALID),
    ("zero values", (None, 4, 0, None, None), OK),
    ("no output asked for", (H, 4, 8, None, None), OK),
    ("null raw", (None, 4, 8, H, H), INVALID),
    ("host raw", (H, 4, 8, H, H), INVALID),
]


@pytest.mark.parametrize("case,args,want", FIELD_TABLE, ids=[c[0] for c in FIELD_TABLE])
def test_field_from_raw_status_table(case, args, want):
    lib = _lib.load()
    raw, ch, n, sigma, rgb = args
    assert lib.nrnerf_field_from_raw(C.c_void_p(raw), ch, n, C.c_void_p(sigma), C.c_void_p(rgb), STREAM) == want


# ---- the pure planners ---------------------------------------------------------------------------------------------------------------------
def test_flat_layout_planner():
    from nonrigid_nerf_amd.render import QUERY_ROW, plan_flat_rows
    assert QUERY_ROW == 64
    assert plan_flat_rows(0) == (0, 64, 0)
    assert plan_flat_rows(1) == (1, 64, 63)
    assert plan_flat_rows(64) == (1, 64, 0)
    assert plan_flat_rows(65) == (2, 64, 63)
    assert plan_flat_rows(1008) == (16, 64, 16)
    assert plan_flat_rows(10, row=7) == (2, 7, 4)
    for m in range(0, 300, 7):
        n_rows, row, pad = plan_flat_rows(m)
        assert n_rows * row - pad == m and 0 <= pad < row
    with pytest.raises(ValueError):
        plan_flat_rows(-1)
    with pytest.raises(ValueError):
        plan_flat_rows(5, row=0)


def test_grid_planners_and_argument_checks():
    from nonrigid_nerf_amd.field import default_rows_per_launch, grid_extent, grid_shape, plan_slabs
    assert grid_shape(24) == (24, 24, 24) and grid_shape((24, 20, 17)) == (24, 20, 17) and grid_shape(np.int64(3)) == (3, 3, 3)
    assert grid_shape((1, 1, _lib.MAX_SAMPLES)) == (1, 1, _lib.MAX_SAMPLES)
    for bad in (0, _lib.MAX_SAMPLES + 1, (4, 4), (4, 0, 4), (4, 4, _lib.MAX_SAMPLES + 1)):
        with pytest.raises(ValueError):
            grid_shape(bad)
    lo, hi = grid_extent([0, -1, 2], (1.5, 1, 2))
    assert lo.dtype == np.float32 and hi.dtype == np.float32 and lo.tolist() == [0, -1, 2] and hi.tolist() == [1.5, 1, 2]
    for bad in (([0, 0], [1, 1, 1]), ([0, 0, 0], [1, -1, 1]), ([0, 0, float("nan")], [1, 1, 1]), ([0, 0, 0], [1, 1, float("inf")])):
        with pytest.raises(ValueError):
            grid_extent(*bad)
    assert plan_slabs(0, 5) == []
    assert plan_slabs(10, None) == [(0, 10)]
    assert plan_slabs(10, 1) == [(r, 1) for r in range(10)]
    assert plan_slabs(10, 7) == [(0, 7), (7, 3)]
    assert plan_slabs(10, 100) == [(0, 10)]
    for n, per in ((340, 7), (340, 340), (1, 1), (17 * 20, 64)):
        slabs = plan_slabs(n, per)
        assert [s[0] for s in slabs] == list(range(0, n, per)) and sum(s[1] for s in slabs) == n and all(0 < s[1] <= per for s in slabs)
    with pytest.raises(ValueError):
        plan_slabs(10, 0)
    with pytest.raises(ValueError):
        plan_slabs(-1, 4)
    assert default_rows_per_launch(64) == (1 << 20) // 64 and default_rows_per_launch(_lib.MAX_SAMPLES) >= 1


def test_load_checkpoint_hands_out_the_query_function():
    """load_checkpoint's kwargs carry render.network_query_fn where the reference's create_nerf puts its own (train.py:633-649, 698-719)."""
    from nonrigid_nerf_amd import render as R
    from nonrigid_nerf_amd.checkpoint import load_checkpoint
    ck = load_checkpoint(os.path.join(REPO, "tests", "golden", "fitted_latest.tar"), N_samples=64, N_importance=128)
    assert ck.render_kwargs_test["network_query_fn"] is R.network_query_fn
