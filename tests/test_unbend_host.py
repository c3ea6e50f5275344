"""The inverse of the ray bender, the parts that need no GPU: the reference solver on the fitted checkpoints (the conditions the GPU tests of
tests/test_unbend.py rely on hold for the REFERENCE alone), the record layout of nrnerf_bender_inverse_args, what the entry point answers
before its first HIP call, the pure mesh helper, and the new code object's metadata."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest
import torch

from nonrigid_nerf_amd import _lib, field as F
from oracle import nrnerf_oracle as O
from tests.unbend_reference import cube_points, fitted, unbend_reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(REPO, "nonrigid_nerf_amd", "csrc", "build")

_solved = {}


def reference_solve(name, scaling=None, omega=1.0, dtype=torch.float64):
    """The reference solver on code 3 of a fitted checkpoint, 2000 seeded points in the cube of half the far bound, tol 1e-6, 64 evaluations;
    computed once per case and shared (tests/test_unbend.py reads it too)."""
    key = (name, scaling, omega, dtype)
    if key not in _solved:
        ck, bender, half = fitted(name)
        pts = cube_points(2000, half, seed=0, dtype=dtype)
        _solved[key] = unbend_reference(pts, ck.latents[3].reshape(1, -1), bender, knobs=O.Knobs(test_time_scaling=scaling), tol=1e-6,
                                        relaxation=omega, max_iters=64)
    return _solved[key]


# ---- 1. the reference on the fitted checkpoints ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fitted_latest", "fitted_config4", "fitted_w128"])
def test_reference_converges_on_the_fitted_checkpoints(name):
    sol = reference_solve(name)
    share = float(sol["converged"].double().mean())
    its = sol["iterations"][sol["converged"]].double()
    print(f"[{name}, omega 1] converged {100 * share:.2f} %, evaluations median {its.median():.0f} / 95 % {its.quantile(0.95):.0f} / max {its.max():.0f}")
    assert share >= 0.995
    assert bool((sol["residual"][sol["converged"]] <= 1e-6).all())
    assert int(sol["iterations"].min()) >= 1 and int(sol["iterations"].max()) <= 64
    assert bool((sol["iterations"][~sol["converged"]] == 64).all())


def test_reference_needs_the_relaxation_factor_under_motion_exaggeration():
    damped = reference_solve("fitted_latest", scaling=2.0, omega=0.7)
    plain = reference_solve("fitted_latest", scaling=2.0, omega=1.0)
    n_damped, n_plain = int(damped["converged"].sum()), int(plain["converged"].sum())
    print(f"[fitted_latest, test_time_scaling 2] converged: omega 0.7 {n_damped} / 2000, omega 1 {n_plain} / 2000")
    assert n_damped >= 0.995 * 2000
    assert n_plain < n_damped


def test_reference_residual_is_that_of_the_returned_point():
    ck, bender, half = fitted("fitted_latest")
    pts = cube_points(200, half, seed=1)
    lat = ck.latents[3].reshape(1, -1)
    for kw in (dict(max_iters=1), dict(max_iters=3, relaxation=0.5), dict(tol=1e-3)):
        sol = unbend_reference(pts, lat, bender, **kw)
        bent = O.bend_points(sol["points"], lat.double().expand(200, -1), bender)[0]
        # (the solver evaluates shrinking subsets of the points: the matrix products of another batch size may round in another order)
        assert float(((bent - pts).abs().max(-1).values - sol["residual"]).abs().max()) <= 1e-12, kw
    assert torch.equal(unbend_reference(pts, lat, bender, max_iters=1)["points"], pts)
    nan = unbend_reference(torch.full((1, 3), float("nan"), dtype=torch.float64), lat, bender, max_iters=5)
    assert int(nan["iterations"]) == 5 and not bool(nan["converged"])


# ---- 2. record layout ------------------------------------------------------------------------------------------------------------------------------
def test_bender_inverse_record_matches_ctypes(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    fields = ["n_rows", "n_samples", "canonical", "point_stride", "initial", "latents", "latent_stride", "has_rigidity_cutoff", "rigidity_cutoff",
              "has_test_time_scaling", "test_time_scaling", "tolerance", "relaxation", "max_iters", "flags", "observed", "residual", "iterations",
              "workspace", "workspace_bytes"]
    assert ["struct_size"] + fields == [f[0] for f in _lib.BenderInverseArgs._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nrnerf.h"\nint main(void) {\n'
                     'printf("%d %zu\\n", NRNERF_ABI_VERSION, sizeof(nrnerf_bender_inverse_args));\n'
                     + "".join(f'printf("%zu\\n", offsetof(nrnerf_bender_inverse_args, {f}));\n' for f in fields)
                     + 'printf("%u\\n", (unsigned)NRNERF_RENDER_FIXED_SHARES);\nreturn 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    BA = _lib.BenderInverseArgs
    assert got == [_lib.ABI_VERSION, C.sizeof(BA)] + [getattr(BA, f).offset for f in fields] + [_lib.BENDER_INVERSE_FLAGS]
    assert _lib.ABI_VERSION == 10


# ---- 3. status table: what nrnerf_bender_inverse answers before its first HIP call -----------------------------------------------------------------
OK, INVALID = _lib.OK, _lib.ERR_INVALID
_HOST = (C.c_char * 4096)()
H = (C.addressof(_HOST) + 255) & ~255      # a non-null pointer, never dereferenced by these cases -- except as a MODEL: zeros, i.e. no ray bender
STREAM = C.c_void_p(0)


def inverse_args(**kw):
    a = _lib.BenderInverseArgs()
    a.struct_size = C.sizeof(_lib.BenderInverseArgs)
    a.n_rows, a.n_samples, a.point_stride, a.latent_stride = 3, 5, 3, 32
    a.tolerance, a.relaxation, a.max_iters = 1e-6, 1.0, 64
    a.canonical, a.latents, a.observed, a.workspace, a.workspace_bytes = H, H, H, H, 256
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ZERO = dict(n_rows=0)      # a valid record answers OK here, so INVALID next to it is the named check's
INVERSE_TABLE = [
    ("null model", None, dict(), INVALID),
    ("null args", H, None, INVALID),
    ("zero rows", H, ZERO, OK),
    ("zero rows, null pointers", H, dict(ZERO, canonical=None, latents=None, observed=None, workspace=None, workspace_bytes=0), OK),
    ("struct_size 0", H, dict(ZERO, struct_size=0), INVALID),
    ("struct_size of another record", H, dict(ZERO, struct_size=C.sizeof(_lib.BenderInverseArgs) - 8), INVALID),
    ("negative rows", H, dict(n_rows=-1), INVALID),
    ("n_samples 0", H, dict(ZERO, n_samples=0), INVALID),
    ("n_samples beyond NRNERF_MAX_SAMPLES", H, dict(ZERO, n_samples=_lib.MAX_SAMPLES + 1), INVALID),
    ("point_stride 2", H, dict(ZERO, point_stride=2), INVALID),
    ("negative latent stride", H, dict(ZERO, latent_stride=-1), INVALID),
    ("negative tolerance", H, dict(ZERO, tolerance=-1e-9), INVALID),
    ("NaN tolerance", H, dict(ZERO, tolerance=float("nan")), INVALID),
    ("tolerance 0", H, dict(ZERO, tolerance=0.0), OK),
    ("infinite tolerance", H, dict(ZERO, tolerance=float("inf")), OK),
    ("relaxation 0", H, dict(ZERO, relaxation=0.0), INVALID),
    ("negative relaxation", H, dict(ZERO, relaxation=-0.5), INVALID),
    ("relaxation above 1", H, dict(ZERO, relaxation=1.0000001), INVALID),
    ("NaN relaxation", H, dict(ZERO, relaxation=float("nan")), INVALID),
    ("relaxation 0.5", H, dict(ZERO, relaxation=0.5), OK),
    ("max_iters 0", H, dict(ZERO, max_iters=0), INVALID),
    ("max_iters 1025", H, dict(ZERO, max_iters=_lib.BENDER_INVERSE_MAX_ITERS + 1), INVALID),
    ("max_iters 1", H, dict(ZERO, max_iters=1), OK),
    ("max_iters 1024", H, dict(ZERO, max_iters=_lib.BENDER_INVERSE_MAX_ITERS), OK),
    ("unknown flag bit", H, dict(ZERO, flags=1 << 20), INVALID),
    ("a render flag the inverse does not honour", H, dict(ZERO, flags=_lib.RENDER_NO_X16), INVALID),
    ("fixed shares", H, dict(ZERO, flags=_lib.RENDER_FIXED_SHARES), OK),
    ("null canonical", H, dict(canonical=None), INVALID),
    ("null latents", H, dict(latents=None), INVALID),
    ("null observed", H, dict(observed=None), INVALID),
    ("a model without ray bender", H, dict(), INVALID),
]


@pytest.mark.parametrize("case,model,kw,want", INVERSE_TABLE, ids=[c[0] for c in INVERSE_TABLE])
def test_bender_inverse_status_table(case, model, kw, want):
    lib = _lib.load()
    args = None if kw is None else C.byref(inverse_args(**kw))
    assert lib.nrnerf_bender_inverse(C.c_void_p(model), args, STREAM) == want


def test_bender_inverse_workspace_bytes_of_nothing_is_zero():
    lib = _lib.load()
    assert lib.nrnerf_bender_inverse_workspace_bytes(None) == 0
    assert lib.nrnerf_bender_inverse_workspace_bytes(C.c_void_p(H)) == 0       # (zeros: a model without ray bender)


# ---- 4. pure helpers -------------------------------------------------------------------------------------------------------------------------------
def _normals_f64(vertices, faces):
    v = vertices.double()
    acc = torch.zeros_like(v)
    for tri in faces.tolist():
        a, b, c = (v[i] for i in tri)
        n = torch.linalg.cross(b - a, c - a)
        for i in tri:
            acc[i] += n
    length = acc.norm(dim=-1, keepdim=True)
    return torch.where(length > 0, acc / length.clamp_min(1e-300), torch.zeros_like(acc))


def test_vertex_normals_of_a_tetrahedron_and_a_strip():
    tet_v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0]])
    tet_f = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32)          # outward winding
    got = F.vertex_normals(tet_v, tet_f)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3)
    assert float((got.double() - _normals_f64(tet_v, tet_f)).abs().max()) <= 4 * 2.0 ** -24
    centre = tet_v.mean(0)
    assert bool((((tet_v - centre) * got).sum(-1) > 0).all())                                       # outward at every vertex
    # two triangles of unequal area folded along their shared edge, and a vertex no triangle uses
    strip_v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 3.0, 2.0], [5.0, 5.0, 5.0]])
    strip_f = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    got = F.vertex_normals(strip_v, strip_f)
    ref = _normals_f64(strip_v, strip_f)
    assert float((got.double() - ref).abs().max()) <= 4 * 2.0 ** -24
    assert torch.equal(got[0], torch.tensor([0.0, 0.0, 1.0]))                                       # only the flat triangle
    assert torch.equal(got[4], torch.zeros(3))
    # area weighting: the shared vertices lean towards the larger triangle's normal
    n_small, n_large = torch.tensor([0.0, 0.0, 1.0]).double(), torch.nn.functional.normalize(torch.linalg.cross(
        (strip_v[1] - strip_v[2]).double(), (strip_v[3] - strip_v[2]).double()), dim=0)
    assert float(ref[1] @ n_large) > float(ref[1] @ n_small)
    assert torch.equal(F.vertex_normals(strip_v, strip_f[:, [0, 2, 1]]), -got)                      # orientation follows the winding
    empty = F.vertex_normals(strip_v, torch.zeros((0, 3), dtype=torch.int32))
    assert torch.equal(empty, torch.zeros(5, 3))


# ---- 5. the code object ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(BUILD) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="no build directory / no llvm-readelf")
def test_inverse_bender_kernels_spill_nothing_and_keep_their_layers_under_a_full_exec_mask():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_exec_regions
    import check_isa
    obj = os.path.join(BUILD, "nrnerf_bend_inverse.o")
    if not os.path.exists(obj):
        pytest.skip("csrc/build/nrnerf_bend_inverse.o not built")
    with tempfile.TemporaryDirectory() as tmp:
        co = check_isa.device_code_object(obj, tmp)
        assert co is not None
        notes = subprocess.run([f"{check_isa.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    seen = {}
    for blk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or "bend_inverse_kernel" not in name.group(1):
            continue
        depth = re.search(r"ArchTI(?:Li\d+E){5}Li(\d+)E", name.group(1))              # W, D, SKIP, L, LV, then the bender's depth
        num = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
        assert depth is not None, f"the bender's depth is no longer the sixth parameter of ArchT in {name.group(1)}: adjust the pattern"
        seen[int(depth.group(1))] = dict(vgpr=num("vgpr_count"), vgpr_spill=num("vgpr_spill_count"), sgpr_spill=num("sgpr_spill_count"),
                                         scratch=num("private_segment_fixed_size"))
    print(seen)
    assert sorted(seen) == [5, 7], seen                                               # both bender architectures
    for depth, r in seen.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (depth, r)
        assert r["vgpr"] <= 128, (depth, r, "four workgroups of four waves per CU need <= 128 registers per lane")
    with tempfile.TemporaryDirectory() as only:
        os.symlink(obj, os.path.join(only, "nrnerf_bend_inverse.o"))
        bad, n = check_exec_regions.offending_regions(only)
    assert n == 1 and not bad, "\n".join(bad)
