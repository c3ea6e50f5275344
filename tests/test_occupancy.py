"""GPU tier of the occupancy masks: ``nrnerf_occupancy_build`` through ``field.build_occupancy`` and ``nrnerf_culled_volume_render`` through
``occupancy=`` of ``render_baked`` / ``render_volume`` / ``warped_volume_render`` / ``sh_volume_render``.

1. the built mask IS the numpy rule's (tests/occupancy_reference.py), ``==``; 2. exactness: with a mask built at threshold 0 every composited
output, the weights, alpha, the surface outputs and points4 are the UNMASKED calls' bits, ``raw`` is theirs in occupied blocks and zero in
empty ones -- and the float64 reference says the cases are not vacuous; 3. all-ones and all-zero masks; 4. the lossy mode against the masked
float64 reference, within 10 x the float32 reference's own error; 5. the lookup kernel, two runs; 6. refusals, and ``occupancy=None`` is the
path it was."""
import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import field as F
from tests import occupancy_reference as OC
from tests import sh_reference as SH
from tests import volume_reference as V
from tests import warp_reference as W
from tests.test_warp import DEV, DTYPES, HI, LO, WHI, WLO, bar, bits_same, crossing_rays, same, sorted_depths, warp

pytestmark = pytest.mark.gpu
GRID = (17, 17, 33)             # (Gx, Gy, Gz): 16 x 16 x 32 cells, 4 x 4 x 8 blocks at block 4
BLOCK = 4
WARP = (5, 4, 3)
MAPS = ("rgb_map", "disp_map", "acc_map", "weights", "alpha")
ALL = dict(retraw=True, weights=True, alpha=True, surface=True, return_points=True)
PATHS = ("warp", "points4", "straight")


def epl_of(s):
    """csrc/nrnerf_kernels.h's ``epl_class`` restated: the lane width of a ray of ``s`` samples."""
    n = (s + 63) // 64
    return n if n <= 4 else 6 if n <= 6 else 8 if n <= 8 else 12 if n <= 12 else 16


# (rays, samples): one S per lane width (EPL 1, 1, 2, 3, 4, 6, 8, 12, 16 by csrc/nrnerf_kernels.h's table: 385 is the one of EPL 8, as
# tests/test_sh.py has it), 3 to 37 rays
SHAPES = [(37, 2), (37, 33), (37, 65), (37, 130), (37, 193), (3, 257), (3, 385), (3, 513), (3, 769)]
assert [epl_of(s) for _, s in SHAPES] == [1, 1, 2, 3, 4, 6, 8, 12, 16]
# the seed of a shape's rays (1 unless named): one at which, by the float64 reference alone, every case of the shape has a quarter of its
# in-box samples in empty blocks, a quarter in occupied ones, and a ray that meets the blob (asserted per case on the CPU)
RAY_SEED = {(3, 513): 5, (3, 769): 2}

_records = {}


def record_cpu(degree, dtype):
    """The CPU copies of a record's raw and sh (None at degree 0) in the storage dtype: the blob volume, test_sh.py's coefficients."""
    vcpu = OC.blob_volume(*GRID, seed=3, centre=(0.5, 0.45, 0.5), radius=0.3, shell=0.1).to(dtype)
    if degree == 0:
        return vcpu, None
    sh = SH.smooth_sh(*GRID, 2, seed=5)[..., :12 * degree].clone()
    if degree == 1:
        sh[..., 9:] = 0
    return vcpu, sh.to(dtype)


def record(degree, dtype):
    """(the volume record on the device, the CPU copies of raw and sh, the exact mask's record, its boolean block grid); built once."""
    key = (degree, dtype)
    if key not in _records:
        vcpu, sh = record_cpu(degree, dtype)
        rec = {"raw": vcpu.to(DEV), "min_point": LO, "max_point": HI}
        if sh is not None:
            rec.update(sh=sh.to(DEV), sh_degree=degree)
        _records[key] = (rec, vcpu, sh, F.build_occupancy(rec, block=BLOCK), OC.mask_reference(vcpu, BLOCK))
    return _records[key]


def case_inputs(shape, path, wdtype=torch.float32):
    """rays, explicit depths (None on the straight path: the coarse spacing), the warp's CPU grid or None, points4 or None."""
    n, s = shape
    rays = crossing_rays(n, RAY_SEED.get(shape, 1) + s)
    z = None if path == "straight" and s > 2 else sorted_depths(n, s, 11 + n + s)          # (two samples of the coarse spacing: near and far, outside the box)
    wcpu = p4 = None
    if path != "straight":
        wcpu = W.smooth_warp(*WARP, seed=sum(WARP), amplitude=0.15).to(wdtype)            # (tests/test_warp.py's warp)
    if path == "points4":
        p4 = W.bend_reference(wcpu, WLO, WHI, W.sample_points(rays, z, torch.float32), dtype=torch.float32)
    return rays, z, wcpu, p4


def reference(vcpu, shcpu, degree, occ, shape, path, rays, z, wcpu, p4, dtype=torch.float64, **kw):
    zz = V.coarse_depths(rays, shape[1], kw.pop("lindisp", False), dtype) if z is None else z
    src = dict(warp=wcpu, warp_min=WLO, warp_max=WHI) if path == "warp" else dict(points4=p4) if path == "points4" else {}
    return OC.render_reference(vcpu, shcpu, degree, LO, HI, rays, zz, occ=occ, block=BLOCK, dtype=dtype, **src, **kw)


def run(rec, degree, rays, s, z, wdtype, p4, path, occupancy, **kw):
    """The call of the public layer that serves (degree, path): masked with ``occupancy``, today's with None."""
    dev = lambda t: None if t is None else t.to(DEV)
    if degree:
        out = F.sh_volume_render(rec, dev(rays), N_samples=s, z_vals=dev(z), warp=warp(WARP, wdtype)[0] if path == "warp" else None,
                                 points4=dev(p4) if path == "points4" else None, occupancy=occupancy, **kw)
    elif path == "warp":
        out = F.warped_volume_render(rec, warp(WARP, wdtype)[0], dev(rays), N_samples=s, z_vals=dev(z), occupancy=occupancy, **kw)
    elif occupancy is not None:
        out = F.culled_volume_render(rec, dev(rays), occupancy=occupancy, N_samples=s, z_vals=dev(z), points4=dev(p4), **kw)
    else:           # today's degree-0 call on ready-made points / straight rays: volume_render (no points4 output; surface needs points4)
        kw = {k: v for k, v in kw.items() if k not in ("return_points", "rigidity_cutoff", "test_time_scaling")}
        if p4 is None:
            kw.pop("surface", None), kw.pop("removal_threshold", None)
        out = F.volume_render(rec, dev(rays), N_samples=s, z_vals=dev(z), points4=dev(p4), **kw)
    torch.cuda.synchronize()
    return out


# ---- 1. the mask ---------------------------------------------------------------------------------------------------------------------------------
def awkward_grid(gx, gy, gz, seed):
    """Sigma logits negative but for a sprinkle of positive vertices (1 % and three more: blocks of either kind exist at blocks of 2 and 4),
    colours of a few units."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(gz, gy, gx, 4, generator=g)
    positive = torch.rand(gz, gy, gx, generator=g) < 0.01 + 3.0 / (gx * gy * gz)
    v[..., 3] = torch.where(positive, v[..., 3].abs() + 0.01, -v[..., 3].abs())
    return v


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("block", [2, 4, 8, 16])
@pytest.mark.parametrize("g", [(9, 10, 11), (6, 5, 4), (33, 33, 33), (2, 2, 2)], ids=["9x10x11", "6x5x4", "33^3", "2^3"])
def test_build_occupancy_is_the_numpy_rule(g, block, storage):
    cpu = awkward_grid(*g, seed=sum(g)).to(DTYPES[storage])
    for threshold in (0.0, 0.75):
        want = OC.mask_reference(cpu, block, threshold)
        got = F.build_occupancy(cpu.to(DEV), block=block, threshold=threshold)
        again = F.build_occupancy({"raw": cpu.to(DEV), "min_point": LO, "max_point": HI}, block=block, threshold=threshold)
        assert got["block"] == block and got["grid"] == (g[2], g[1], g[0]) and got["threshold"] == threshold
        assert got["bits"].dtype == torch.int32 and got["bits"].device.type == "cuda"
        assert np.array_equal(got["bits"].cpu().numpy(), OC.pack_bits(want)), (g, block, threshold)
        assert torch.equal(got["bits"], again["bits"])                              # two runs, a bare grid and a record: the same bits
    if g != (2, 2, 2) and (block == 2 or (block == 4 and g != (6, 5, 4))):
        exact = OC.mask_reference(cpu, block)
        assert exact.any() and not exact.all()                                      # (both kinds of block exist: a condition of the inputs)


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("channel,value", [(3, float("nan")), (3, float("inf")), (3, float("-inf")), (0, float("nan")), (2, float("-inf"))],
                         ids=["sigma NaN", "sigma +inf", "sigma -inf", "red NaN", "blue -inf"])
def test_build_occupancy_marks_what_is_not_finite(channel, value, storage):
    cpu = torch.full((11, 10, 9, 4), -1.0)
    cpu[5, 4, 2, channel] = value                   # y = 4: on the face between two blocks of 4
    cpu[10, 9, 8, channel] = value                  # the grid's last vertex
    cpu = cpu.to(DTYPES[storage])
    for block in (2, 4, 16):
        want = OC.mask_reference(cpu, block, 3.0)
        assert want.sum() == {2: 5, 4: 3, 16: 1}[block]
        got = F.build_occupancy(cpu.to(DEV), block=block, threshold=3.0)
        assert np.array_equal(got["bits"].cpu().numpy(), OC.pack_bits(want))


# ---- 2. exactness ----------------------------------------------------------------------------------------------------------------------------------
def check_exact(degree, storage, path, shape, coarse=False, **knobs):
    """``coarse``: the warp path without explicit depths, the coarse spacing between near and far (what reads ``lindisp``)."""
    dtype = DTYPES[storage]
    rec, vcpu, shcpu, mask, occ = record(degree, dtype)
    n, s = shape
    rays, z, wcpu, p4 = case_inputs(shape, path, dtype)
    if coarse:
        assert path == "warp"
        z = None
    ref_knobs = {k: v for k, v in knobs.items() if k in ("white_bkgd", "lindisp", "rigidity_cutoff", "test_time_scaling", "removal_threshold")}
    # from the float64 reference alone: the case is not vacuous
    ref = reference(vcpu, shcpu, degree, occ, shape, path, rays, z, wcpu, p4, **ref_knobs)
    inside, hit = ref["inside"], ref["occupied"]
    n_in, n_skip, n_keep = int(inside.sum()), int((inside & ~hit).sum()), int((inside & hit).sum())
    print(f"[degree {degree} {storage} {path} {shape} {knobs}] {n_in} of {inside.numel()} samples in the box: {n_skip} in empty blocks, "
          f"{n_keep} in occupied ones; acc_map up to {float(ref['acc_map'].max()):.3f}")
    assert n_skip >= 0.25 * n_in and n_keep >= 0.25 * n_in and n_in > 0
    assert float(ref["acc_map"].max()) > 0.5
    want = run(rec, degree, rays, s, z, dtype, p4, path, None, **knobs, **ALL)
    got = run(rec, degree, rays, s, z, dtype, p4, path, mask, **knobs, **ALL)
    for k in want:
        if k == "raw":
            continue
        assert torch.equal(got[k], want[k]) or (k == "disp_map" and bits_same(got[k], want[k])), k         # (disp_map of a ray that hits nothing: NaN)
    for k in MAPS[:1] + MAPS[2:]:
        assert bool(torch.isfinite(got[k]).all()), k
    # raw: the unmasked call's in occupied blocks, the empty sample's in empty ones -- by the float32 cell of the kernel's own points4
    p4_dev = got["points4"].cpu() if "points4" in got else (p4 if p4 is not None else ref["points4"].float())
    _, hit32 = OC.sample_state(occ, BLOCK, GRID, LO, HI, p4_dev[..., :3], torch.float32)
    g_raw, w_raw = got["raw"].cpu(), want["raw"].cpu()
    assert torch.equal(g_raw[hit32], w_raw[hit32])
    assert torch.equal(g_raw[~hit32], torch.zeros_like(g_raw[~hit32]))
    assert bool((w_raw[~hit32] != 0).any())                     # (the unmasked call did have something there)
    assert set(want) <= set(got)           # (volume_render, today's degree-0 call without a warp, has no points4 and, on straight rays, no surface outputs)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{s}" for n, s in SHAPES])
def test_an_exact_mask_keeps_every_composited_bit(shape, degree, storage, path):
    check_exact(degree, storage, path, shape)


@pytest.mark.parametrize("degree", [0, 2])
@pytest.mark.parametrize("knob", [dict(rigidity_cutoff=0.2), dict(test_time_scaling=1.5), dict(removal_threshold=0.3), dict(white_bkgd=True),
                                  dict(lindisp=True)], ids=["cutoff", "scaling", "removal", "white_bkgd", "lindisp"])
def test_an_exact_mask_keeps_every_bit_under_each_knob(knob, degree):
    check_exact(degree, "f32", "warp", (37, 65), coarse="lindisp" in knob, **knob)           # (lindisp is read with the coarse spacing only)


# ---- 3. all-ones and all-zero masks ------------------------------------------------------------------------------------------------------------------
def mask_like(mask, fill):
    words = np.zeros(mask["bits"].numel(), dtype=np.int32) if not fill else OC.pack_bits(np.ones(tuple(OC.blocks(g, BLOCK) for g in mask["grid"]), dtype=bool))
    return dict(mask, bits=torch.from_numpy(words).to(DEV))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("S", [33, 193, 385, 769])
def test_an_all_ones_mask_is_the_unmasked_call_raw_included(S, degree, path):
    rec, _, _, mask, _ = record(degree, torch.float32)
    rays, z, wcpu, p4 = case_inputs((5, S), path)
    want = run(rec, degree, rays, S, z, torch.float32, p4, path, None, **ALL)
    got = run(rec, degree, rays, S, z, torch.float32, p4, path, mask_like(mask, True), **ALL)
    for k in want:
        assert same(got[k], want[k]), k
    assert bool((got["raw"] != 0).any())


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("degree", [0, 2])
def test_an_all_zero_mask_renders_the_background(degree, white):
    rec, _, _, mask, _ = record(degree, torch.float32)
    rays, z, wcpu, p4 = case_inputs((7, 65), "warp")
    got = run(rec, degree, rays, 65, z, torch.float32, p4, "warp", mask_like(mask, False), white_bkgd=white, **ALL)
    assert torch.equal(got["acc_map"], torch.zeros_like(got["acc_map"])) and not bool(got["raw"].any()) and not bool(got["weights"].any())
    assert torch.equal(got["rgb_map"], torch.full_like(got["rgb_map"], 1.0 if white else 0.0))


# ---- 4. the lossy mode against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("degree", [0, 2])
def test_a_lossy_mask_matches_the_masked_float64_reference(degree, path):
    """Tolerances: 10 x the maximum error of the SAME masked reference evaluated in float32 on the same inputs, computed here and printed; the
    seed is one at which the float32 reference alone picks the float64 reference's median sample on every ray (asserted)."""
    rec, vcpu, shcpu, exact, occ0 = record(degree, torch.float32)
    threshold = 5.0                                                 # (the blob's logits reach 7: its thin rim goes)
    occ = OC.mask_reference(vcpu, BLOCK, threshold)
    assert occ.sum() < occ0.sum() and occ.any()                     # (it does drop blocks the exact mask keeps)
    mask = F.build_occupancy(rec, block=BLOCK, threshold=threshold)
    assert np.array_equal(mask["bits"].cpu().numpy(), OC.pack_bits(occ))
    shape = (37, 65)
    n, s = shape
    rays, z, wcpu, p4 = case_inputs(shape, path)
    kw = dict(white_bkgd=True, removal_threshold=0.3 if path != "straight" else None)
    ref64 = reference(vcpu, shcpu, degree, occ, shape, path, rays, z, wcpu, p4, **kw)
    ref32 = reference(vcpu, shcpu, degree, occ, shape, path, rays, z, wcpu, p4, dtype=torch.float32, **kw)
    assert torch.equal(ref32["median_index"], ref64["median_index"]), "pick another seed for this case"
    exact64 = reference(vcpu, shcpu, degree, occ0, shape, path, rays, z, wcpu, p4, **kw)
    print(f"[degree {degree} {path}] threshold {threshold}: rgb_map moves by up to {float((ref64['rgb_map'] - exact64['rgb_map']).abs().max()):.3e} "
          f"against the exact mask")
    assert float((ref64["rgb_map"] - exact64["rgb_map"]).abs().max()) > 1e-3           # (lossy: the picture does change)
    got = {k: v.cpu() for k, v in run(rec, degree, rays, s, z, torch.float32, p4, path, mask, **kw, **ALL).items()}
    for k in ("points4", "raw") + MAPS:
        tol = bar(ref64[k], ref32[k], k)
        g64, r64 = got[k].double(), ref64[k]
        both = torch.isfinite(g64) & torch.isfinite(r64)
        if k != "disp_map":
            assert bool(both.all()), k
        worst = float((g64 - r64)[both].abs().max()) if bool(both.any()) else 0.0
        print(f"  {k}: kernel max error {worst:.3e}")
        assert worst <= tol, k
    assert torch.equal(got["median_index"].long(), ref64["median_index"])
    for k in ("surface_pts", "surface_rigidity"):
        tol = bar(ref64[k], ref32[k], k)
        worst = float((got[k].double() - ref64[k]).abs().max())
        print(f"  {k}: kernel max error {worst:.3e}")
        assert worst <= tol, k


# ---- 5. the lookup kernel, two runs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("S", [2, 65, 193, 385, 513, 1024])
def test_lookup_kernel_and_two_runs_give_the_same_bits(S, degree, storage):
    rec, _, _, mask, _ = record(degree, DTYPES[storage])
    wrp, _ = warp(WARP, torch.float16 if S % 2 else torch.float32)
    rays = crossing_rays(5, S).to(DEV)
    knobs = dict(rigidity_cutoff=0.2, test_time_scaling=1.5, removal_threshold=0.3)
    call = lambda **kw: F.culled_volume_render(rec, rays, occupancy=mask, N_samples=S, **kw)
    for z in (sorted_depths(5, S, S).to(DEV), None):
        fused = call(z_vals=z, warp=wrp, white_bkgd=z is None, **knobs, **ALL)
        again = call(z_vals=z, warp=wrp, white_bkgd=z is None, **knobs, **ALL)
        split = call(z_vals=z, points4=fused["points4"], white_bkgd=z is None, removal_threshold=0.3, **ALL)
        alone = call(z_vals=z, warp=wrp, composite=False, retraw=True, return_points=True, **knobs)
        alone_p4 = call(z_vals=z, points4=fused["points4"], composite=False, retraw=True, removal_threshold=0.3)
        a = call(z_vals=z, retraw=True)
        b = call(z_vals=z, composite=False)
        torch.cuda.synchronize()
        assert bits_same(a["raw"], b["raw"]), "straight"
        assert sorted(fused) == sorted(split) == sorted(again)
        for k in fused:
            eq = torch.equal if k == "median_index" else bits_same
            assert eq(fused[k], again[k]), ("two runs", k)
            assert eq(fused[k], split[k]), ("own points4", k)
        assert sorted(alone) == ["points4", "raw"] and bits_same(alone["raw"], fused["raw"]) and bits_same(alone["points4"], fused["points4"])
        assert bits_same(alone_p4["raw"], fused["raw"])
        assert bool((fused["raw"] != 0).any()) and bool((fused["raw"] == 0).all(-1).any())


# ---- 6. the python layer -----------------------------------------------------------------------------------------------------------------------------
def test_the_frames_wrappers_and_render_volume_take_the_mask():
    rec, _, _, mask, _ = record(1, torch.float32)
    plain = {k: v for k, v in rec.items() if k not in ("sh", "sh_degree")}
    rays = crossing_rays(9, 4).to(DEV)
    for r in (rec, plain):
        m = F.build_occupancy(r, block=BLOCK)
        assert torch.equal(m["bits"], mask["bits"])
        for surface in (False, True):
            want = F.render_volume(r, rays, N_samples=65, surface=surface, retraw=True)
            got = F.render_volume(r, rays, N_samples=65, surface=surface, retraw=True, occupancy=m)
            assert sorted(got) == sorted(want)
            for k in want:
                if k != "raw":
                    assert bits_same(got[k], want[k]), k
            assert not torch.equal(got["raw"], want["raw"])
    poses = [torch.tensor([[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, 0.6], [0.0, 0.0, 1.0, 6.0]]) for _ in range(2)]      # looking down -z at the box
    intr = dict(height=6, width=8, focal_x=20.0, focal_y=20.0, center_x=4.0, center_y=3.0)
    wrp = warp(WARP)[0]
    for r in (rec, plain):
        a = F.render_baked_frames(r, wrp, poses, intr, 1.0, 6.0, N_samples=33)
        b = F.render_baked_frames(r, wrp, poses, intr, 1.0, 6.0, N_samples=33, occupancy=mask)
        assert torch.equal(a[0], b[0]) and bits_same(a[1], b[1]) and int(a[0].max()) > 0
        a = F.render_volume_frames(r, poses, intr, 1.0, 6.0, N_samples=33)
        b = F.render_volume_frames(r, poses, intr, 1.0, 6.0, N_samples=33, occupancy=mask)
        assert torch.equal(a[0], b[0]) and bits_same(a[1], b[1]) and int(a[0].max()) > 0


def test_without_a_mask_the_calls_are_what_they_were():
    """``occupancy=None`` (and no argument at all) are the same call: every key ``==``."""
    for degree in (0, 2):
        rec, _, _, _, _ = record(degree, torch.float32)
        rays = crossing_rays(5, 9).to(DEV)
        wrp = warp(WARP)[0]
        kw = dict(N_samples=65, surface=True, retraw=True, return_points=True, removal_threshold=0.3)
        a, b = F.render_baked(rec, wrp, rays, **kw), F.render_baked(rec, wrp, rays, occupancy=None, **kw)
        assert sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
        a, b = F.render_volume(rec, rays, N_samples=65, surface=True), F.render_volume(rec, rays, N_samples=65, surface=True, occupancy=None)
        assert sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
        if degree:
            a, b = F.sh_volume_render(rec, rays, warp=wrp, **kw), F.sh_volume_render(rec, rays, warp=wrp, occupancy=None, **kw)
        else:
            a, b = F.warped_volume_render(rec, wrp, rays, **kw), F.warped_volume_render(rec, wrp, rays, occupancy=None, **kw)
        assert sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)


def test_refusals():
    rec, vcpu, _, mask, _ = record(2, torch.float32)
    rays = crossing_rays(3, 1).to(DEV)
    wrp = warp(WARP)[0]
    with pytest.raises(ValueError):
        F.build_occupancy(rec, threshold=-0.5)
    with pytest.raises(ValueError):
        F.build_occupancy(rec, threshold=float("nan"))
    for bad in (3, 1, 32, 0):
        with pytest.raises(ValueError):
            F.build_occupancy(rec, block=bad)
    sh = rec["sh"].clone()
    sh[3, 2, 1, 5] = float("inf")
    with pytest.raises(ValueError):
        F.build_occupancy(dict(rec, sh=sh))
    sh[3, 2, 1, 5] = float("nan")
    with pytest.raises(ValueError):
        F.build_occupancy(dict(rec, sh=sh))
    # a mask of another grid
    other = F.build_occupancy(torch.full((33, 17, 18, 4), -1.0, device=DEV), block=BLOCK)
    for call in (lambda m: F.render_baked(rec, wrp, rays, N_samples=5, occupancy=m), lambda m: F.render_volume(rec, rays, N_samples=5, occupancy=m),
                 lambda m: F.sh_volume_render(rec, rays, N_samples=5, occupancy=m),
                 lambda m: F.warped_volume_render(rec, wrp, rays, N_samples=5, occupancy=m)):
        with pytest.raises(ValueError):
            call(other)
        with pytest.raises(ValueError):
            call(dict(mask, bits=mask["bits"][:-1]))
        with pytest.raises(ValueError):
            call(dict(mask, bits=mask["bits"].to(torch.int64)))
        with pytest.raises(ValueError):
            call(dict(mask, block=8))                           # (the word count of another block size)
        assert "rgb_map" in call(mask)
    # the autograd path takes no mask
    for fn in (F.render_baked_train, F.refine_bake, F.grid_lookup):
        import inspect
        assert "occupancy" not in inspect.signature(fn).parameters
