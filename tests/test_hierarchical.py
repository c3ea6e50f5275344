"""GPU tier of the hierarchical baked render: ``nrnerf_hierarchical_volume_render`` through ``field.hierarchical_volume_render`` /
``render_baked`` / ``render_volume``.

1. the fused kernel returns the bits of the composition it replaces -- (A) ``warped_volume_render`` at S_c with ``raw``, (B)
``nrnerf_composite_forward`` on that raw with n_importance = I, (C) ``warped_volume_render`` at S_c + I at (B)'s merged depths -- over every
output; 2. no warp is an all-zero warp, and ``render_volume`` composes ``volume_render``; 3. the same bits on every run and for a ray whatever
the rays around it; 4. beyond the kernel's bounds, with an ``"sh"`` record and with a mask ``render_baked`` composes; 5. properties of the merged
depths; 6. importance sampling does its job on a thin shell; 7. ``N_importance=0`` is the call it was.

Outputs are compared as int32 views: a NaN counts, +0 and -0 differ."""
import pytest
import torch

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd import field as F
from nonrigid_nerf_amd import render as R
from tests import hierarchical_reference as H
from tests import volume_reference as V
from tests import warp_reference as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO, HI = (-0.5, 0.25, 1.0), (1.5, 1.0, 4.0)                 # the volume's box (tests/test_warp.py): rays from z = 0 cross its near and far faces
WLO, WHI = (-0.1, 0.4, 0.5), (1.1, 1.3, 3.2)                # the warp's: partly overlapping
VOLUMES = [(5, 4, 3), (17, 9, 33)]                          # (Gx, Gy, Gz)
WARPS = [(2, 2, 2), (5, 4, 3)]
DTYPES = [torch.float32, torch.float16]
RAY_COUNTS = [1, 37, 300]                                   # none a multiple of the four waves of a workgroup
# every EPL_C class, the EPL_F classes 1, 2, 3, 4, 8 and the extremes of the dispatch table
PAIRS = [(3, 1), (3, 5), (33, 7), (64, 64), (64, 128), (65, 63), (64, 129), (129, 63), (192, 64), (128, 257), (256, 256)]
FINE_ONLY = ("rgb_map", "disp_map", "acc_map", "raw", "weights", "alpha", "surface_pts", "surface_rigidity", "median_index", "points4")
ALL = dict(retraw=True, weights=True, alpha=True, surface=True, return_points=True)

_cache = {}


def volume(g, dtype):
    key = ("v", g, dtype)
    if key not in _cache:
        _cache[key] = {"raw": V.smooth_volume(*g, seed=sum(g)).to(dtype).to(DEV), "min_point": LO, "max_point": HI}
    return _cache[key]


def warp(g, dtype):
    key = ("w", g, dtype)
    if key not in _cache:
        _cache[key] = {"warp": W.smooth_warp(*g, seed=sum(g), amplitude=0.15).to(dtype).to(DEV), "min_point": WLO, "max_point": WHI}
    return _cache[key]


def crossing_rays(n, seed, near=0.5, far=5.0):
    """``n`` rays that cross the box LO .. HI along +z from in front of it, with different direction lengths: samples before the near face
    and behind the far face are empty."""
    key = ("r", n, seed, near, far)
    if key not in _cache:
        g = torch.Generator().manual_seed(seed)
        o = torch.tensor([0.5, 0.6, 0.0]) + 0.05 * torch.randn(n, 3, generator=g)
        d = (torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(n, 3, generator=g)) * (0.5 + torch.rand(n, 1, generator=g))
        _cache[key] = torch.cat([o, d, torch.full((n, 1), near), torch.full((n, 1), far)], -1).to(DEV)
    return _cache[key]


def sorted_depths(n, s, seed):
    return torch.sort(0.5 + 4.5 * torch.rand(n, s, generator=torch.Generator().manual_seed(seed)), -1).values.to(DEV)


def uniforms(n, i, seed):
    return torch.rand(n, i, generator=torch.Generator().manual_seed(seed)).to(DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_same_bits(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert torch.equal(bits(got[k]), bits(want[k])), (what, k, int((bits(got[k]) != bits(want[k])).sum()))


def composition(render, rays, S, I, z=None, u=None, lindisp=False, white_bkgd=False, **outputs):
    """(A), (B), (C) spelled out over ``render(N_samples=, z_vals=, retraw=, ...)``, under the fused call's keys."""
    first = render(N_samples=S, z_vals=z, retraw=True)
    z_merged, z_std = F.importance_depths(first["raw"], rays, N_importance=I, z_vals=z, importance_u=u, lindisp=lindisp, white_bkgd=white_bkgd)
    out = render(N_samples=S + I, z_vals=z_merged, **outputs)
    out.update(rgb0=first["rgb_map"], disp0=first["disp_map"], acc0=first["acc_map"], z_std=z_std, z_vals=z_merged)
    return out


def warped(vol, wrp, rays, **fixed):
    return lambda **kw: F.warped_volume_render(vol, wrp, rays, **fixed, **kw)


KEYS = FINE_ONLY + ("rgb0", "disp0", "acc0", "z_std", "z_vals")


# ---- 1. fused == (A) -> (B) -> (C), bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=[f"{s}+{i}" for s, i in PAIRS])
def test_fused_equals_the_composition_bit_for_bit(pair):
    S, I = pair
    empty_seen = False
    for n in RAY_COUNTS:
        rays = crossing_rays(n, 7 + n)
        for vg in VOLUMES:
            for wg in WARPS:
                for vd in DTYPES:
                    for wd in DTYPES:
                        vol, wrp = volume(vg, vd), warp(wg, wd)
                        got = F.hierarchical_volume_render(vol, wrp, rays, N_samples=S, N_importance=I, **ALL)
                        want = composition(warped(vol, wrp, rays), rays, S, I, **ALL)
                        assert sorted(got) == sorted(KEYS)
                        assert_same_bits(got, want, KEYS, (n, vg, wg, vd, wd))
                        hit = (got["raw"] != 0).any(-1)
                        empty_seen |= bool((~hit).any()) and bool(hit.any())
    assert empty_seen           # the rays cross the box's faces: some samples are empty, others are not


VARIANTS = {
    "lindisp white_bkgd": dict(lindisp=True, white_bkgd=True),
    "caller's z_vals": dict(z=True),
    "importance_u": dict(u=True),
    "z_vals, importance_u, knobs, surface": dict(z=True, u=True, white_bkgd=True, rigidity_cutoff=0.4, test_time_scaling=1.7, removal_threshold=0.8),
}
VARIANT_SCENES = [(37, (17, 9, 33), torch.float16, (5, 4, 3), torch.float32), (300, (5, 4, 3), torch.float32, (2, 2, 2), torch.float16)]


@pytest.mark.parametrize("pair", [(33, 7), (64, 128), (129, 63), (256, 256)], ids=lambda p: f"{p[0]}+{p[1]}")
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_equals_the_composition_with_depths_uniforms_and_knobs(variant, pair):
    S, I = pair
    kw = dict(VARIANTS[variant])
    for n, vg, vd, wg, wd in VARIANT_SCENES:
        rays = crossing_rays(n, 11 + n)
        vol, wrp = volume(vg, vd), warp(wg, wd)
        z = sorted_depths(n, S, 3 + n) if kw.get("z") else None
        u = uniforms(n, I, 5 + n) if kw.get("u") else None
        fixed = {k: v for k, v in kw.items() if k not in ("z", "u")}
        got = F.hierarchical_volume_render(vol, wrp, rays, N_samples=S, N_importance=I, z_vals=z, importance_u=u, **fixed, **ALL)
        want = composition(warped(vol, wrp, rays, **fixed), rays, S, I, z, u, fixed.get("lindisp", False), fixed.get("white_bkgd", False), **ALL)
        assert_same_bits(got, want, KEYS, (variant, n))
        if "removal_threshold" in fixed:        # the knobs act: the removal knob zeroes some sigma logits, the cutoff some masks
            plain = F.hierarchical_volume_render(vol, wrp, rays, N_samples=S, N_importance=I, z_vals=z, importance_u=u, white_bkgd=True, **ALL)
            assert not torch.equal(plain["raw"], got["raw"]) and not torch.equal(plain["points4"], got["points4"])
    # through render_baked: the same call, both routes
    a = F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, z_vals=z, importance_u=u, retraw=True, surface=True, return_points=True, **fixed)
    b = F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, z_vals=z, importance_u=u, retraw=True, surface=True, return_points=True,
                       fused=False, **fixed)
    keys = tuple(k for k in KEYS if k not in ("weights", "alpha"))
    assert sorted(a) == sorted(b) == sorted(keys)
    assert_same_bits(a, got, keys, "render_baked, fused")
    assert_same_bits(b, got, keys, "render_baked, composed")


# ---- 2. no warp ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(3, 5), (64, 64), (192, 64)], ids=lambda p: f"{p[0]}+{p[1]}")
def test_no_warp_is_an_all_zero_warp_and_render_volume_composes_volume_render(pair):
    S, I = pair
    rays = crossing_rays(37, 21)
    for vg in VOLUMES:
        for vd in DTYPES:
            vol = volume(vg, vd)
            zero = {"warp": torch.zeros(2, 2, 2, 4, device=DEV), "min_point": WLO, "max_point": WHI}
            kw = dict(N_samples=S, N_importance=I, white_bkgd=True, rigidity_cutoff=0.1, test_time_scaling=2.0, **ALL)
            assert_same_bits(F.hierarchical_volume_render(vol, None, rays, **kw), F.hierarchical_volume_render(vol, zero, rays, **kw), KEYS, "zero warp")
            # render_volume: the coarse depths are sample_rays', the composition is over volume_render on straight rays
            z = F.sample_rays(rays, S)[0]

            def straight(N_samples, z_vals, retraw=False, surface=False):
                p4 = None
                if surface:
                    p = rays[:, None, 0:3] + rays[:, None, 3:6] * z_vals[..., None]
                    p4 = torch.cat([p, torch.zeros_like(p[..., :1])], -1)
                return F.volume_render(vol, rays, N_samples=N_samples, z_vals=z_vals, points4=p4, retraw=retraw, surface=surface)
            want = composition(straight, rays, S, I, z, retraw=True, surface=True)
            keys = tuple(k for k in KEYS if k not in ("weights", "alpha", "points4"))
            for fused in (None, True, False):
                got = F.render_volume(vol, rays, N_samples=S, N_importance=I, retraw=True, surface=True, fused=fused)
                assert sorted(got) == sorted(keys)
                assert_same_bits(got, want, keys, ("render_volume", fused))


def test_render_volume_refuses_a_network_between_the_passes():
    with pytest.raises(R.Unsupported):
        F.render_volume(volume(VOLUMES[0], torch.float32), crossing_rays(9, 1), network=object(), N_samples=8, N_importance=4)


# ---- 3. determinism; a ray does not depend on the rays around it ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(33, 7), (64, 128), (128, 257)], ids=lambda p: f"{p[0]}+{p[1]}")
def test_two_calls_agree_and_a_ray_does_not_depend_on_its_neighbours(pair):
    S, I = pair
    rays = crossing_rays(300, 31)
    vol, wrp = volume(VOLUMES[1], torch.float16), warp(WARPS[1], torch.float32)
    u = uniforms(300, I, 9)
    a = F.hierarchical_volume_render(vol, wrp, rays, N_samples=S, N_importance=I, importance_u=u, **ALL)
    b = F.hierarchical_volume_render(vol, wrp, rays, N_samples=S, N_importance=I, importance_u=u, **ALL)
    assert_same_bits(a, b, KEYS, "second call")
    pick = torch.tensor([0, 5, 17, 64, 131, 255, 256, 298, 299], device=DEV)         # 9 rays: other waves, other neighbours, no LDS left over
    few = F.hierarchical_volume_render(vol, wrp, rays[pick].contiguous(), N_samples=S, N_importance=I, importance_u=u[pick].contiguous(), **ALL)
    assert_same_bits(few, {k: v[pick] for k, v in a.items()}, KEYS, "9 of 300")


# ---- 4. beyond the kernel's bounds, "sh" records, masks: the composed route ----------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(257, 10), (64, 449)], ids=lambda p: f"{p[0]}+{p[1]}")
def test_beyond_the_bounds_the_entry_point_refuses_and_render_baked_composes(pair):
    S, I = pair
    rays = crossing_rays(37, 41)
    vol, wrp = volume(VOLUMES[1], torch.float32), warp(WARPS[1], torch.float16)
    with pytest.raises(_lib.NrnerfError) as e:
        F.hierarchical_volume_render(vol, wrp, rays, N_samples=S, N_importance=I)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(R.Unsupported):
        F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, fused=True)
    got = F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, retraw=True, surface=True, return_points=True)
    want = composition(warped(vol, wrp, rays), rays, S, I, retraw=True, surface=True, return_points=True)
    keys = tuple(k for k in KEYS if k not in ("weights", "alpha"))
    assert sorted(got) == sorted(keys)
    assert_same_bits(got, want, keys, "composed")


@pytest.mark.parametrize("pair", [(33, 7), (64, 128)], ids=lambda p: f"{p[0]}+{p[1]}")
def test_sh_records_and_masks_take_the_composed_route(pair):
    S, I = pair
    rays = crossing_rays(37, 43)
    vol, wrp = volume(VOLUMES[1], torch.float32), warp(WARPS[1], torch.float32)
    keys = tuple(k for k in KEYS if k not in ("weights", "alpha"))
    outs = dict(retraw=True, surface=True, return_points=True)
    # a mask
    occ = F.build_occupancy(vol, block=4)
    got = F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, occupancy=occ, **outs)
    want = composition(lambda **kw: F.warped_volume_render(vol, wrp, rays, occupancy=occ, **kw), rays, S, I, **outs)
    assert_same_bits(got, want, keys, "occupancy")
    with pytest.raises(R.Unsupported):
        F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I, occupancy=occ, fused=True)
    # a view-dependent record
    g = torch.Generator().manual_seed(3)
    sh = dict(vol, sh=(0.3 * torch.randn(tuple(vol["raw"].shape[:3]) + (F.sh_channels(1),), generator=g)).to(DEV), sh_degree=1)
    got = F.render_baked(sh, wrp, rays, N_samples=S, N_importance=I, **outs)
    want = composition(lambda **kw: F.sh_volume_render(sh, rays, warp=wrp, **kw), rays, S, I, **outs)
    assert_same_bits(got, want, keys, "sh")
    assert not torch.equal(got["rgb_map"], F.render_baked(vol, wrp, rays, N_samples=S, N_importance=I)["rgb_map"])
    got = F.render_volume(sh, rays, N_samples=S, N_importance=I, occupancy=occ)
    assert sorted(got) == sorted(("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std", "z_vals"))


# ---- 5. the merged depths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(3, 5), (33, 7), (64, 128), (129, 63)], ids=lambda p: f"{p[0]}+{p[1]}")
def test_properties_of_the_merged_depths(pair):
    S, I = pair
    n = 37
    rays = crossing_rays(n, 51)
    vol, wrp = volume(VOLUMES[1], torch.float32), warp(WARPS[1], torch.float32)
    zc = F.sample_rays(rays, S)[0]
    for u in (None, uniforms(n, I, 13)):
        out = F.hierarchical_volume_render(vol, wrp, rays, N_samples=S, N_importance=I, z_vals=zc, importance_u=u)
        zv, z0 = out["z_vals"].cpu(), zc.cpu()
        assert bool((zv[:, 1:] >= zv[:, :-1]).all())                                # non-decreasing
        mids = 0.5 * (z0[:, 1:] + z0[:, :-1])
        new = []
        for r in range(n):
            coarse, rest, j = z0[r].tolist(), [], 0
            for v in zv[r].tolist():                                                # the merge is stable: the coarse depths come first among equals
                if j < S and v == coarse[j]:
                    j += 1
                else:
                    rest.append(v)
            assert j == S and len(rest) == I, (r, j, len(rest))                     # every coarse depth is there; what is left: the I new ones
            assert all(float(mids[r, 0]) <= v <= float(mids[r, -1]) for v in rest), r
            new.append(rest)
        std = torch.tensor(new, dtype=torch.float64).std(-1, unbiased=False)
        got = out["z_std"].cpu().double()
        print(f"  {S} + {I}, u {'given' if u is not None else 'linspace'}: max |z_std - std| / std = {float(((got - std).abs() / std).max()):.2e}")
        assert bool(((got - std).abs() <= 1e-6 * std).all())


# ---- 6. importance sampling does its job -----------------------------------------------------------------------------------------------------------
def test_importance_sampling_beats_uniform_sampling_on_a_thin_shell():
    """A Gaussian density shell (tests/hierarchical_reference.py) baked analytically into 48^3: mean |acc_map| and |rgb_map| error against a
    1024-sample uniform render, 32 + 32 hierarchical against 64 uniform.  The shell's width was chosen with the float64 model
    (tests/test_hierarchical_host.py), which shows a factor 31.4 on acc_map (3.32e-3 against 1.06e-4) and 6.3 on rgb_map (1.03e-2 against
    1.62e-3); measured on the device: 31.4 (3.321e-3 / 1.059e-4) and 6.3 (1.025e-2 / 1.623e-3).  Asserted: the strict inequality alone."""
    vol = {"raw": H.shell_volume().to(DEV), "min_point": H.SHELL_BOX[0], "max_point": H.SHELL_BOX[1]}
    rays = H.shell_rays().to(DEV)
    truth = F.render_volume(vol, rays, N_samples=1024)
    uniform = F.render_volume(vol, rays, N_samples=64)
    hier = F.render_volume(vol, rays, N_samples=32, N_importance=32)
    eu, eh = H.mean_abs_errors(uniform, truth), H.mean_abs_errors(hier, truth)
    print(f"mean |acc - truth|: 64 uniform {eu[0]:.3e}, 32 + 32 {eh[0]:.3e} (factor {eu[0] / eh[0]:.2f}); "
          f"mean |rgb - truth|: 64 uniform {eu[1]:.3e}, 32 + 32 {eh[1]:.3e} (factor {eu[1] / eh[1]:.2f})")
    assert eh[0] < eu[0] and eh[1] < eu[1]


# ---- 7. N_importance = 0 is the call it was --------------------------------------------------------------------------------------------------------
def test_without_importance_samples_nothing_changes():
    rays = crossing_rays(37, 61)
    vol, wrp = volume(VOLUMES[1], torch.float16), warp(WARPS[1], torch.float32)
    kw = dict(N_samples=33, white_bkgd=True, rigidity_cutoff=0.3, retraw=True, surface=True, return_points=True)
    want = F.warped_volume_render(vol, wrp, rays, **kw)
    for extra in (dict(), dict(N_importance=0), dict(N_importance=0, importance_u=None, fused=False)):
        got = F.render_baked(vol, wrp, rays, **kw, **extra)
        assert sorted(got) == sorted(want)
        assert_same_bits(got, want, tuple(want), extra)
    z = F.sample_rays(rays, 33)[0]
    want = F.volume_render(vol, rays, N_samples=33, z_vals=z, retraw=True)
    for extra in (dict(), dict(N_importance=0)):
        got = F.render_volume(vol, rays, N_samples=33, retraw=True, **extra)
        assert sorted(got) == sorted(want)
        assert_same_bits(got, want, tuple(want), extra)
