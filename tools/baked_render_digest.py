#!/usr/bin/env python
"""The bits of the baked render kernels, as digests: every family (baked volume, baked warp, view-dependent bake of degree 1 / 2, the same
behind an occupancy mask at degree 0 / 1 / 2, hierarchical sampling) on small seeded inputs -- a 17 x 17 x 33 volume, a 9^3 warp, 37 rays --
at one sample count per lane width (2, 65, 130, 193, 257, 385, 513, 769), both storage types of each grid, every point source, each
test-time knob on once, and the lookup-only calls.  One line per case: its name, then ``output=SHA-256`` of every tensor the call returned.
These kernels have no atomics and every sum is spelled out, so two builds of the library that compute the same thing print the same text:
    NRNERF_LIB=<one library> python tools/baked_render_digest.py > a.txt
    NRNERF_LIB=<another>     python tools/baked_render_digest.py > b.txt && cmp a.txt b.txt
(profiles/baked_render_digest.txt holds the record.)  The whole run takes seconds."""
import hashlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from nonrigid_nerf_amd import field as F  # noqa: E402

SAMPLES = (2, 65, 130, 193, 257, 385, 513, 769)            # lane widths 1, 2, 3, 4, 6, 8, 12, 16
HIERARCHICAL = ((40, 30), (100, 93), (150, 150), (200, 250))          # coarse lane widths 1 .. 4, merged 2, 4, 6, 8
N_RAYS = 37
ALL = dict(retraw=True, weights=True, alpha=True, surface=True, return_points=True)
DTYPES = (torch.float32, torch.float16)
NAME = {torch.float32: "f32", torch.float16: "f16"}


def inputs(dev):
    g = torch.Generator().manual_seed(20240521)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    raw = rnd(33, 17, 17, 4)
    z, y, x = torch.meshgrid(torch.linspace(-1, 1, 33), torch.linspace(-1, 1, 17), torch.linspace(-1, 1, 17), indexing="ij")
    raw[..., 3] = torch.where(x * x + y * y + z * z < 0.5, 2.0 * raw[..., 3] + 1.0, -raw[..., 3].abs() - 0.1)       # empty blocks outside a ball
    sh = 0.5 * rnd(33, 17, 17, 24)
    warp = torch.cat([0.1 * rnd(9, 9, 9, 3), torch.rand(9, 9, 9, 1, generator=g)], -1)
    o = torch.tensor([0.1, -0.2, -2.0]) + 0.05 * rnd(N_RAYS, 3)
    d = torch.tensor([0.0, 0.0, 1.0]) + 0.35 * rnd(N_RAYS, 3)
    rays = torch.cat([o, d, torch.full((N_RAYS, 1), 0.5), torch.full((N_RAYS, 1), 3.5)], -1)
    box = dict(min_point=(-1.0, -1.0, -1.0), max_point=(1.0, 1.0, 1.0))
    wbox = dict(min_point=(-1.2, -1.2, -1.2), max_point=(1.2, 1.2, 1.2))
    vols = {t: dict(box, raw=raw.to(dev, t)) for t in DTYPES}
    shs = {(t, deg): dict(box, raw=raw.to(dev, t), sh=sh[..., :12 * deg].to(dev, t).contiguous(), sh_degree=deg) for t in DTYPES for deg in (1, 2)}
    warps = {t: dict(wbox, warp=warp.to(dev, t)) for t in DTYPES}
    u = torch.rand(N_RAYS, 512, generator=g)
    return vols, shs, warps, rays.to(dev), g, u


def emit(name, out):
    torch.cuda.synchronize()
    parts = [f"{k}={hashlib.sha256(out[k].contiguous().cpu().numpy().tobytes()).hexdigest()}" for k in sorted(out)]
    print(name, *parts, flush=True)


def main():
    dev = torch.device("cuda:0")
    vols, shs, warps, rays, g, u = inputs(dev)
    occ = {t: F.build_occupancy(vols[t], block=2) for t in DTYPES}
    no_points = {k: v for k, v in ALL.items() if k != "return_points"}
    for S in SAMPLES:
        points4 = (torch.cat([1.3 * torch.rand(N_RAYS, S, 3, generator=g) * 2 - 1.3, torch.rand(N_RAYS, S, 1, generator=g)], -1)).to(dev)
        for vt in DTYPES:
            v = NAME[vt]
            emit(f"volume S={S} vol={v} straight", F.volume_render(vols[vt], rays, N_samples=S, retraw=True, weights=True, alpha=True))
            emit(f"volume S={S} vol={v} points4", F.volume_render(vols[vt], rays, N_samples=S, points4=points4, **no_points))
            emit(f"culled0 S={S} vol={v} straight", F.culled_volume_render(vols[vt], rays, occupancy=occ[vt], N_samples=S, **ALL))
            emit(f"culled0 S={S} vol={v} points4", F.culled_volume_render(vols[vt], rays, occupancy=occ[vt], N_samples=S, points4=points4, **ALL))
            for wt in DTYPES:
                w = NAME[wt]
                emit(f"warp S={S} vol={v} warp={w}", F.warped_volume_render(vols[vt], warps[wt], rays, N_samples=S, **ALL))
                emit(f"culled0 S={S} vol={v} warp={w}", F.culled_volume_render(vols[vt], rays, occupancy=occ[vt], warp=warps[wt], N_samples=S, **ALL))
                for deg in (1, 2):
                    rec = shs[vt, deg]
                    emit(f"sh{deg} S={S} vol={v} warp={w}", F.sh_volume_render(rec, rays, N_samples=S, warp=warps[wt], **ALL))
                    emit(f"culled{deg} S={S} vol={v} warp={w}", F.culled_volume_render(rec, rays, occupancy=occ[vt], warp=warps[wt], N_samples=S, **ALL))
            for deg in (1, 2):
                rec = shs[vt, deg]
                for call, kw in (("sh", {}), ("culled", dict(occupancy=occ[vt]))):
                    fn = F.sh_volume_render if call == "sh" else F.culled_volume_render
                    emit(f"{call}{deg} S={S} vol={v} straight ray-directions", fn(rec, rays, N_samples=S, **ALL, **kw))
                    emit(f"{call}{deg} S={S} vol={v} points4", fn(rec, rays, N_samples=S, points4=points4, **ALL, **kw))
    # ---- the knobs, each on once, and the lookup-only calls: float16 volume, float32 warp, two lane widths
    vol, wrp, rec, mask = vols[torch.float16], warps[torch.float32], shs[torch.float16, 2], occ[torch.float16]
    for S in (65, 257):
        z_vals = (0.5 + 3.0 * torch.sort(torch.rand(N_RAYS, S, generator=g), -1).values).to(dev)
        knobs = dict(cutoff=dict(rigidity_cutoff=0.4), scaling=dict(test_time_scaling=1.7), removal=dict(removal_threshold=0.6),
                     white=dict(white_bkgd=True), lindisp=dict(lindisp=True), z_vals=dict(z_vals=z_vals))
        for name, kw in knobs.items():
            emit(f"warp S={S} knob={name}", F.warped_volume_render(vol, wrp, rays, N_samples=S, **ALL, **kw))
            emit(f"culled0 S={S} knob={name}", F.culled_volume_render(vol, rays, occupancy=mask, warp=wrp, N_samples=S, **ALL, **kw))
            emit(f"sh2 S={S} knob={name}", F.sh_volume_render(rec, rays, N_samples=S, warp=wrp, **ALL, **kw))
            emit(f"culled2 S={S} knob={name}", F.culled_volume_render(rec, rays, occupancy=mask, warp=wrp, N_samples=S, **ALL, **kw))
        emit(f"sh2 S={S} knob=ray-directions", F.sh_volume_render(rec, rays, N_samples=S, warp=wrp, ray_directions=True, **ALL))
        emit(f"culled2 S={S} knob=ray-directions", F.culled_volume_render(rec, rays, occupancy=mask, warp=wrp, N_samples=S, ray_directions=True, **ALL))
        emit(f"volume S={S} knob=removal", F.volume_render(vol, rays, N_samples=S, removal_threshold=0.6, retraw=True,
                                                            points4=F.warped_volume_render(vol, wrp, rays, N_samples=S, composite=False, return_points=True)["points4"]))
        lookup = dict(composite=False, retraw=True, return_points=True)
        emit(f"volume S={S} lookup", F.volume_render(vol, rays, N_samples=S, composite=False))
        for vt in DTYPES:
            for wt in DTYPES:
                tag = f"S={S} vol={NAME[vt]} warp={NAME[wt]} lookup"
                emit(f"warp {tag}", F.warped_volume_render(vols[vt], warps[wt], rays, N_samples=S, **lookup))
                emit(f"culled0 {tag}", F.culled_volume_render(vols[vt], rays, occupancy=occ[vt], warp=warps[wt], N_samples=S, **lookup))
                for deg in (1, 2):
                    emit(f"sh{deg} {tag}", F.sh_volume_render(shs[vt, deg], rays, N_samples=S, warp=warps[wt], **lookup))
                    emit(f"culled{deg} {tag}", F.culled_volume_render(shs[vt, deg], rays, occupancy=occ[vt], warp=warps[wt], N_samples=S, **lookup))
        emit(f"culled2 S={S} straight lookup", F.culled_volume_render(rec, rays, occupancy=mask, N_samples=S, **lookup))
        emit(f"sh2 S={S} straight lookup differences", F.sh_volume_render(rec, rays, N_samples=S, ray_directions=False, **lookup))
    z_vals = (0.5 + 3.0 * torch.sort(torch.rand(N_RAYS, 100, generator=g), -1).values).to(dev)
    for name, kw in dict(cutoff=dict(rigidity_cutoff=0.4), scaling=dict(test_time_scaling=1.7), removal=dict(removal_threshold=0.6),
                         white=dict(white_bkgd=True), lindisp=dict(lindisp=True), z_vals=dict(z_vals=z_vals)).items():
        emit(f"hier 100+93 knob={name}", F.hierarchical_volume_render(vol, wrp, rays, N_samples=100, N_importance=93, **ALL, **kw))
    # ---- hierarchical sampling: one (coarse, importance) pair per coarse lane width, with a warp of either storage and without one
    for Sc, I in HIERARCHICAL:
        for vt in DTYPES:
            for wt in DTYPES:
                emit(f"hier {Sc}+{I} vol={NAME[vt]} warp={NAME[wt]}",
                     F.hierarchical_volume_render(vols[vt], warps[wt], rays, N_samples=Sc, N_importance=I, importance_u=u[:, :I].to(dev), **ALL))
            emit(f"hier {Sc}+{I} vol={NAME[vt]} no warp", F.hierarchical_volume_render(vols[vt], None, rays, N_samples=Sc, N_importance=I, **ALL))


if __name__ == "__main__":
    main()
