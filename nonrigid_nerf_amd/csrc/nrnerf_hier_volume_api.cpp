// nrnerf_hier_volume_api.cpp -- nrnerf_hierarchical_volume_render of the C ABI (include/nrnerf.h, "ABI 10 (additions): hierarchical sampling of
// a baked scene"): model-free -- validate, run the launcher of nrnerf_hier_volume.h on the device that owns the outputs.  The checks come in the
// order the header states them, the ones that need no HIP call first; the entry point keeps no state.  What it shares with the other baked
// renders is in nrnerf_baked_api.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_baked_api.h"
#include "nrnerf_hier_volume.h"

using namespace nrn;

extern "C" {

int nrnerf_hierarchical_volume_render(const nrnerf_hierarchical_volume_render_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_hierarchical_volume_render_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 3 || a->n_importance < 1 || a->ray_stride < 8) return NRNERF_ERR_INVALID;
    if (!grid_ok(a->g, a->min_point, a->max_point, a->volume_dtype)) return NRNERF_ERR_INVALID;
    if (a->warp && !grid_ok(a->warp_g, a->warp_min_point, a->warp_max_point, a->warp_dtype)) return NRNERF_ERR_INVALID;
    if (a->n_samples > HIER_MAX_COARSE || (long long)a->n_samples + a->n_importance > HIER_MAX_MERGED) return NRNERF_ERR_UNSUPPORTED;
    if (grid_too_large(a->g) || (a->warp && grid_too_large(a->warp_g))) return NRNERF_ERR_UNSUPPORTED;
    const int n_merged = a->n_samples + a->n_importance;
    if ((long long)a->n_rays * n_merged >= (1ll << 31)) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || !a->volume) return NRNERF_ERR_INVALID;
    if (!a->rgb || !a->disp || !a->acc) return NRNERF_ERR_INVALID;
    const bool coarse = a->rgb0 && a->disp0 && a->acc0;
    if (!coarse && (a->rgb0 || a->disp0 || a->acc0)) return NRNERF_ERR_INVALID;
    // device memory, all of it on one device
    int dev = 0;
    if (device_of(a->rgb, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    if (!all_on_device({a->rays, a->z, a->u, a->volume, a->warp, a->rgb, a->disp, a->acc, a->rgb0, a->disp0, a->acc0, a->z_std, a->z_vals, a->raw,
                        a->weights, a->alpha, a->surface_pts, a->surface_rigidity, a->median_index, a->points4}, dev)) return NRNERF_ERR_INVALID;
    if (a->points4 && ((uintptr_t)a->points4 & 15)) return NRNERF_ERR_INVALID;
    if (a->raw && ((uintptr_t)a->raw & 15)) return NRNERF_ERR_INVALID;
    if (!grid_aligned(a->volume, a->volume_dtype) || (a->warp && !grid_aligned(a->warp, a->warp_dtype))) return NRNERF_ERR_INVALID;
    HierArgs k{};
    // the fine pass
    CompositeArgs& f = k.w.c;
    f.rays = a->rays; f.ray_stride = a->ray_stride; f.white_bkgd = a->white_bkgd; f.n_rays = a->n_rays; f.S = n_merged;
    f.z = a->rays;          // never read: says "explicit depths" (they are in LDS)
    f.rgb = a->rgb; f.disp = a->disp; f.acc = a->acc; f.vis = a->weights; f.alpha = a->alpha;
    k.w.surf_pts = a->surface_pts; k.w.surf_rig = a->surface_rigidity; k.w.med_idx = a->median_index;
    k.w.vol = grid_of(a->volume, a->volume_dtype, a->g, a->min_point, a->max_point);
    if (a->warp) k.w.warp = grid_of(a->warp, a->warp_dtype, a->warp_g, a->warp_min_point, a->warp_max_point);
    k.w.has_cutoff = a->has_rigidity_cutoff; k.w.cutoff = a->rigidity_cutoff;
    k.w.has_scaling = a->has_test_time_scaling; k.w.scaling = a->test_time_scaling;
    k.w.has_removal = a->has_removal_threshold; k.w.removal = a->removal_threshold;
    k.w.raw_out = a->raw; k.w.points4_out = a->points4;
    // the coarse pass and the sampling
    CompositeArgs& c = k.cc;
    c.rays = a->rays; c.ray_stride = a->ray_stride; c.z = a->z; c.lindisp = a->lindisp; c.white_bkgd = a->white_bkgd;
    c.n_rays = a->n_rays; c.S = a->n_samples; c.n_importance = a->n_importance; c.u = a->u;
    if (coarse) { c.rgb = a->rgb0; c.disp = a->disp0; c.acc = a->acc0; }
    c.z_std = a->z_std; c.z_out = a->z_vals;
    k.coarse_maps = coarse;
    return launch_on(dev, k, launch_hier_volume_render, hip_stream);
} NRN_CATCH

}  // extern "C"
