// nrnerf_culled_volume_api.cpp -- nrnerf_culled_volume_render of the C ABI (include/nrnerf.h, "ABI 10 (additions): occupancy masks"):
// model-free -- validate, run the launcher of nrnerf_culled_volume.h on the device that owns the outputs.  The checks come in the order the
// header states them, the ones that need no HIP call first; the entry point keeps no state.  What it shares with the other baked renders is
// in nrnerf_baked_api.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_baked_api.h"
#include "nrnerf_culled_volume.h"

using namespace nrn;

extern "C" {

int nrnerf_culled_volume_render(const nrnerf_culled_volume_render_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_culled_volume_render_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->ray_stride < 8) return NRNERF_ERR_INVALID;
    if (a->sh_degree < 0 || a->sh_degree > 2) return NRNERF_ERR_INVALID;
    if (a->direction_mode != NRNERF_SH_DIRECTION_DIFFERENCES && a->direction_mode != NRNERF_SH_DIRECTION_RAY) return NRNERF_ERR_INVALID;
    if (a->sh_degree >= 1 && a->direction_mode == NRNERF_SH_DIRECTION_DIFFERENCES && a->n_samples == 1) return NRNERF_ERR_INVALID;
    if (a->warp && a->points4_in) return NRNERF_ERR_INVALID;
    if (!grid_ok(a->g, a->min_point, a->max_point, a->volume_dtype)) return NRNERF_ERR_INVALID;
    if (a->warp && !grid_ok(a->warp_g, a->warp_min_point, a->warp_max_point, a->warp_dtype)) return NRNERF_ERR_INVALID;
    if (a->occupancy_log2_block < OCC_MIN_LOG2_BLOCK || a->occupancy_log2_block > OCC_MAX_LOG2_BLOCK) return NRNERF_ERR_INVALID;
    if (grid_too_large(a->g) || (a->warp && grid_too_large(a->warp_g))) return NRNERF_ERR_UNSUPPORTED;
    if ((long long)a->n_rays * a->n_samples >= (1ll << 31)) return NRNERF_ERR_UNSUPPORTED;
    const int gg[3] = {a->g[0], a->g[1], a->g[2]};
    if (a->occupancy_words != occupancy_words(gg, a->occupancy_log2_block)) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || !a->volume) return NRNERF_ERR_INVALID;
    if (!a->occupancy) return NRNERF_ERR_INVALID;
    if ((a->sh_degree == 0) != (a->sh == nullptr)) return NRNERF_ERR_INVALID;
    const bool maps = a->rgb && a->disp && a->acc;
    if (!maps && (a->rgb || a->disp || a->acc)) return NRNERF_ERR_INVALID;
    if (!maps && !a->raw && !a->points4) return NRNERF_ERR_INVALID;
    const bool surface = a->surface_pts || a->surface_rigidity || a->median_index;
    if (!maps && (a->weights || a->alpha || surface)) return NRNERF_ERR_INVALID;
    // device memory, all of it on one device
    const void* const owner = maps ? (const void*)a->rgb : a->raw ? (const void*)a->raw : (const void*)a->points4;
    int dev = 0;
    if (device_of(owner, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    if (!all_on_device({a->rays, a->z, a->volume, a->sh, a->warp, a->points4_in, a->rgb, a->disp, a->acc, a->raw, a->weights, a->alpha,
                        a->surface_pts, a->surface_rigidity, a->median_index, a->points4, a->occupancy}, dev)) return NRNERF_ERR_INVALID;
    if (((uintptr_t)a->points4 | (uintptr_t)a->raw | (uintptr_t)a->points4_in) & 15) return NRNERF_ERR_INVALID;
    if (!grid_aligned(a->volume, a->volume_dtype) || (a->sh && !grid_aligned(a->sh, a->volume_dtype))) return NRNERF_ERR_INVALID;
    if (a->warp && !grid_aligned(a->warp, a->warp_dtype)) return NRNERF_ERR_INVALID;
    if ((uintptr_t)a->occupancy & 3) return NRNERF_ERR_INVALID;
    CulledVolumeArgs k{};
    ShVolumeArgs& s = k.s;
    s.w.c = composite_args_of(*a, maps);
    if (maps) { s.w.surf_pts = a->surface_pts; s.w.surf_rig = a->surface_rigidity; s.w.med_idx = a->median_index; }
    s.w.vol = grid_of(a->volume, a->volume_dtype, a->g, a->min_point, a->max_point);
    if (a->warp) {
        s.w.warp = grid_of(a->warp, a->warp_dtype, a->warp_g, a->warp_min_point, a->warp_max_point);
        s.w.has_cutoff = a->has_rigidity_cutoff; s.w.cutoff = a->rigidity_cutoff;
        s.w.has_scaling = a->has_test_time_scaling; s.w.scaling = a->test_time_scaling;
    }
    s.w.has_removal = a->has_removal_threshold; s.w.removal = a->removal_threshold;
    s.w.raw_out = a->raw; s.w.points4_out = a->points4;
    s.sh = a->sh; s.degree = a->sh_degree; s.points4_in = a->points4_in;
    s.ray_dirs = a->direction_mode == NRNERF_SH_DIRECTION_RAY;
    k.occ = (const unsigned*)a->occupancy; k.k = a->occupancy_log2_block;
    k.nb[0] = occupancy_blocks(a->g[0], k.k); k.nb[1] = occupancy_blocks(a->g[1], k.k);
    return launch_on(dev, k, launch_culled_volume_render, hip_stream);
} NRN_CATCH

}  // extern "C"
