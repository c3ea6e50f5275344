// nrnerf_sh_volume_api.cpp -- nrnerf_sh_volume_render of the C ABI (include/nrnerf.h, "ABI 10 (additions): view-dependent bakes"): model-free --
// validate, run the launcher of nrnerf_sh_volume.h on the device that owns the outputs.  The checks come in the order the header states them,
// the ones that need no HIP call first; the entry point keeps no state.  What it shares with the other baked renders is in nrnerf_baked_api.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_baked_api.h"
#include "nrnerf_sh_volume.h"

using namespace nrn;

extern "C" {

int nrnerf_sh_volume_render(const nrnerf_sh_volume_render_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_sh_volume_render_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->ray_stride < 8) return NRNERF_ERR_INVALID;
    if (a->sh_degree != 1 && a->sh_degree != 2) return NRNERF_ERR_INVALID;
    if (a->direction_mode != NRNERF_SH_DIRECTION_DIFFERENCES && a->direction_mode != NRNERF_SH_DIRECTION_RAY) return NRNERF_ERR_INVALID;
    if (a->direction_mode == NRNERF_SH_DIRECTION_DIFFERENCES && a->n_samples == 1) return NRNERF_ERR_INVALID;
    if (a->warp && a->points4_in) return NRNERF_ERR_INVALID;
    if (!grid_ok(a->g, a->min_point, a->max_point, a->volume_dtype)) return NRNERF_ERR_INVALID;
    if (a->warp && !grid_ok(a->warp_g, a->warp_min_point, a->warp_max_point, a->warp_dtype)) return NRNERF_ERR_INVALID;
    if (grid_too_large(a->g) || (a->warp && grid_too_large(a->warp_g))) return NRNERF_ERR_UNSUPPORTED;
    if ((long long)a->n_rays * a->n_samples >= (1ll << 31)) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || !a->volume || !a->sh) return NRNERF_ERR_INVALID;
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
                        a->surface_pts, a->surface_rigidity, a->median_index, a->points4}, dev)) return NRNERF_ERR_INVALID;
    if (((uintptr_t)a->points4 | (uintptr_t)a->raw | (uintptr_t)a->points4_in) & 15) return NRNERF_ERR_INVALID;
    if (!grid_aligned(a->volume, a->volume_dtype) || !grid_aligned(a->sh, a->volume_dtype)) return NRNERF_ERR_INVALID;
    if (a->warp && !grid_aligned(a->warp, a->warp_dtype)) return NRNERF_ERR_INVALID;
    ShVolumeArgs k{};
    k.w.c = composite_args_of(*a, maps);
    if (maps) { k.w.surf_pts = a->surface_pts; k.w.surf_rig = a->surface_rigidity; k.w.med_idx = a->median_index; }
    k.w.vol = grid_of(a->volume, a->volume_dtype, a->g, a->min_point, a->max_point);
    if (a->warp) {
        k.w.warp = grid_of(a->warp, a->warp_dtype, a->warp_g, a->warp_min_point, a->warp_max_point);
        k.w.has_cutoff = a->has_rigidity_cutoff; k.w.cutoff = a->rigidity_cutoff;
        k.w.has_scaling = a->has_test_time_scaling; k.w.scaling = a->test_time_scaling;
    }
    k.w.has_removal = a->has_removal_threshold; k.w.removal = a->removal_threshold;
    k.w.raw_out = a->raw; k.w.points4_out = a->points4;
    k.sh = a->sh; k.degree = a->sh_degree; k.points4_in = a->points4_in;
    k.ray_dirs = a->direction_mode == NRNERF_SH_DIRECTION_RAY;
    return launch_on(dev, k, launch_sh_volume_render, hip_stream);
} NRN_CATCH

}  // extern "C"
