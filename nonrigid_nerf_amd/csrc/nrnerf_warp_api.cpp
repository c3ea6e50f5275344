// nrnerf_warp_api.cpp -- nrnerf_warped_volume_render of the C ABI (include/nrnerf.h, "ABI 10 (additions): baked warps"): model-free -- validate,
// run the launcher of nrnerf_warp.h on the device that owns the outputs.  The checks come in the order the header states them, the ones that
// need no HIP call first; the entry point keeps no state.  What it shares with nrnerf_volume_render is in nrnerf_baked_api.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_baked_api.h"
#include "nrnerf_warp.h"

using namespace nrn;

extern "C" {

int nrnerf_warped_volume_render(const nrnerf_warped_volume_render_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_warped_volume_render_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->ray_stride < 8) return NRNERF_ERR_INVALID;
    if (!grid_ok(a->g, a->min_point, a->max_point, a->volume_dtype)) return NRNERF_ERR_INVALID;
    if (!grid_ok(a->warp_g, a->warp_min_point, a->warp_max_point, a->warp_dtype)) return NRNERF_ERR_INVALID;
    if (grid_too_large(a->g) || grid_too_large(a->warp_g)) return NRNERF_ERR_UNSUPPORTED;
    if ((long long)a->n_rays * a->n_samples >= (1ll << 31)) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || !a->volume || !a->warp) return NRNERF_ERR_INVALID;
    const bool maps = a->rgb && a->disp && a->acc;
    if (!maps && (a->rgb || a->disp || a->acc)) return NRNERF_ERR_INVALID;
    if (!maps && !a->raw && !a->points4) return NRNERF_ERR_INVALID;
    const bool surface = a->surface_pts || a->surface_rigidity || a->median_index;
    if (!maps && (a->weights || a->alpha || surface)) return NRNERF_ERR_INVALID;
    // device memory, all of it on one device
    const void* const owner = maps ? (const void*)a->rgb : a->raw ? (const void*)a->raw : (const void*)a->points4;
    int dev = 0;
    if (device_of(owner, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    if (!all_on_device({a->rays, a->z, a->volume, a->warp, a->rgb, a->disp, a->acc, a->raw, a->weights, a->alpha,
                        a->surface_pts, a->surface_rigidity, a->median_index, a->points4}, dev)) return NRNERF_ERR_INVALID;
    if (a->points4 && ((uintptr_t)a->points4 & 15)) return NRNERF_ERR_INVALID;
    if (a->raw && ((uintptr_t)a->raw & 15)) return NRNERF_ERR_INVALID;
    if (!grid_aligned(a->volume, a->volume_dtype) || !grid_aligned(a->warp, a->warp_dtype)) return NRNERF_ERR_INVALID;
    WarpArgs k{};
    k.c = composite_args_of(*a, maps);
    if (maps) { k.surf_pts = a->surface_pts; k.surf_rig = a->surface_rigidity; k.med_idx = a->median_index; }
    k.vol = grid_of(a->volume, a->volume_dtype, a->g, a->min_point, a->max_point);
    k.warp = grid_of(a->warp, a->warp_dtype, a->warp_g, a->warp_min_point, a->warp_max_point);
    k.has_cutoff = a->has_rigidity_cutoff; k.cutoff = a->rigidity_cutoff;
    k.has_scaling = a->has_test_time_scaling; k.scaling = a->test_time_scaling;
    k.has_removal = a->has_removal_threshold; k.removal = a->removal_threshold;
    k.raw_out = a->raw; k.points4_out = a->points4;
    return launch_on(dev, k, launch_warped_volume_render, hip_stream);
} NRN_CATCH

}  // extern "C"
