// nrnerf_warp_api.cpp -- nrnerf_warped_volume_render of the C ABI (include/nrnerf.h, "ABI 10 (additions): baked warps"): model-free -- validate,
// run the launcher of nrnerf_warp.h on the device that owns the outputs.  The checks come in the order the header states them, the ones that
// need no HIP call first; the entry point keeps no state.  Its own unit, so that the objects of the existing entry points are built from
// unchanged sources.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_model.h"
#include "nrnerf_warp.h"

using namespace nrn;

namespace {

bool grid_ok(const int32_t (&g)[3], const float (&lo)[3], const float (&hi)[3], int32_t dtype) {
    for (int c = 0; c < 3; ++c)
        if (g[c] < 2 || !(hi[c] > lo[c])) return false;                                                      // (NaN included)
    return dtype == NRNERF_VOLUME_F32 || dtype == NRNERF_VOLUME_F16;
}

bool grid_too_large(const int32_t (&g)[3]) {
    return (double)g[0] * (double)g[1] * (double)g[2] > (double)(1ll << 30);      // (in double: three factors below 2^31 overflow 64 bits)
}

GridArgs grid_of(const void* base, int32_t dtype, const int32_t (&g)[3], const float (&lo)[3], const float (&hi)[3]) {
    GridArgs k{};
    k.vol = base; k.half = dtype == NRNERF_VOLUME_F16;
    for (int c = 0; c < 3; ++c) {
        k.g[c] = g[c]; k.lo[c] = lo[c];
        k.top[c] = (float)(g[c] - 1);
        volatile float extent = hi[c] - lo[c];          // (each operation rounded to fp32, whatever the host compiler would like to keep wider)
        volatile float scale = k.top[c] / extent;
        k.scale[c] = scale;
    }
    return k;
}

}  // namespace

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
    const void* ptrs[] = {a->rays, a->z, a->volume, a->warp, a->rgb, a->disp, a->acc, a->raw, a->weights, a->alpha,
                          a->surface_pts, a->surface_rigidity, a->median_index, a->points4};
    for (const void* p : ptrs) {
        int d = 0;
        if (p && (device_of(p, d) != NRNERF_OK || d != dev)) return NRNERF_ERR_INVALID;
    }
    if (a->points4 && ((uintptr_t)a->points4 & 15)) return NRNERF_ERR_INVALID;
    if (a->raw && ((uintptr_t)a->raw & 15)) return NRNERF_ERR_INVALID;
    if ((uintptr_t)a->volume & (a->volume_dtype == NRNERF_VOLUME_F16 ? 7 : 15)) return NRNERF_ERR_INVALID;
    if ((uintptr_t)a->warp & (a->warp_dtype == NRNERF_VOLUME_F16 ? 7 : 15)) return NRNERF_ERR_INVALID;
    WarpArgs k{};
    k.c.rays = a->rays; k.c.ray_stride = a->ray_stride; k.c.z = a->z; k.c.lindisp = a->lindisp; k.c.white_bkgd = a->white_bkgd;
    k.c.n_rays = a->n_rays; k.c.S = a->n_samples;
    if (maps) {
        k.c.rgb = a->rgb; k.c.disp = a->disp; k.c.acc = a->acc; k.c.vis = a->weights; k.c.alpha = a->alpha;
        k.surf_pts = a->surface_pts; k.surf_rig = a->surface_rigidity; k.med_idx = a->median_index;
    }
    k.vol = grid_of(a->volume, a->volume_dtype, a->g, a->min_point, a->max_point);
    k.warp = grid_of(a->warp, a->warp_dtype, a->warp_g, a->warp_min_point, a->warp_max_point);
    k.has_cutoff = a->has_rigidity_cutoff; k.cutoff = a->rigidity_cutoff;
    k.has_scaling = a->has_test_time_scaling; k.scaling = a->test_time_scaling;
    k.has_removal = a->has_removal_threshold; k.removal = a->removal_threshold;
    k.raw_out = a->raw; k.points4_out = a->points4;
    return on_device(dev, [&]() -> int {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return NRNERF_ERR_HIP;
        return status_of(launch_warped_volume_render(k, cus, (hipStream_t)hip_stream));
    });
} NRN_CATCH

}  // extern "C"
