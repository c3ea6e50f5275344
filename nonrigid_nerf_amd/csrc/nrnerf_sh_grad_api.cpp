// nrnerf_sh_grad_api.cpp -- nrnerf_sh_lookup_backward of the C ABI (include/nrnerf.h, "ABI 10 (additions): the adjoint of the colour sum"):
// model-free -- validate, run the launcher of nrnerf_sh_grad.h on the device that owns the outputs.  The checks come in the order the header
// states them, the ones that need no HIP call first; the entry point keeps no state.  The grid checks are those of the baked renders
// (nrnerf_baked_api.h).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_baked_api.h"
#include "nrnerf_sh_grad.h"

using namespace nrn;

extern "C" {

int nrnerf_sh_lookup_backward(const nrnerf_sh_lookup_backward_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_sh_lookup_backward_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES) return NRNERF_ERR_INVALID;
    if (a->sh_degree != 1 && a->sh_degree != 2) return NRNERF_ERR_INVALID;
    if (a->direction_mode != NRNERF_SH_DIRECTION_DIFFERENCES && a->direction_mode != NRNERF_SH_DIRECTION_RAY) return NRNERF_ERR_INVALID;
    const bool ray_dirs = a->direction_mode == NRNERF_SH_DIRECTION_RAY;
    if (!ray_dirs && a->n_samples == 1) return NRNERF_ERR_INVALID;
    if (ray_dirs && a->ray_stride < 6) return NRNERF_ERR_INVALID;
    if (!grid_ok(a->g, a->min_point, a->max_point, a->sh_dtype)) return NRNERF_ERR_INVALID;
    if (grid_too_large(a->g)) return NRNERF_ERR_UNSUPPORTED;
    if ((long long)a->n_rays * a->n_samples >= (1ll << 31)) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->points4 || !a->g_raw || (ray_dirs && !a->rays)) return NRNERF_ERR_INVALID;
    if (!a->d_sh && !a->d_points && !a->d_dirs) return NRNERF_ERR_INVALID;
    const bool reads_sh = a->d_points || a->d_dirs;
    if (reads_sh && !a->sh) return NRNERF_ERR_INVALID;
    if (!ray_dirs && a->d_points && !a->d_dirs) return NRNERF_ERR_INVALID;
    // device memory, all of it on one device
    const void* const owner = a->d_sh ? (const void*)a->d_sh : a->d_points ? (const void*)a->d_points : (const void*)a->d_dirs;
    int dev = 0;
    if (device_of(owner, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    const void* const sh_read = reads_sh ? a->sh : nullptr;
    if (!all_on_device({ray_dirs ? a->rays : nullptr, a->points4, a->g_raw, sh_read, a->d_sh, a->d_points, a->d_dirs}, dev)) return NRNERF_ERR_INVALID;
    if (((uintptr_t)a->points4 | (uintptr_t)a->g_raw) & 15) return NRNERF_ERR_INVALID;
    if (sh_read && !grid_aligned(sh_read, a->sh_dtype)) return NRNERF_ERR_INVALID;
    ShGradArgs k{};
    k.grid = grid_of(sh_read, a->sh_dtype, a->g, a->min_point, a->max_point);
    k.degree = a->sh_degree;
    k.n_rays = a->n_rays; k.S = a->n_samples;
    k.rays = ray_dirs ? a->rays : nullptr; k.ray_stride = a->ray_stride;
    k.points4 = a->points4;
    k.ray_dirs = ray_dirs;
    k.g_raw = a->g_raw;
    k.d_sh = a->d_sh; k.d_points = a->d_points; k.d_dirs = a->d_dirs;
    return launch_on(dev, k, launch_sh_lookup_backward, hip_stream);
} NRN_CATCH

}  // extern "C"
