// nrnerf_grid_grad_api.cpp -- nrnerf_grid_lookup_backward of the C ABI (include/nrnerf.h, "ABI 10 (additions): the adjoint of the lookup"):
// model-free -- validate, run the launcher of nrnerf_grid_grad.h on the device that owns the outputs.  The checks come in the order the header
// states them, the ones that need no HIP call first; the entry point keeps no state.  The grid checks are those of the baked renders
// (nrnerf_baked_api.h).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_baked_api.h"
#include "nrnerf_grid_grad.h"

using namespace nrn;

extern "C" {

int nrnerf_grid_lookup_backward(const nrnerf_grid_lookup_backward_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_grid_lookup_backward_args)) return NRNERF_ERR_INVALID;
    if (a->n_points < 0 || a->point_stride < 3) return NRNERF_ERR_INVALID;
    if (!grid_ok(a->g, a->min_point, a->max_point, a->grid_dtype)) return NRNERF_ERR_INVALID;
    if (grid_too_large(a->g)) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_points == 0) return NRNERF_OK;
    if (!a->points || !a->g_value) return NRNERF_ERR_INVALID;
    if (!a->d_grid && !a->d_points) return NRNERF_ERR_INVALID;
    if (a->d_points && !a->grid) return NRNERF_ERR_INVALID;
    // device memory, all of it on one device
    const void* const owner = a->d_grid ? (const void*)a->d_grid : (const void*)a->d_points;
    int dev = 0;
    if (device_of(owner, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    const void* const grid_read = a->d_points ? a->grid : nullptr;
    if (!all_on_device({a->points, a->g_value, grid_read, a->d_grid, a->d_points}, dev)) return NRNERF_ERR_INVALID;
    if ((uintptr_t)a->g_value & 15) return NRNERF_ERR_INVALID;
    if (grid_read && !grid_aligned(grid_read, a->grid_dtype)) return NRNERF_ERR_INVALID;
    GridGradArgs k{};
    k.grid = grid_of(grid_read, a->grid_dtype, a->g, a->min_point, a->max_point);
    k.n_points = a->n_points;
    k.points = a->points; k.point_stride = a->point_stride;
    k.g_value = a->g_value;
    k.d_grid = a->d_grid; k.d_points = a->d_points;
    return launch_on(dev, k, launch_grid_lookup_backward, hip_stream);
} NRN_CATCH

}  // extern "C"
