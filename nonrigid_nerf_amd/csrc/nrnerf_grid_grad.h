// nrnerf_grid_grad.h -- launch interface of the adjoint of the grid lookup (the kernels: nrnerf_grid_grad.hip; what nrnerf_grid_lookup_backward
// runs).  No kernel body: the entry point's unit includes this alone.
#pragma once
#include "nrnerf_kernels.h"
#include "nrnerf_volume.h"

namespace nrn {

struct GridGradArgs {
    GridArgs grid;           // the grid the values were looked up in; grid.vol is read only when d_points is asked for
    long long n_points;      // M
    const float* points;     // [M, point_stride] xyz first
    int point_stride;        // >= 3
    const float* g_value;    // [M, 4] the cotangent of the looked-up value, 16-byte aligned
    float* d_grid;           // float32 [gz, gy, gx, 4], ADDED INTO with atomics (the caller zeroes it), or nullptr
    float* d_points;         // [M, 3], written, or nullptr
};
// One launch per output that is asked for; hipErrorInvalidValue when neither is (nothing is launched).  `num_cus` sizes the grids of the point
// loops; d_points does not depend on it, d_grid only through the order of its sums
hipError_t launch_grid_lookup_backward(const GridGradArgs& a, int num_cus, hipStream_t stream);

}  // namespace nrn
