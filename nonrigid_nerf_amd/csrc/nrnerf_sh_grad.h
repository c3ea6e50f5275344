// nrnerf_sh_grad.h -- launch interface of the adjoint of the spherical-harmonic colour sum (the kernels: nrnerf_sh_grad.hip; what
// nrnerf_sh_lookup_backward runs).  No kernel body: the entry point's unit includes this alone.
#pragma once
#include "nrnerf_kernels.h"
#include "nrnerf_volume.h"

namespace nrn {

struct ShGradArgs {
    GridArgs grid;           // the grid of the coefficients; grid.vol = sh [gz,gy,gx,12 * degree], read only for d_points / d_dirs
    int degree;              // 1 or 2
    int n_rays, S;           // N, samples per ray
    const float* rays;       // [N, ray_stride], columns 3 .. 5 read when ray_dirs
    int ray_stride;
    const float* points4;    // [N,S,4] the bent points (xyz first), 16-byte aligned
    int ray_dirs;            // 0: a sample's direction from the difference of the ray's bent points, 1: the ray's own direction
    const float* g_raw;      // [N,S,4] cotangents of the samples' logits, channels 0 .. 2 read, 16-byte aligned
    float* d_sh;             // float32 [gz,gy,gx,12 * degree], ADDED INTO with atomics (the caller zeroes it), or nullptr
    float* d_points;         // [N,S,3], written, or nullptr
    float* d_dirs;           // [N,S,3], written, or nullptr; with differences d_points needs it (the workspace of the chain)
};
// One launch per kernel that is needed: the scatter (d_sh), the point / direction gradient (d_points or d_dirs), the direction chain (d_points
// with differences).  hipErrorInvalidValue for a degree other than 1 or 2, nothing to write, differences with S == 1 or with d_points but no
// d_dirs, 2^31 or more samples (nothing is launched).  `num_cus` sizes the grids of the sample loops; d_points and d_dirs do not depend on it, d_sh only through the
// order of its sums
hipError_t launch_sh_lookup_backward(const ShGradArgs& a, int num_cus, hipStream_t stream);

}  // namespace nrn
