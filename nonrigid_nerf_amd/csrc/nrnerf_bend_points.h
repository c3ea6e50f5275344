// nrnerf_bend_points.h -- launch interface of the POINT-SOURCE variants of the stand-alone benders (bend_kernel<.., POINTS> of nrnerf_bend.h,
// bend_kernel_x16<.., POINTS> of nrnerf_bend_x16.h): the bender on caller-given points instead of samples placed on rays.  What nrnerf_query runs
// (the reference's network_query_fn, train.py:57-105, 633-649).  A record of its own AROUND BendArgs: BendArgs and the ray-source kernels
// stay as they are.
#pragma once
#include "nrnerf_kernels.h"

namespace nrn {

struct BendPointSrc {
    const float* points; int stride;     // [n_rays, n_per_ray, stride >= 3]; 16-byte loads when stride == 4 and the base is 16-byte aligned
    float* unmasked;                     // [n_rays, n_per_ray, 3] unmasked offsets (rnh:541), or nullptr
    float* masked;                       // [n_rays, n_per_ray, 3] masked (and scaled) offsets (rnh:567-569), or nullptr
};
// b.rays / ray_stride / z / lindisp / rank are not read and b.out_stride must equal b.n_per_ray (bent4 rows in the order of the points); the
// latent code (per row, or one for the launch), the knobs, the work counter and bent4 as for the ray-source kernels
struct BendPointArgs { BendArgs b; BendPointSrc src; };
__host__ __device__ inline const BendArgs& bend_args_of(const BendArgs& a) { return a; }
__host__ __device__ inline const BendArgs& bend_args_of(const BendPointArgs& a) { return a.b; }
__host__ __device__ inline const BendPointSrc& bend_points_of(const BendPointArgs& a) { return a.src; }

// the 32x32x16 kernel: the three precision policies x bender architectures 0 (5 x 64) and 1 (7 x 64), as launch_bend
hipError_t launch_bend_points(int precision, int arch_id, const BendPointArgs& a, int num_cus, hipStream_t stream);
// the 16x16x32 kernel: the image of pack_pass_x16_bend, as launch_bend_x16
hipError_t launch_bend_points_x16(int arch, const BendPointArgs& a, int num_cus, hipStream_t stream);

}  // namespace nrn
