// nrnerf_baked_launch.h -- the one launch idiom of the baked render kernels (nrnerf_volume.hip, nrnerf_warp.hip, nrnerf_sh_volume.hip,
// nrnerf_culled_volume.hip, nrnerf_hier_volume.hip): the workgroup shape, the two grid sizes, the storage switch and the launch itself.  The
// argument checks of each launch_* entry stay in their units.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace nrn {

constexpr int BAKED_WAVES = 4;          // waves (= rays in flight) per workgroup of a ray-loop kernel
constexpr int BAKED_MAXS = 1024;        // NRNERF_MAX_SAMPLES: EPL <= 16

// the ray loop: one wave per ray at a time, BAKED_WAVES * 64 threads per workgroup; the result does not depend on the grid
inline dim3 ray_loop_grid(const int n_rays, const int num_cus) {
    const long long want = ((long long)n_rays + BAKED_WAVES - 1) / BAKED_WAVES, cap = (long long)(num_cus > 0 ? num_cus : 256) * 16;
    return dim3((unsigned)(want < cap ? want : cap));
}

// one thread per sample, 256 per workgroup
inline dim3 sample_grid(const int n_rays, const int S, const int num_cus) {
    const long long want = ((long long)n_rays * S + 255) / 256, cap = (long long)(num_cus > 0 ? num_cus : 256) * 32;
    return dim3((unsigned)(want < cap ? want : cap));
}

// f(volume is half, warp is half) with the two storage types as std::bool_constant (with_epl's style, nrnerf_kernels.h)
template <class F>
auto with_storage(const bool vol_half, const bool warp_half, F&& f) {
    switch ((vol_half ? 2 : 0) | (warp_half ? 1 : 0)) {
        case 0: return f(std::false_type{}, std::false_type{});
        case 1: return f(std::false_type{}, std::true_type{});
        case 2: return f(std::true_type{}, std::false_type{});
        default: return f(std::true_type{}, std::true_type{});
    }
}

template <class KERNEL, class ARGS>
hipError_t launch(KERNEL kernel, const ARGS& a, const dim3 grid, const dim3 block, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace nrn
