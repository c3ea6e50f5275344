// nrnerf_sh_volume.h -- launch interface of the view-dependent baked renderer (the kernels: nrnerf_sh_volume.hip; what nrnerf_sh_volume_render
// runs).  No kernel body: the entry point's unit includes this alone.
#pragma once
#include "nrnerf_kernels.h"
#include "nrnerf_volume.h"
#include "nrnerf_warp.h"

namespace nrn {

struct ShVolumeArgs {
    // everything nrnerf_warped_volume_render's kernels take, read the same way; w.warp.vol == nullptr: no warp (points4_in, or straight rays:
    // then the cutoff and the scaling have nothing to act on and the mask is 0)
    WarpArgs w;
    const void* sh;          // [gz,gy,gx,12 * degree] on w.vol's grid, w.vol's storage: channel 3 (k - 1) + c = coefficient k of colour c
    int degree;              // 1 or 2
    const float* points4_in; // [N,S,4] ready-made (bent xyz, mask) or nullptr
    int ray_dirs;            // 0: a sample's direction from the difference of the ray's bent points, 1: the ray's own direction
};
// hipErrorInvalidValue for S outside 1 .. 1024, a degree other than 1 or 2, differences with S == 1 (nothing is launched).  `num_cus` sizes the
// grid of the ray loop; the result does not depend on it
// (one translation unit per degree defines its specialisation: nrnerf_sh_volume.hip with NRN_SH_DEGREE = 1 / 2)
template <int DEG>
hipError_t launch_sh_volume_render_degree(const ShVolumeArgs& a, int num_cus, hipStream_t stream);
template <> hipError_t launch_sh_volume_render_degree<1>(const ShVolumeArgs& a, int num_cus, hipStream_t stream);
template <> hipError_t launch_sh_volume_render_degree<2>(const ShVolumeArgs& a, int num_cus, hipStream_t stream);
inline hipError_t launch_sh_volume_render(const ShVolumeArgs& a, int num_cus, hipStream_t stream) {
    if (a.degree == 1) return launch_sh_volume_render_degree<1>(a, num_cus, stream);
    if (a.degree == 2) return launch_sh_volume_render_degree<2>(a, num_cus, stream);
    return hipErrorInvalidValue;
}

}  // namespace nrn
