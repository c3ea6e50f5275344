// nrnerf_culled_volume.h -- launch interface of the baked renderer that skips empty space by an occupancy mask (the kernels:
// nrnerf_culled_volume.hip; what nrnerf_culled_volume_render runs).  No kernel body: the entry point's unit includes this alone.
#pragma once
#include "nrnerf_kernels.h"
#include "nrnerf_occupancy.h"
#include "nrnerf_sh_volume.h"

namespace nrn {

struct CulledVolumeArgs {
    // everything nrnerf_sh_volume_render's kernels take, read the same way; s.degree == 0: `raw` alone (s.sh is not read, no direction is made)
    ShVolumeArgs s;
    const unsigned* occ;     // the mask of s.w.vol's grid: bit (bz * nb[1] + by) * nb[0] + bx, word index >> 5, bit index & 31
    int k;                   // log2 of the block's cells per axis
    int nb[2];               // blocks along x, y
};
// hipErrorInvalidValue for S outside 1 .. 1024, a degree outside 0 .. 2, differences with S == 1 at degree 1 / 2, a warp together with
// points4_in, k outside 1 .. 4, and a compositing record with noise: noise added to sigma voids the mask's criterion (nothing is launched).
// `num_cus` sizes the grid of the ray loop; the result does not depend on it
// (one translation unit per degree defines its specialisation: nrnerf_culled_volume.hip with NRN_CULL_DEGREE = 0 / 1 / 2.  Call
// launch_culled_volume_render: the noise and k checks are made there, once, and the specialisations rely on them)
template <int DEG>
hipError_t launch_culled_volume_render_degree(const CulledVolumeArgs& a, int num_cus, hipStream_t stream);
template <> hipError_t launch_culled_volume_render_degree<0>(const CulledVolumeArgs& a, int num_cus, hipStream_t stream);
template <> hipError_t launch_culled_volume_render_degree<1>(const CulledVolumeArgs& a, int num_cus, hipStream_t stream);
template <> hipError_t launch_culled_volume_render_degree<2>(const CulledVolumeArgs& a, int num_cus, hipStream_t stream);
inline hipError_t launch_culled_volume_render(const CulledVolumeArgs& a, int num_cus, hipStream_t stream) {
    if (a.s.w.c.noise || a.k < OCC_MIN_LOG2_BLOCK || a.k > OCC_MAX_LOG2_BLOCK) return hipErrorInvalidValue;
    if (a.s.degree == 0) return launch_culled_volume_render_degree<0>(a, num_cus, stream);
    if (a.s.degree == 1) return launch_culled_volume_render_degree<1>(a, num_cus, stream);
    if (a.s.degree == 2) return launch_culled_volume_render_degree<2>(a, num_cus, stream);
    return hipErrorInvalidValue;
}

}  // namespace nrn
