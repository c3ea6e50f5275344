// nrnerf_warp.h -- launch interface of the baked-warp renderer (the kernels: nrnerf_warp.hip; what nrnerf_warped_volume_render runs).
// No kernel body: the entry point's unit includes this alone.
#pragma once
#include "nrnerf_kernels.h"
#include "nrnerf_volume.h"

namespace nrn {

struct WarpArgs {
    // rays / ray_stride / z / lindisp / white_bkgd / n_rays / S / rgb / disp / acc / vis / alpha as composite_kernel reads them; everything
    // else stays zero -- bent4 too: no bent point is in memory, the kernel reduces the surface outputs itself.  rgb == nullptr: nothing is
    // composited, the lookup kernel writes raw_out and / or points4_out
    CompositeArgs c;
    GridArgs vol;            // the canonical volume: (r, g, b, sigma) logits
    GridArgs warp;           // the offset grid: (unmasked offset x, y, z, rigidity mask)
    int has_cutoff; float cutoff;        // mask = 0 where mask <= cutoff (rnh:563-564)
    int has_scaling; float scaling;      // offset * scaling (rnh:567-569)
    int has_removal; float removal;      // sigma logit * 0 where the mask (after the cutoff) >= removal (rnh:308-311)
    float* raw_out;          // [N,S,4] the sampled logits or nullptr
    float* points4_out;      // [N,S,4] (bent xyz, mask after the cutoff) or nullptr
    float* surf_pts;         // [N,3] / [N] / [N]: the surface reduction over (bent, mask), each or nullptr
    float* surf_rig;
    int* med_idx;
};
// hipErrorInvalidValue for S outside 1 .. 1024 (nothing is launched).  `num_cus` sizes the grid of the ray loop; the result does not depend on it
hipError_t launch_warped_volume_render(const WarpArgs& a, int num_cus, hipStream_t stream);

}  // namespace nrn
