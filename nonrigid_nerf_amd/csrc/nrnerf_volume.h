// nrnerf_volume.h -- launch interface of the baked-volume renderer (the kernels: nrnerf_volume.hip; what nrnerf_volume_render runs).
// No kernel body: the entry point's unit includes this alone.
#pragma once
#include "nrnerf_kernels.h"

namespace nrn {

// a vertex-centred grid of four channels: a baked volume's logits, a baked warp's offsets (the lookup: nrnerf_volume_lookup.h)
struct GridArgs {
    const void* vol;         // [gz,gy,gx,4]
    int half;                // 0: float32 (16 bytes per vertex), 1: IEEE half (8 bytes per vertex)
    int g[3];                // gx, gy, gz, each >= 2
    float lo[3];             // min_point
    float scale[3];          // (float)(g - 1) / (max_point - min_point), each operation rounded to fp32
    float top[3];            // (float)(g - 1)
};

struct VolumeArgs {
    // rays / ray_stride / z / lindisp / white_bkgd / n_rays / S / rgb / disp / acc / vis / alpha and the surface reduction (bent4 = the
    // sample points, surf_pts, surf_rig, med_idx) as composite_kernel reads them; raw4, noise, u, n_importance and the split-bender fields
    // stay zero.  rgb == nullptr: nothing is composited, the lookup kernel writes raw_out alone
    CompositeArgs c;
    const float* points4;    // [N,S,4] sample points (xyz, rigidity) or nullptr: o + d z
    GridArgs grid;           // the volume: (r, g, b, sigma) logits
    int has_removal; float removal;      // sigma logit * 0 where points4.w >= removal (needs points4)
    float* raw_out;          // [N,S,4] the sampled logits or nullptr
};
// hipErrorInvalidValue for S outside 1 .. 1024 (nothing is launched).  `num_cus` sizes the grid of the ray loop; the result does not depend on it
hipError_t launch_volume_render(const VolumeArgs& a, int num_cus, hipStream_t stream);

}  // namespace nrn
