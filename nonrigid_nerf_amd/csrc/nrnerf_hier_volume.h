// nrnerf_hier_volume.h -- launch interface of the hierarchical baked render (the kernel: nrnerf_hier_volume.hip; what
// nrnerf_hierarchical_volume_render runs): coarse pass, sample_pdf + merge, fine pass of a baked scene in ONE kernel.  No kernel body: the entry
// point's unit includes this alone.
#pragma once
#include "nrnerf_kernels.h"
#include "nrnerf_volume.h"
#include "nrnerf_warp.h"

namespace nrn {

struct HierArgs {
    // the FINE pass, as warped_render_kernel reads a WarpArgs: w.c.S = S_c + I, the fine maps, weights, alpha; raw_out / points4_out / the
    // surface outputs; both grids and the knobs, which serve the coarse pass too.  w.warp.vol == nullptr: no warp, (u, m) = 0 at every sample.
    // w.c.z is not read (the merged depths are in LDS) but must not be nullptr: composite_ray takes "the pass has explicit depths" from it
    WarpArgs w;
    // the COARSE pass, as composite_ray and sample_merge_ray read a CompositeArgs: S = S_c, z (the caller's or nullptr: the coarse spacing),
    // lindisp, n_importance = I, u; rgb / disp / acc = the coarse maps (all or none: coarse_maps), z_std, z_out = z_vals [N, S_c + I], each or nullptr
    CompositeArgs cc;
    int coarse_maps;
};

constexpr int HIER_MAX_COARSE = 256;        // EPL_C in 1 .. 4
constexpr int HIER_MAX_MERGED = 512;        // EPL_F in 1, 2, 3, 4, 6, 8

// one unit per coarse lane width (they build side by side): hipErrorInvalidValue when epl_class(a.cc.S) is not the unit's or a.w.c.S is beyond 512
hipError_t launch_hier_volume_c1(const HierArgs& a, int num_cus, hipStream_t stream);
hipError_t launch_hier_volume_c2(const HierArgs& a, int num_cus, hipStream_t stream);
hipError_t launch_hier_volume_c3(const HierArgs& a, int num_cus, hipStream_t stream);
hipError_t launch_hier_volume_c4(const HierArgs& a, int num_cus, hipStream_t stream);

// hipErrorInvalidValue for S_c outside 3 .. 256, I < 1 or S_c + I > 512 (nothing is launched).  `num_cus` sizes the grid of the ray loop; the
// result does not depend on it
inline hipError_t launch_hier_volume_render(const HierArgs& a, int num_cus, hipStream_t stream) {
    if (a.cc.S < 3 || a.cc.S > HIER_MAX_COARSE || a.cc.n_importance < 1 || a.w.c.S != a.cc.S + a.cc.n_importance || a.w.c.S > HIER_MAX_MERGED)
        return hipErrorInvalidValue;
    if (a.cc.n_rays <= 0) return hipSuccess;
    switch (epl_class(a.cc.S)) {
        case 1: return launch_hier_volume_c1(a, num_cus, stream);
        case 2: return launch_hier_volume_c2(a, num_cus, stream);
        case 3: return launch_hier_volume_c3(a, num_cus, stream);
        default: return launch_hier_volume_c4(a, num_cus, stream);
    }
}

}  // namespace nrn
