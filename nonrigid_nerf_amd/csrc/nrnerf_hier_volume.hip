// nrnerf_hier_volume.hip -- hierarchical sampling of a baked scene in ONE kernel: the coarse pass of warped_render_kernel (nrnerf_warp.hip),
// sample_pdf + z_std + the merge of sample_merge_ray (nrnerf_composite_ray.h), and the fine pass at the merged depths, which never leave the
// wave's LDS -- neither `raw [N, S_c, 4]` nor `z [N, S_c + I]` goes through memory.  The value rule is the composition of the three calls it
// replaces (include/nrnerf.h, "hierarchical sampling of a baked scene"); layout, resources and measurements: DESIGN.md section 3.19.
//
// hier_render_kernel<EPL_C, EPL_F, VHALF, WHALF>: warped_render_kernel's mapping -- one wave per ray at a time, four waves per workgroup, rays
// handed out by a grid-stride loop (no atomics, no device counter: the same bits on every run).  Lane l owns the coarse samples l * EPL_C .. and
// then the merged samples l * EPL_F ..; both passes gather in warped_render_kernel's groups (gather_ray below is its sample loop, with the
// depth of a sample handed in and "no warp" as one more case).  The waves of a workgroup run different numbers of rays, so nothing in the loop
// is a workgroup barrier: the phases of a ray are ordered by ray_phase_sync<true> (the LDS areas are private to the wave), one more of them at
// the end of an iteration, before the next ray's cdf overwrites the merged depths the fine pass has just read.
// LDS of a wave: s_z [64 * EPL_F] (the S_c + I depths to merge), then s_cdf / s_bins [64 * EPL_C] each; the merged depths lie over s_cdf and
// s_bins -- dead once the importance depths are drawn -- and whatever they need beyond: at most 1024 floats per wave, 16 KiB per workgroup.
// One object per EPL_C (NRN_HIER_EPL_C = 1 .. 4), so that the four build side by side; EPL_F runs over the widths >= EPL_C up to 8.
#include <hip/hip_runtime.h>

#include "nrnerf_hier_volume.h"
#include "nrnerf_baked_launch.h"
#include "nrnerf_composite_ray.h"
#include "nrnerf_volume_lookup.h"
#include "nrnerf_baked_sample.h"

#ifndef NRN_HIER_EPL_C
#error "NRN_HIER_EPL_C = 1 .. 4: the coarse lane width of this unit"
#endif
static_assert(NRN_FUSE_PREFETCH >= 2, "the fine pass hands composite_ray its depths through `pre`");

namespace nrn {

namespace {

// the sample loop of warped_render_kernel for the S samples of one pass: sample i lies at depth_at(i); raw[k] = the logits of sample
// lane * EPL + k (beyond S: the last sample's, as composite_ray asks for).  No warp: an empty request, (u, m) = 0
template <int EPL, bool VHALF, bool WHALF, class DEPTH>
__device__ __forceinline__ void gather_ray(const WarpArgs& a, const __attribute__((address_space(1))) float* rp, const int ray, const int lane,
                                           const int S, DEPTH&& depth_at, f32x4 (&raw)[EPL], float* raw_out, float* points4_out) {
    constexpr int GROUP = gather_group(EPL);
    static_assert(EPL % GROUP == 0, "whole groups");
    const bool has_warp = a.warp.vol != nullptr;
#pragma unroll
    for (int g0 = 0; g0 < EPL; g0 += GROUP) {
        float p[GROUP][3];
        GridFetch<WHALF> tw[GROUP];
        GridFetch<VHALF> tv[GROUP];
        f32x4 b[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            const int i = lane * EPL + g0 + k;
            sample_point(rp, depth_at(i < S ? i : S - 1), p[k]);
            if (has_warp) grid_fetch<WHALF>(a.warp, p[k][0], p[k][1], p[k][2], tw[k]);
            else {
                tw[k].ok = false;
                tw[k].f[0] = tw[k].f[1] = tw[k].f[2] = 0.0f;
#pragma unroll
                for (int c = 0; c < 8; ++c) tw[k].c[c] = typename GridFetch<WHALF>::vertex{};
            }
        }
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            b[k] = bend(a, p[k], grid_value<WHALF>(tw[k]));
            grid_fetch<VHALF>(a.vol, b[k][0], b[k][1], b[k][2], tv[k]);
        }
#pragma unroll
        for (int k = 0; k < GROUP; ++k) {
            const int i = lane * EPL + g0 + k;
            raw[g0 + k] = removed(a, grid_value<VHALF>(tv[k]), b[k][3]);
            if (i < S) {
                if (raw_out) *(__attribute__((address_space(1))) f32x4*)(gmem(raw_out) + ((size_t)ray * S + i) * 4) = raw[g0 + k];
                if (points4_out) *(__attribute__((address_space(1))) f32x4*)(gmem(points4_out) + ((size_t)ray * S + i) * 4) = b[k];
            }
        }
    }
}

template <int EPL_C, int EPL_F, bool VHALF, bool WHALF>
__global__ void __launch_bounds__(BAKED_WAVES * 64) hier_render_kernel(const HierArgs a) {
    static_assert(EPL_F >= EPL_C, "the merged depths hold the coarse ones");
    constexpr int NC = 64 * EPL_C, NF = 64 * EPL_F;
    constexpr int NM = 2 * NC > NF ? 2 * NC : NF;            // the merged depths lie over s_cdf and s_bins
    __shared__ float lds[BAKED_WAVES][NF + NM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* const s_z = lds[wave];
    float* const s_cdf = s_z + NF;
    float* const s_bins = s_cdf + NC;
    float* const s_m = s_cdf;
    const int Sc = a.cc.S, Sf = a.w.c.S;
    const long long step = (long long)gridDim.x * BAKED_WAVES;
    for (long long rr = (long long)blockIdx.x * BAKED_WAVES + wave; rr < a.cc.n_rays; rr += step) {
        const int ray = (int)rr;
        const __attribute__((address_space(1))) float* rp = gmem(a.cc.rays) + (size_t)ray * a.cc.ray_stride;
        // ---- the coarse pass: its maps (when asked for), its depths and weights for the sampling
        {
            float z[EPL_C + 1], w[EPL_C];
            {
                f32x4 raw[EPL_C];
                gather_ray<EPL_C, VHALF, WHALF>(a.w, rp, ray, lane, Sc, [&](int ic) { return sample_depth(a.cc, rp, ray, ic); }, raw, nullptr, nullptr);
                int next = 0;
                composite_ray<EPL_C>(a.cc, ray, a.coarse_maps != 0, lane, [&](int) { return raw[next++]; }, z, w);
            }
            // ---- inverse CDF, z_std, stable merge: the S_c + I depths in rank order at s_m
            sample_merge_ray<EPL_C, true, true>(a.cc, ray, true, lane, z, w, s_cdf, s_bins, s_z, s_m);
        }
        ray_phase_sync<true>();
        // ---- the fine pass at the merged depths
        f32x4 raw[EPL_F];
        gather_ray<EPL_F, VHALF, WHALF>(a.w, rp, ray, lane, Sf, [&](int ic) { return s_m[ic]; }, raw, a.w.raw_out, a.w.points4_out);
        float pre[3 + EPL_F];
        pre[0] = rp[3]; pre[1] = rp[4]; pre[2] = rp[5];
#pragma unroll
        for (int k = 0; k < EPL_F; ++k) {
            const int i = lane * EPL_F + k;
            pre[3 + k] = s_m[i < Sf ? i : Sf - 1];
        }
        int next = 0;
        float z[EPL_F + 1], w[EPL_F];
        composite_ray<EPL_F>(a.w.c, ray, true, lane, [&](int) { return raw[next++]; }, z, w, pre);
        // ---- the surface outputs, as warped_render_kernel's: the picked sample bent again by lane 0
        if (a.w.surf_pts || a.w.surf_rig || a.w.med_idx) {
            const int bidx = surface_index<EPL_F>(w, lane, Sf);
            if (lane == 0) {
                float p[3];
                sample_point(rp, s_m[bidx], p);
                const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
                const f32x4 s = bend(a.w, p, a.w.warp.vol ? volume_at<WHALF>(a.w.warp, p[0], p[1], p[2]) : zero);
                if (a.w.surf_pts) { gmem(a.w.surf_pts)[(size_t)ray * 3] = s[0]; gmem(a.w.surf_pts)[(size_t)ray * 3 + 1] = s[1]; gmem(a.w.surf_pts)[(size_t)ray * 3 + 2] = s[2]; }
                if (a.w.surf_rig) gmem(a.w.surf_rig)[ray] = s[3];
                if (a.w.med_idx) gmem(a.w.med_idx)[ray] = bidx;
            }
        }
        ray_phase_sync<true>();         // the next ray's cdf and depths overwrite what this one has just read
    }
}

template <int EPL_C, int EPL_F>
hipError_t launch_epl(const HierArgs& a, int num_cus, hipStream_t stream) {
    if constexpr (EPL_F < EPL_C || EPL_F > 8) {
        return hipErrorInvalidValue;
    } else {
        return with_storage(a.w.vol.half, a.w.warp.half, [&](auto vh, auto wh) {
            return launch(hier_render_kernel<EPL_C, EPL_F, vh(), wh()>, a, ray_loop_grid(a.cc.n_rays, num_cus), dim3(BAKED_WAVES * 64), stream);
        });
    }
}

}  // namespace

#define NRN_HIER_CAT2(x, y) x##y
#define NRN_HIER_CAT(x, y) NRN_HIER_CAT2(x, y)
hipError_t NRN_HIER_CAT(launch_hier_volume_c, NRN_HIER_EPL_C)(const HierArgs& a, int num_cus, hipStream_t stream) {
    if (epl_class(a.cc.S) != NRN_HIER_EPL_C || a.cc.S < 3 || a.cc.n_importance < 1 || a.w.c.S != a.cc.S + a.cc.n_importance ||
        a.w.c.S > HIER_MAX_MERGED || !a.w.c.z)
        return hipErrorInvalidValue;
    if (a.cc.n_rays <= 0) return hipSuccess;
    return with_epl(a.w.c.S, [&](auto epl) { return launch_epl<NRN_HIER_EPL_C, epl()>(a, num_cus, stream); });
}

}  // namespace nrn
