// nrnerf_warp.hip -- a baked scene rendered with no network: per sample the ray bender's (offset, rigidity mask) from a coarse grid baked per
// time step, the bend with its test-time knobs, the canonical volume's logits at the bent point, then the alpha compositing of
// nrnerf_composite_ray.h -- ONE kernel, nothing per sample goes through memory.  The value rule is stated in include/nrnerf.h ("baked warps")
// and, in float64, in tests/warp_reference.py; layout, resources and measurements: DESIGN.md section 3.14.
//
// warped_render_kernel<EPL, VHALF, WHALF>: volume_render_kernel's mapping (nrnerf_volume.hip) -- one wave per ray at a time, rays handed out by
// a grid-stride loop (no atomics, no device counter: the same bits on every run), lane l owns the EPL consecutive samples l*EPL .. l*EPL+EPL-1.
// The two gathers of a sample depend on each other, so a lane works on GROUP samples at a time (all EPL up to 4; 3 of 6; 2 of 8 and 12; 1 of
// 16): the warp corners of the whole group are requested before the first of them is interpolated, every bent point's canonical corners are
// requested as soon as it is known, and the canonical interpolations start when all of the group's requests are out.  The corners of a group
// are GROUP * 64 registers in float32: beyond EPL = 4 the groups are sized so that, next to raw[EPL], every instantiation stays within 256
// VGPRs and parks nothing in AGPRs.  An empty sample requests nothing.  composite_ray<EPL> then runs on the registers.
// The surface outputs: composite_ray reads the bent point of the sample surface_index picks from memory, where this kernel has none; it calls
// surface_index itself on the weights composite_ray returns, and lane 0 bends the one sample it picks again.
// warped_lookup_kernel<VHALF, WHALF>: the same per-sample rule, one thread per sample, no compositing.
// No multiply-add is fused that the rule does not name: every product that feeds a sum goes through rounded() (nrnerf_volume_lookup.h).
// bend / removed / sample_bent live in nrnerf_baked_sample.h, shared with nrnerf_sh_volume.hip and nrnerf_culled_volume.hip.
// culled_render_kernel (nrnerf_culled_volume.hip) is warped_render_kernel's text with the point source as a parameter and the occupancy mask in
// grid_fetch: two texts, because shared behind a function they measured slower.  The launch idiom: nrnerf_baked_launch.h.
#include <hip/hip_runtime.h>

#include "nrnerf_warp.h"
#include "nrnerf_baked_launch.h"
#include "nrnerf_composite_ray.h"
#include "nrnerf_volume_lookup.h"
#include "nrnerf_baked_sample.h"

namespace nrn {

namespace {

template <int EPL, bool VHALF, bool WHALF>
__global__ void __launch_bounds__(BAKED_WAVES * 64) warped_render_kernel(const WarpArgs a) {
    constexpr int GROUP = gather_group(EPL);
    static_assert(EPL % GROUP == 0, "whole groups");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = a.c.S;
    const long long step = (long long)gridDim.x * BAKED_WAVES;
    for (long long rr = (long long)blockIdx.x * BAKED_WAVES + wave; rr < a.c.n_rays; rr += step) {
        const int ray = (int)rr;
        const __attribute__((address_space(1))) float* rp = gmem(a.c.rays) + (size_t)ray * a.c.ray_stride;
        f32x4 raw[EPL];
#pragma unroll
        for (int g0 = 0; g0 < EPL; g0 += GROUP) {
            float p[GROUP][3];
            GridFetch<WHALF> tw[GROUP];
            GridFetch<VHALF> tv[GROUP];
            f32x4 b[GROUP];
#pragma unroll
            for (int k = 0; k < GROUP; ++k) {
                const int i = lane * EPL + g0 + k;
                sample_point(rp, sample_depth(a.c, rp, ray, i < S ? i : S - 1), p[k]);       // (beyond S: the last sample's, as composite_ray asks for)
                grid_fetch<WHALF>(a.warp, p[k][0], p[k][1], p[k][2], tw[k]);
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
                    if (a.raw_out) *(__attribute__((address_space(1))) f32x4*)(gmem(a.raw_out) + ((size_t)ray * S + i) * 4) = raw[g0 + k];
                    if (a.points4_out) *(__attribute__((address_space(1))) f32x4*)(gmem(a.points4_out) + ((size_t)ray * S + i) * 4) = b[k];
                }
            }
        }
        // composite_ray asks for this lane's samples once each, in order k = 0 .. EPL-1 (its loading loop, fully unrolled): the k-th request
        // is answered from the k-th register, as in volume_render_kernel
        int next = 0;
        float z[EPL + 1], w[EPL];
        composite_ray<EPL>(a.c, ray, true, lane, [&](int) { return raw[next++]; }, z, w);

        // ---- the surface outputs: the sample surface_index picks on the weights composite_ray returned, bent again; its bent point and mask
        if (a.surf_pts || a.surf_rig || a.med_idx) {
            const int bidx = surface_index<EPL>(w, lane, S);
            if (lane == 0) {
                const f32x4 s = sample_bent<WHALF>(a, ray, bidx);
                if (a.surf_pts) { gmem(a.surf_pts)[(size_t)ray * 3] = s[0]; gmem(a.surf_pts)[(size_t)ray * 3 + 1] = s[1]; gmem(a.surf_pts)[(size_t)ray * 3 + 2] = s[2]; }
                if (a.surf_rig) gmem(a.surf_rig)[ray] = s[3];
                if (a.med_idx) gmem(a.med_idx)[ray] = bidx;
            }
        }
    }
}

template <bool VHALF, bool WHALF>
__global__ void __launch_bounds__(256) warped_lookup_kernel(const WarpArgs a) {
    const int S = a.c.S;
    const long long total = (long long)a.c.n_rays * S, step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const int ray = (int)(t / S), i = (int)(t % S);
        const f32x4 b = sample_bent<WHALF>(a, ray, i);
        if (a.points4_out) *(__attribute__((address_space(1))) f32x4*)(gmem(a.points4_out) + (size_t)t * 4) = b;
        if (a.raw_out)
            *(__attribute__((address_space(1))) f32x4*)(gmem(a.raw_out) + (size_t)t * 4) = removed(a, volume_at<VHALF>(a.vol, b[0], b[1], b[2]), b[3]);
    }
}

}  // namespace

hipError_t launch_warped_volume_render(const WarpArgs& a, int num_cus, hipStream_t stream) {
    if (a.c.S < 1 || a.c.S > BAKED_MAXS) return hipErrorInvalidValue;
    if (a.c.n_rays <= 0) return hipSuccess;
    if (!a.c.rgb) {                         // the lookup alone
        if (!a.raw_out && !a.points4_out) return hipErrorInvalidValue;
        return with_storage(a.vol.half, a.warp.half, [&](auto vh, auto wh) {
            return launch(warped_lookup_kernel<vh(), wh()>, a, sample_grid(a.c.n_rays, a.c.S, num_cus), dim3(256), stream);
        });
    }
    return with_epl(a.c.S, [&](auto epl) {
        return with_storage(a.vol.half, a.warp.half, [&](auto vh, auto wh) {
            return launch(warped_render_kernel<epl(), vh(), wh()>, a, ray_loop_grid(a.c.n_rays, num_cus), dim3(BAKED_WAVES * 64), stream);
        });
    });
}

}  // namespace nrn
