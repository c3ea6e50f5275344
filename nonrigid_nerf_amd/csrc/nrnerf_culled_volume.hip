// nrnerf_culled_volume.hip -- a baked scene rendered with no network, skipping empty space: the kernels of nrnerf_warp.hip (degree 0) and
// nrnerf_sh_volume.hip (degree 1 / 2) with ONE addition -- after the cell of a sample's bent point is known, the lane reads the bit of the
// cell's block in the occupancy mask and ANDs it into the sample's "not empty" flag, before any corner of `raw` or of a chunk of `sh` is
// requested.  A sample in an empty block is the value rule's empty sample: raw = 0, v = 0, nothing requested.  With a mask built at threshold 0
// every weight such a sample would have had is exactly +0, so every composited output keeps its bits (include/nrnerf.h, "occupancy masks";
// in float64: tests/occupancy_reference.py; layout, resources and measurements: DESIGN.md section 3.17).
//
// culled_render_kernel<EPL, VHALF, SRC, WHALF> (degree 0): warped_render_kernel's mapping and groups -- one wave per ray at a time, rays
// handed out by a grid-stride loop, lane l owns the EPL consecutive samples l*EPL .. l*EPL+EPL-1, GROUP samples' requests in flight -- serving
// the three point sources of the view-dependent call.  The source is a template parameter (SRC: straight samples, ready-made points4_in, a
// warp): chosen at run time inside one kernel, the allocator keeps the warp's and the volume's corners of a group apart and the EPL = 4 kernel
// needs 358 registers instead of 217.
// culled_sh_render_kernel<DEG, EPL, VHALF, WHALF> (degree 1 / 2): sh_render_kernel's text with the masked cell.
// The mask is a policy of the shared lookup (BlockMask: grid_fetch, nrnerf_volume_lookup.h; cell_of and sample_logits, nrnerf_baked_sample.h).
// The ray loops are texts of their own next to the unmasked kernels': shared behind a function they measured slower.
// culled_lookup_kernel<DEG, VHALF, WHALF>: the same device functions, one thread per sample, no compositing: the render kernels' raw / points4
// bits.
// The mask is read through global memory: a 256^3 volume at the default block is 4 KiB of words, which every wave of a CU keeps hitting in the
// vector L1; the word's load depends on the cell alone and is one more request ahead of the eight of the corners (a copy in LDS has no room at
// EPL = 16, whose parked logits take the 64 KiB a workgroup may have).  No atomics, no device counter: the same bits on every run.
// One translation unit per degree (NRN_CULL_DEGREE), so that the three build side by side.
#include <hip/hip_runtime.h>

#include "nrnerf_culled_volume.h"
#include "nrnerf_baked_launch.h"
#include "nrnerf_baked_sample.h"

#ifndef NRN_CULL_DEGREE
#error "NRN_CULL_DEGREE: 0, 1 or 2"
#endif

namespace nrn {

namespace {

__device__ __forceinline__ BlockMask block_mask(const CulledVolumeArgs& a) { return BlockMask{a.occ, a.k, {a.nb[0], a.nb[1]}}; }

// the surface outputs, as the parents have them: the sample surface_index picks on the weights composite_ray returned, bent again
template <int EPL, bool WHALF>
__device__ __forceinline__ void surface_outputs(const ShVolumeArgs& a, const int ray, const int lane, const float (&w)[EPL]) {
    if (a.w.surf_pts || a.w.surf_rig || a.w.med_idx) {
        const int bidx = surface_index<EPL>(w, lane, a.w.c.S);
        if (lane == 0) {
            const f32x4 s = sample_bent<WHALF>(a, ray, bidx);
            if (a.w.surf_pts) { gmem(a.w.surf_pts)[(size_t)ray * 3] = s[0]; gmem(a.w.surf_pts)[(size_t)ray * 3 + 1] = s[1]; gmem(a.w.surf_pts)[(size_t)ray * 3 + 2] = s[2]; }
            if (a.w.surf_rig) gmem(a.w.surf_rig)[ray] = s[3];
            if (a.w.med_idx) gmem(a.w.med_idx)[ray] = bidx;
        }
    }
}

constexpr int SRC_STRAIGHT = 0, SRC_POINTS4 = 1, SRC_WARP = 2;

template <int EPL, bool VHALF, int SRC, bool WHALF>
__global__ void __launch_bounds__(BAKED_WAVES * 64) culled_render_kernel(const CulledVolumeArgs a) {
    constexpr bool WARPED = SRC == SRC_WARP;
    constexpr int GROUP = gather_group(EPL);
    static_assert(EPL % GROUP == 0, "whole groups");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WarpArgs& w = a.s.w;
    const int S = w.c.S;
    const long long step = (long long)gridDim.x * BAKED_WAVES;
    for (long long rr = (long long)blockIdx.x * BAKED_WAVES + wave; rr < w.c.n_rays; rr += step) {
        const int ray = (int)rr;
        const __attribute__((address_space(1))) float* rp = gmem(w.c.rays) + (size_t)ray * w.c.ray_stride;
        f32x4 raw[EPL];
#pragma unroll
        for (int g0 = 0; g0 < EPL; g0 += GROUP) {
            float p[GROUP][3], m[GROUP];                // the point before the warp acts, and the mask of a point that no warp bends
            GridFetch<WHALF> tw[GROUP];
            GridFetch<VHALF> tv[GROUP];
            f32x4 b[GROUP];
#pragma unroll
            for (int k = 0; k < GROUP; ++k) {
                const int i = lane * EPL + g0 + k, ic = i < S ? i : S - 1;            // (beyond S: the last sample's, as composite_ray asks for)
                m[k] = 0.0f;
                if constexpr (SRC == SRC_POINTS4) {
                    const f32x4 q = *(const __attribute__((address_space(1))) f32x4*)(gmem(a.s.points4_in) + ((size_t)ray * S + ic) * 4);
                    p[k][0] = q[0]; p[k][1] = q[1]; p[k][2] = q[2]; m[k] = q[3];
                } else sample_point(rp, sample_depth(w.c, rp, ray, ic), p[k]);
                if constexpr (WARPED) grid_fetch<WHALF>(w.warp, p[k][0], p[k][1], p[k][2], tw[k]);
            }
#pragma unroll
            for (int k = 0; k < GROUP; ++k) {
                if constexpr (WARPED) b[k] = bend(w, p[k], grid_value<WHALF>(tw[k]));
                else { b[k][0] = p[k][0]; b[k][1] = p[k][1]; b[k][2] = p[k][2]; b[k][3] = m[k]; }
                grid_fetch<VHALF>(w.vol, b[k][0], b[k][1], b[k][2], tv[k], block_mask(a));
            }
#pragma unroll
            for (int k = 0; k < GROUP; ++k) {
                const int i = lane * EPL + g0 + k;
                raw[g0 + k] = removed(w, grid_value<VHALF>(tv[k]), b[k][3]);
                if (i < S) {
                    if (w.raw_out) *(__attribute__((address_space(1))) f32x4*)(gmem(w.raw_out) + ((size_t)ray * S + i) * 4) = raw[g0 + k];
                    if (w.points4_out) *(__attribute__((address_space(1))) f32x4*)(gmem(w.points4_out) + ((size_t)ray * S + i) * 4) = b[k];
                }
            }
        }
        // composite_ray asks for this lane's samples once each, in order k = 0 .. EPL-1: the k-th request is answered from the k-th register
        int next = 0;
        float z[EPL + 1], wt[EPL];
        composite_ray<EPL>(w.c, ray, true, lane, [&](int) { return raw[next++]; }, z, wt);
        surface_outputs<EPL, WHALF>(a.s, ray, lane, wt);
    }
}

template <int DEG, int EPL, bool VHALF, bool WHALF>
__global__ void __launch_bounds__(BAKED_WAVES * 64, 2) culled_sh_render_kernel(const CulledVolumeArgs a) {
    constexpr bool PIPE = EPL <= 4;             // two chunks of `sh` in flight (64 registers of corners in float32), else one
    constexpr bool PARK = EPL == 16;            // the samples' logits wait for composite_ray in LDS (a lane reads what it wrote: no barrier), else in registers
    constexpr bool EARLY = EPL <= 8;            // chunk 0 is requested together with raw's corners, else after raw is interpolated
    constexpr int CHUNKS = 3 * DEG;
    __shared__ f32x4 parked[PARK ? BAKED_WAVES * 64 * EPL : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ShVolumeArgs& s = a.s;
    const int S = s.w.c.S;
    const bool warped = s.w.warp.vol != nullptr;
    const long long step = (long long)gridDim.x * BAKED_WAVES;
    for (long long rr = (long long)blockIdx.x * BAKED_WAVES + wave; rr < s.w.c.n_rays; rr += step) {
        const int ray = (int)rr;
        const __attribute__((address_space(1))) float* rp = gmem(s.w.c.rays) + (size_t)ray * s.w.c.ray_stride;
        f32x4 raw[PARK ? 1 : EPL];
        float d[3] = {0.0f, 0.0f, 0.0f};
        f32x4 prev = {0.0f, 0.0f, 0.0f, 0.0f};          // the bent point before the sample at hand (lane 0, first sample: the one after it)
        if (s.ray_dirs) ray_dir(rp, d);
        else {
            const int nb = lane == 0 ? 1 : (lane * EPL - 1 < S ? lane * EPL - 1 : S - 1);
            prev = sample_bent<WHALF>(s, ray, nb);
        }
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
            const int i = lane * EPL + k, ic = i < S ? i : S - 1;          // (beyond S: the last sample's, as composite_ray asks for)
            f32x4 b;
            if (s.points4_in) b = *(const __attribute__((address_space(1))) f32x4*)(gmem(s.points4_in) + ((size_t)ray * S + ic) * 4);
            else {
                float p[3];
                sample_point(rp, sample_depth(s.w.c, rp, ray, ic), p);
                b[0] = p[0]; b[1] = p[1]; b[2] = p[2]; b[3] = 0.0f;
                if (warped) {
                    GridFetch<WHALF> tw;
                    grid_fetch<WHALF>(s.w.warp, p[0], p[1], p[2], tw);
                    b = bend(s.w, p, grid_value<WHALF>(tw));
                }
            }
            Cell cell;
            GridFetch<VHALF> tv, tu;
            cell_of(s.w.vol, b, cell, block_mask(a));            // the block's bit is in cell.ok before the first request
            cell_fetch<VHALF>(s.w.vol.vol, s.w.vol, cell, 1, 0, tv);
            if (EARLY) cell_fetch<VHALF>(s.sh, s.w.vol, cell, CHUNKS, 0, tu);
            if (!s.ray_dirs) {
                const bool first = lane == 0 && k == 0;                     // d_0 = d_1: `prev` holds sample 1
                diff_dir(first ? prev : b, first ? b : prev, d);
                prev = b;
            }
            float Y[(DEG + 1) * (DEG + 1) - 1];
            sh_basis<DEG>(d, Y);
            f32x4 acc = grid_value<VHALF>(tv);
            acc[3] = removed(s.w, acc[3], b[3]);
            pin(acc);
            if (!EARLY) cell_fetch<VHALF>(s.sh, s.w.vol, cell, CHUNKS, 0, tu);
            // the chunks (chunk 0 is in tu).  PIPE: two in flight, chunk j + 1 is requested before chunk j is
            // interpolated; else one.  pin() in fold keeps each chunk's interpolation where it is written
#pragma unroll
            for (int j = 0; j < CHUNKS; ++j) {
                GridFetch<VHALF>& cur = (PIPE && (j & 1)) ? tv : tu;
                GridFetch<VHALF>& nxt = (PIPE && (j & 1)) ? tu : tv;
                if (PIPE && j + 1 < CHUNKS) cell_fetch<VHALF>(s.sh, s.w.vol, cell, CHUNKS, j + 1, nxt);
                fold<DEG>(Y, grid_value<VHALF>(cur), j, acc);
                if (!PIPE && j + 1 < CHUNKS) cell_fetch<VHALF>(s.sh, s.w.vol, cell, CHUNKS, j + 1, tu);
            }
            if constexpr (PARK) parked[(wave * EPL + k) * 64 + lane] = acc;
            else raw[k] = acc;
            if (i < S) {
                if (s.w.raw_out) *(__attribute__((address_space(1))) f32x4*)(gmem(s.w.raw_out) + ((size_t)ray * S + i) * 4) = acc;
                if (s.w.points4_out) *(__attribute__((address_space(1))) f32x4*)(gmem(s.w.points4_out) + ((size_t)ray * S + i) * 4) = b;
            }
        }
        // composite_ray asks for this lane's samples once each, in order k = 0 .. EPL-1: the k-th request is answered from the k-th register
        int next = 0;
        float z[EPL + 1], wt[EPL];
        composite_ray<EPL>(s.w.c, ray, true, lane, [&](int) { if constexpr (PARK) return parked[(wave * EPL + next++) * 64 + lane]; else return raw[next++]; }, z, wt);
        surface_outputs<EPL, WHALF>(s, ray, lane, wt);
    }
}

template <int DEG, bool VHALF, bool WHALF>
__global__ void __launch_bounds__(256) culled_lookup_kernel(const CulledVolumeArgs a) {
    const ShVolumeArgs& s = a.s;
    const int S = s.w.c.S;
    const long long total = (long long)s.w.c.n_rays * S, step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const int ray = (int)(t / S), i = (int)(t % S);
        const f32x4 b = sample_bent<WHALF>(s, ray, i);
        if (s.w.points4_out) *(__attribute__((address_space(1))) f32x4*)(gmem(s.w.points4_out) + (size_t)t * 4) = b;
        if (s.w.raw_out) {
            float d[3] = {0.0f, 0.0f, 0.0f};
            if constexpr (DEG >= 1) {
                if (s.ray_dirs) ray_dir(gmem(s.w.c.rays) + (size_t)ray * s.w.c.ray_stride, d);
                else if (i == 0) diff_dir(sample_bent<WHALF>(s, ray, 1), b, d);      // d_0 = d_1
                else diff_dir(b, sample_bent<WHALF>(s, ray, i - 1), d);
            }
            *(__attribute__((address_space(1))) f32x4*)(gmem(s.w.raw_out) + (size_t)t * 4) = sample_logits<DEG, VHALF>(s, b, d, block_mask(a));
        }
    }
}

template <int DEG, int EPL>
hipError_t launch_epl(const CulledVolumeArgs& a, int num_cus, hipStream_t stream) {
    const dim3 grid = ray_loop_grid(a.s.w.c.n_rays, num_cus), block(BAKED_WAVES * 64);
    if constexpr (DEG == 0) {
        // without a warp its storage is no parameter
        if (a.s.points4_in) {
            if (a.s.w.vol.half) return launch(culled_render_kernel<EPL, true, SRC_POINTS4, false>, a, grid, block, stream);
            return launch(culled_render_kernel<EPL, false, SRC_POINTS4, false>, a, grid, block, stream);
        }
        if (!a.s.w.warp.vol) {
            if (a.s.w.vol.half) return launch(culled_render_kernel<EPL, true, SRC_STRAIGHT, false>, a, grid, block, stream);
            return launch(culled_render_kernel<EPL, false, SRC_STRAIGHT, false>, a, grid, block, stream);
        }
        return with_storage(a.s.w.vol.half, a.s.w.warp.half, [&](auto vh, auto wh) {
            return launch(culled_render_kernel<EPL, vh(), SRC_WARP, wh()>, a, grid, block, stream);
        });
    } else {
        return with_storage(a.s.w.vol.half, a.s.w.warp.half, [&](auto vh, auto wh) {
            return launch(culled_sh_render_kernel<DEG, EPL, vh(), wh()>, a, grid, block, stream);
        });
    }
}

}  // namespace

template <>
hipError_t launch_culled_volume_render_degree<NRN_CULL_DEGREE>(const CulledVolumeArgs& a, int num_cus, hipStream_t stream) {
    constexpr int DEG = NRN_CULL_DEGREE;
    const WarpArgs& w = a.s.w;
    if (w.c.S < 1 || w.c.S > BAKED_MAXS || a.s.degree != DEG || (DEG >= 1 && !a.s.ray_dirs && w.c.S < 2)) return hipErrorInvalidValue;
    if (w.warp.vol && a.s.points4_in) return hipErrorInvalidValue;
    // (noise and the range of k are launch_culled_volume_render's checks, the one caller: nrnerf_culled_volume.h)
    if (!a.occ) return hipErrorInvalidValue;
    if (a.nb[0] != occupancy_blocks(w.vol.g[0], a.k) || a.nb[1] != occupancy_blocks(w.vol.g[1], a.k)) return hipErrorInvalidValue;
    if (w.c.n_rays <= 0) return hipSuccess;
    if (!w.c.rgb) {                         // the lookup alone
        if (!w.raw_out && !w.points4_out) return hipErrorInvalidValue;
        return with_storage(w.vol.half, w.warp.half, [&](auto vh, auto wh) {
            return launch(culled_lookup_kernel<DEG, vh(), wh()>, a, sample_grid(w.c.n_rays, w.c.S, num_cus), dim3(256), stream);
        });
    }
    return with_epl(w.c.S, [&](auto epl) { return launch_epl<DEG, epl()>(a, num_cus, stream); });
}

}  // namespace nrn
