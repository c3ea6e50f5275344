// nrnerf_sh_volume.hip -- a baked scene with a view-dependent head rendered with no network: nrnerf_warp.hip's kernel with, per sample, the
// colour logits of a direction instead of one colour: raw (the mean over directions) plus the real spherical harmonics of degree 1 .. DEG at the
// sample's direction times the coefficients of the `sh` array at the bent point.  The value rule is stated in include/nrnerf.h ("view-dependent
// bakes") and, in float64, in tests/sh_reference.py; layout, resources and measurements: DESIGN.md section 3.16.
//
// sh_render_kernel<DEG, EPL, VHALF, WHALF>: warped_render_kernel's mapping -- one wave per ray at a time, rays handed out by a grid-stride loop
// (no atomics, no device counter: the same bits on every run), lane l owns the EPL consecutive samples l*EPL .. l*EPL+EPL-1, one at a
// time.  Per sample the bent point (the warp's, the caller's points4_in, or the straight sample), then the cell and the fractions in the volume's
// grid ONCE (grid_cell): `raw` and every chunk of `sh` are gathered at that cell.  `sh` is gathered in chunks of four channels -- 3 (degree 1) or
// 6 (degree 2) of them -- and each chunk is interpolated (lerp4, as the volume's channels) and folded into the three colour sums before the
// next one is interpolated: the eight corners of one chunk are 32 registers in float32, all 24 channels' would be 192.
// The direction of a sample under DIFFERENCES needs the bent point before it.  Inside a lane that is the previous sample's; the first sample of
// lane l needs the last one of lane l - 1, which that lane only knows at the end of its own loop -- too late for a cross-lane move unless
// every bent point of the ray is kept (4 * EPL registers more).  The lane bends that ONE neighbour again instead (lane 0: sample 1, d_0 = d_1):
// one warp gather in EPL more, of a coarse grid that sits in cache.
// sh_lookup_kernel<DEG, VHALF, WHALF>: the same device functions, one thread per sample, no compositing: the render kernel's raw / points4 bits.
// No multiply-add is fused that the rule does not name: every product that feeds a sum goes through rounded() (nrnerf_volume_lookup.h).
// One translation unit per degree (NRN_SH_DEGREE), so that the two build side by side.
// The device functions of a sample (bend, removed, sample_bent, unit_dir, sh_basis, Cell, cell_of, cell_fetch, pin, fold, sample_logits) live
// in nrnerf_baked_sample.h, shared with nrnerf_warp.hip and nrnerf_culled_volume.hip.
// culled_sh_render_kernel / culled_lookup_kernel (nrnerf_culled_volume.hip) are sh_render_kernel's / sh_lookup_kernel's text with the occupancy
// mask in cell_of: two texts, because shared behind a function they measured slower.  The launch idiom:
// nrnerf_baked_launch.h.
#include <hip/hip_runtime.h>

#include "nrnerf_sh_volume.h"
#include "nrnerf_baked_launch.h"
#include "nrnerf_composite_ray.h"
#include "nrnerf_volume_lookup.h"
#include "nrnerf_baked_sample.h"

#ifndef NRN_SH_DEGREE
#error "NRN_SH_DEGREE: 1 or 2"
#endif

namespace nrn {

namespace {

template <int DEG, int EPL, bool VHALF, bool WHALF>
__global__ void __launch_bounds__(BAKED_WAVES * 64, 2) sh_render_kernel(const ShVolumeArgs a) {
    constexpr bool PIPE = EPL <= 4;             // two chunks of `sh` in flight (64 registers of corners in float32), else one
    constexpr bool PARK = EPL == 16;            // the samples' logits wait for composite_ray in LDS (a lane reads what it wrote: no barrier), else in registers
    constexpr bool EARLY = EPL <= 8;            // chunk 0 is requested together with raw's corners, else after raw is interpolated
    constexpr int CHUNKS = 3 * DEG;
    __shared__ f32x4 parked[PARK ? BAKED_WAVES * 64 * EPL : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = a.w.c.S;
    const bool warped = a.w.warp.vol != nullptr;
    const long long step = (long long)gridDim.x * BAKED_WAVES;
    for (long long rr = (long long)blockIdx.x * BAKED_WAVES + wave; rr < a.w.c.n_rays; rr += step) {
        const int ray = (int)rr;
        const __attribute__((address_space(1))) float* rp = gmem(a.w.c.rays) + (size_t)ray * a.w.c.ray_stride;
        f32x4 raw[PARK ? 1 : EPL];
        float d[3] = {0.0f, 0.0f, 0.0f};
        f32x4 prev = {0.0f, 0.0f, 0.0f, 0.0f};          // the bent point before the sample at hand (lane 0, first sample: the one after it)
        if (a.ray_dirs) ray_dir(rp, d);
        else {
            const int nb = lane == 0 ? 1 : (lane * EPL - 1 < S ? lane * EPL - 1 : S - 1);
            prev = sample_bent<WHALF>(a, ray, nb);
        }
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
            const int i = lane * EPL + k, ic = i < S ? i : S - 1;          // (beyond S: the last sample's, as composite_ray asks for)
            f32x4 b;
            if (a.points4_in) b = *(const __attribute__((address_space(1))) f32x4*)(gmem(a.points4_in) + ((size_t)ray * S + ic) * 4);
            else {
                float p[3];
                sample_point(rp, sample_depth(a.w.c, rp, ray, ic), p);
                b[0] = p[0]; b[1] = p[1]; b[2] = p[2]; b[3] = 0.0f;
                if (warped) {
                    GridFetch<WHALF> tw;
                    grid_fetch<WHALF>(a.w.warp, p[0], p[1], p[2], tw);
                    b = bend(a.w, p, grid_value<WHALF>(tw));
                }
            }
            Cell cell;
            GridFetch<VHALF> tv, tu;
            cell_of(a.w.vol, b, cell);
            cell_fetch<VHALF>(a.w.vol.vol, a.w.vol, cell, 1, 0, tv);
            if (EARLY) cell_fetch<VHALF>(a.sh, a.w.vol, cell, CHUNKS, 0, tu);
            if (!a.ray_dirs) {
                const bool first = lane == 0 && k == 0;                     // d_0 = d_1: `prev` holds sample 1
                diff_dir(first ? prev : b, first ? b : prev, d);
                prev = b;
            }
            float Y[(DEG + 1) * (DEG + 1) - 1];
            sh_basis<DEG>(d, Y);
            f32x4 acc = grid_value<VHALF>(tv);
            acc[3] = removed(a.w, acc[3], b[3]);
            pin(acc);
            if (!EARLY) cell_fetch<VHALF>(a.sh, a.w.vol, cell, CHUNKS, 0, tu);
            // the chunks (chunk 0 is in tu).  PIPE: two in flight, chunk j + 1 is requested before chunk j is
            // interpolated; else one.  pin() in fold keeps each chunk's interpolation where it is written
#pragma unroll
            for (int j = 0; j < CHUNKS; ++j) {
                GridFetch<VHALF>& cur = (PIPE && (j & 1)) ? tv : tu;
                GridFetch<VHALF>& nxt = (PIPE && (j & 1)) ? tu : tv;
                if (PIPE && j + 1 < CHUNKS) cell_fetch<VHALF>(a.sh, a.w.vol, cell, CHUNKS, j + 1, nxt);
                fold<DEG>(Y, grid_value<VHALF>(cur), j, acc);
                if (!PIPE && j + 1 < CHUNKS) cell_fetch<VHALF>(a.sh, a.w.vol, cell, CHUNKS, j + 1, tu);
            }
            if constexpr (PARK) parked[(wave * EPL + k) * 64 + lane] = acc;
            else raw[k] = acc;
            if (i < S) {
                if (a.w.raw_out) *(__attribute__((address_space(1))) f32x4*)(gmem(a.w.raw_out) + ((size_t)ray * S + i) * 4) = acc;
                if (a.w.points4_out) *(__attribute__((address_space(1))) f32x4*)(gmem(a.w.points4_out) + ((size_t)ray * S + i) * 4) = b;
            }
        }
        // composite_ray asks for this lane's samples once each, in order k = 0 .. EPL-1: the k-th request is answered from the k-th register,
        // as in warped_render_kernel
        int next = 0;
        float z[EPL + 1], w[EPL];
        composite_ray<EPL>(a.w.c, ray, true, lane, [&](int) { if constexpr (PARK) return parked[(wave * EPL + next++) * 64 + lane]; else return raw[next++]; }, z, w);

        // ---- the surface outputs, as warped_render_kernel has them: the sample surface_index picks, its bent point and mask once more
        if (a.w.surf_pts || a.w.surf_rig || a.w.med_idx) {
            const int bidx = surface_index<EPL>(w, lane, S);
            if (lane == 0) {
                const f32x4 s = sample_bent<WHALF>(a, ray, bidx);
                if (a.w.surf_pts) { gmem(a.w.surf_pts)[(size_t)ray * 3] = s[0]; gmem(a.w.surf_pts)[(size_t)ray * 3 + 1] = s[1]; gmem(a.w.surf_pts)[(size_t)ray * 3 + 2] = s[2]; }
                if (a.w.surf_rig) gmem(a.w.surf_rig)[ray] = s[3];
                if (a.w.med_idx) gmem(a.w.med_idx)[ray] = bidx;
            }
        }
    }
}

template <int DEG, bool VHALF, bool WHALF>
__global__ void __launch_bounds__(256) sh_lookup_kernel(const ShVolumeArgs a) {
    const int S = a.w.c.S;
    const long long total = (long long)a.w.c.n_rays * S, step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const int ray = (int)(t / S), i = (int)(t % S);
        const f32x4 b = sample_bent<WHALF>(a, ray, i);
        if (a.w.points4_out) *(__attribute__((address_space(1))) f32x4*)(gmem(a.w.points4_out) + (size_t)t * 4) = b;
        if (a.w.raw_out) {
            float d[3];
            if (a.ray_dirs) ray_dir(gmem(a.w.c.rays) + (size_t)ray * a.w.c.ray_stride, d);
            else if (i == 0) diff_dir(sample_bent<WHALF>(a, ray, 1), b, d);      // d_0 = d_1
            else diff_dir(b, sample_bent<WHALF>(a, ray, i - 1), d);
            *(__attribute__((address_space(1))) f32x4*)(gmem(a.w.raw_out) + (size_t)t * 4) = sample_logits<DEG, VHALF>(a, b, d);
        }
    }
}

}  // namespace

template <>
hipError_t launch_sh_volume_render_degree<NRN_SH_DEGREE>(const ShVolumeArgs& a, int num_cus, hipStream_t stream) {
    constexpr int DEG = NRN_SH_DEGREE;
    if (a.w.c.S < 1 || a.w.c.S > BAKED_MAXS || a.degree != DEG || (!a.ray_dirs && a.w.c.S < 2)) return hipErrorInvalidValue;
    if (a.w.warp.vol && a.points4_in) return hipErrorInvalidValue;
    if (a.w.c.n_rays <= 0) return hipSuccess;
    if (!a.w.c.rgb) {                       // the lookup alone
        if (!a.w.raw_out && !a.w.points4_out) return hipErrorInvalidValue;
        return with_storage(a.w.vol.half, a.w.warp.half, [&](auto vh, auto wh) {
            return launch(sh_lookup_kernel<DEG, vh(), wh()>, a, sample_grid(a.w.c.n_rays, a.w.c.S, num_cus), dim3(256), stream);
        });
    }
    return with_epl(a.w.c.S, [&](auto epl) {
        return with_storage(a.w.vol.half, a.w.warp.half, [&](auto vh, auto wh) {
            return launch(sh_render_kernel<DEG, epl(), vh(), wh()>, a, ray_loop_grid(a.w.c.n_rays, num_cus), dim3(BAKED_WAVES * 64), stream);
        });
    });
}

}  // namespace nrn
