// nrnerf_volume.hip -- a baked volume of the field rendered by lookup: per sample the trilinear interpolation of the volume's (r, g, b, sigma)
// logits at the sample's (bent) point, then the alpha compositing of nrnerf_composite_ray.h.  The sampling rule is stated in include/nrnerf.h
// ("baked volumes") and, in float64, in tests/volume_reference.py; layout, resources and measurements: DESIGN.md section 3.13.
//
// volume_render_kernel<EPL, HALF>: one wave per ray at a time, rays handed out by a grid-stride loop (no atomics, no device counter: the same
// bits on every run).  Lane l owns the EPL consecutive samples l*EPL .. l*EPL+EPL-1 -- composite_ray's mapping -- so a lane's points4 loads are
// 16 * EPL contiguous bytes, coalesced across the wave.  Each lane gathers its samples' logits ONCE into registers (eight corners per sample:
// four pairs of x-neighbours, a pair adjacent in memory and requested together), then composite_ray<EPL> runs on those registers.
// volume_lookup_kernel<HALF>: the same per-sample device function, one thread per sample, the logits alone (no compositing).
// The lookup itself (lerp4 / load_pair / volume_at) lives in nrnerf_volume_lookup.h, shared with the other baked render kernels; the launch
// idiom is theirs too (nrnerf_baked_launch.h).
// Every multiply-add is spelled __fmaf_rn and every product that feeds a sum or a difference goes through rounded(): this build's
// -ffp-contract=fast would otherwise fuse them per instantiation (nrnerf_composite_ray.h), and the two kernels must give the same bits.
#include <hip/hip_runtime.h>

#include "nrnerf_volume.h"
#include "nrnerf_baked_launch.h"
#include "nrnerf_composite_ray.h"
#include "nrnerf_volume_lookup.h"

namespace nrn {

namespace {

// the logits of sample ic (< S) of `ray`: its point (points4, or sample_point at sample_depth),
// the lookup, the removal knob
template <bool HALF>
__device__ __forceinline__ f32x4 sample_logits(const VolumeArgs& a, const int ray, const int ic) {
    const int S = a.c.S;
    float p[3], rig = 0.0f;
    if (a.points4) {
        const f32x4 q = *(const __attribute__((address_space(1))) f32x4*)(gmem(a.points4) + ((size_t)ray * S + ic) * 4);
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; rig = q[3];
    } else {
        const __attribute__((address_space(1))) float* rp = gmem(a.c.rays) + (size_t)ray * a.c.ray_stride;
        sample_point(rp, sample_depth(a.c, rp, ray, ic), p);
    }
    f32x4 r = volume_at<HALF>(a.grid, p[0], p[1], p[2]);
    if (a.has_removal && rig >= a.removal) r[3] = rounded(r[3] * 0.0f);          // rnh:308-311 (a product: NaN stays NaN)
    return r;
}

template <int EPL, bool HALF>
__global__ void __launch_bounds__(BAKED_WAVES * 64) volume_render_kernel(const VolumeArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = a.c.S;
    const long long step = (long long)gridDim.x * BAKED_WAVES;
    for (long long rr = (long long)blockIdx.x * BAKED_WAVES + wave; rr < a.c.n_rays; rr += step) {
        const int ray = (int)rr;
        f32x4 raw[EPL];
#pragma unroll
        for (int k = 0; k < EPL; ++k) {
            const int i = lane * EPL + k;
            raw[k] = sample_logits<HALF>(a, ray, i < S ? i : S - 1);           // (beyond S: the last sample's, as composite_ray asks for)
            if (a.raw_out && i < S) *(__attribute__((address_space(1))) f32x4*)(gmem(a.raw_out) + ((size_t)ray * S + i) * 4) = raw[k];
        }
        // composite_ray asks for this lane's samples once each, in order k = 0 .. EPL-1 (its loading loop, fully unrolled): the k-th request
        // is answered from the k-th register -- a compile-time index after unrolling, no gather is repeated and nothing is indexed dynamically
        int next = 0;
        float z[EPL + 1], w[EPL];
        composite_ray<EPL>(a.c, ray, true, lane, [&](int) { return raw[next++]; }, z, w);
    }
}

template <bool HALF>
__global__ void __launch_bounds__(256) volume_lookup_kernel(const VolumeArgs a) {
    const int S = a.c.S;
    const long long total = (long long)a.c.n_rays * S, step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const int ray = (int)(t / S), i = (int)(t % S);
        *(__attribute__((address_space(1))) f32x4*)(gmem(a.raw_out) + (size_t)t * 4) = sample_logits<HALF>(a, ray, i);
    }
}

}  // namespace

hipError_t launch_volume_render(const VolumeArgs& a, int num_cus, hipStream_t stream) {
    if (a.c.S < 1 || a.c.S > BAKED_MAXS) return hipErrorInvalidValue;
    if (a.c.n_rays <= 0) return hipSuccess;
    if (!a.c.rgb) {                         // the lookup alone
        if (!a.raw_out) return hipErrorInvalidValue;
        const dim3 grid = sample_grid(a.c.n_rays, a.c.S, num_cus);
        if (a.grid.half) return launch(volume_lookup_kernel<true>, a, grid, dim3(256), stream);
        return launch(volume_lookup_kernel<false>, a, grid, dim3(256), stream);
    }
    return with_epl(a.c.S, [&](auto epl) {
        const dim3 grid = ray_loop_grid(a.c.n_rays, num_cus), block(BAKED_WAVES * 64);
        if (a.grid.half) return launch(volume_render_kernel<epl(), true>, a, grid, block, stream);
        return launch(volume_render_kernel<epl(), false>, a, grid, block, stream);
    });
}

}  // namespace nrn
