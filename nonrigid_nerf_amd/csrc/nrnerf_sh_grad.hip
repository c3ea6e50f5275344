// nrnerf_sh_grad.hip -- the adjoint of the direction-dependent part of a view-dependent bake's colour logits,
//     s_c(b, d) = sum over k = 1 .. K - 1 of Y_k(d) v_{k,c}(b),
// v the `sh` array at the bent point b by THE VALUE AT A POINT, Y_k the basis polynomials: from the cotangents g_c of the logits, the gradient
// of the coefficients (d_sh[corner j, 3 (k - 1) + c] += w_j (Y_k g_c)), of the point (position part: scale * d/df of the interpolation) and of
// the direction (d_dirs = sum_k (sum_c g_c v_{k,c}) dY_k), and under DIFFERENCES the chain from the directions back to the bent points.  The rule
// is stated in include/nrnerf.h ("the adjoint of the colour sum") and, in float64, in tests/sh_grad_reference.py; resources and measurements:
// DESIGN.md section 3.18.  Three kernels, each a grid-stride loop without LDS; the cell and the fractions are grid_cell's, the direction and the
// basis the forward's device functions (nrnerf_baked_sample.h), so the two directions cannot disagree on the cell or on d.
//
// sh_scatter_kernel<DEG, LPP> (d_sh): LPP LANES PER POINT.  A vertex and its x-neighbour are one run of 2 * 12 DEG contiguous floats (96 / 192
// bytes); lane l of a point adds elements l, l + LPP, .. of that run in each of the four (y, z) rows, so one atomic instruction covers, per
// point, min(LPP, run) contiguous floats: float32 atomic adds to global memory without a return value (global_atomic_add_f32, no
// compare-and-swap loop).  The order of the sums is the order of arrival, so d_sh is NOT the same bits on every run.  The coefficients are not
// read.  At degree 1 the run's elements 9 .. 11 and 21 .. 23 (the zero channels) are skipped.  NRN_SH_SCATTER_LANES picks LPP (8, 16, 32 or
// 64; degree 1 takes at most 32, which covers its run): 64 -- one wave per point at degree 2, the whole 192-byte run in one instruction per
// row, 48 lanes at work -- added 0.76 TB/s against 0.49 / 0.42 / 0.47 at 32 / 16 / 8 lanes; degree 1 0.32 TB/s at 32 lanes (one 96-byte run per
// half wave) against 0.28 / 0.29 at 16 / 8.
// sh_point_dir_grad_kernel<DEG, HALF> (position part of d_points, d_dirs): one thread per sample; the corners arrive in chunks of four channels
// as the forward's do (cell_fetch); per chunk the corners are contracted with Y_k g_c into EIGHT scalars u_j and the chunk's interpolated
// value with g_c into the K - 1 sums t_k before the next chunk is asked for: eight + K - 1 accumulators and one chunk of corners are live.  The
// position part is the derivative of the trilinear interpolation of the eight scalars (section 3.15's ddx / ddy / ddz forms).  One writer per
// element and a fixed operation order: the same bits on every run.
// sh_direction_chain_kernel (direction part of d_points, DIFFERENCES): one thread per sample, no grid: d_i = e_i / (n_i + eps), e_i = b_i -
// b_{i-1}, so E_i = G_i / (n_i + eps) - e_i (G_i . e_i) / (n_i (n_i + eps)^2) goes to b_i and -E_i to b_{i-1}; G_i = d_dirs[i], G_1 = d_dirs[1] +
// d_dirs[0] (d_0 = d_1).  The thread of sample i adds E_i and subtracts E_{i+1}; it runs after the kernel above on the same stream.
// Every multiply-add is spelled __fmaf_rn and every product that feeds a sum or a difference goes through rounded(), as in the forward.
#include <hip/hip_runtime.h>

#include "nrnerf_sh_grad.h"
#include "nrnerf_composite_ray.h"
#include "nrnerf_volume_lookup.h"
#include "nrnerf_baked_sample.h"

#ifndef NRN_SH_SCATTER_LANES
#define NRN_SH_SCATTER_LANES 64
#endif

namespace nrn {

namespace {

constexpr float SH_C1 = 0.4886025119029199f, SH_C2 = 1.0925484305920792f, SH_C20 = 0.31539156525252005f, SH_C22 = 0.5462742152960396f;

__device__ __forceinline__ f32x4 quad_at(const float* base, const long long t) {
    return *(const __attribute__((address_space(1))) f32x4*)(gmem(base) + (size_t)t * 4);
}

// the direction of sample i of `ray` (t = ray * S + i, b its bent point): the forward's, by the call's mode
__device__ __forceinline__ void sample_dir(const ShGradArgs& a, const int ray, const int i, const long long t, const f32x4 b, float (&d)[3]) {
    if (a.ray_dirs) ray_dir(gmem(a.rays) + (size_t)ray * a.ray_stride, d);
    else if (i == 0) diff_dir(quad_at(a.points4, t + 1), b, d);         // d_0 = d_1
    else diff_dir(b, quad_at(a.points4, t - 1), d);
}

// v_k for a k known at run time, by selects on values: no indexed array (a loop over an array here is still a loop when the optimiser
// decides where the array lives, and the array then goes to LDS)
__device__ __forceinline__ float pick3(const int k, const float v0, const float v1, const float v2) { return k == 0 ? v0 : k == 1 ? v1 : v2; }
template <int DEG>
__device__ __forceinline__ float pick_basis(const float (&Y)[(DEG + 1) * (DEG + 1) - 1], const int k) {
    const float lo = pick3(k, Y[0], Y[1], Y[2]);
    if constexpr (DEG >= 2) {
        const float mid = pick3(k - 3, Y[3], Y[4], Y[5]), hi = k == 6 ? Y[6] : Y[7];
        return k < 3 ? lo : k < 6 ? mid : hi;
    }
    return lo;
}

__device__ __forceinline__ float lerp1(const float a, const float b, const float f) { return __fmaf_rn(f, b, __fmaf_rn(-f, a, a)); }

// thread t: lane t % LPP of sample t / LPP; an empty sample (outside the box, or NaN) adds nothing
template <int DEG, int LPP>
__global__ void __launch_bounds__(256) sh_scatter_kernel(const ShGradArgs a) {
    constexpr int K1 = (DEG + 1) * (DEG + 1) - 1, C = 12 * DEG, USED = 3 * K1, RUN = 2 * C, ITERS = (RUN + LPP - 1) / LPP;
    const long long total = (long long)a.n_rays * a.S * LPP, step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const unsigned pt = (unsigned)(t / LPP);           // (fewer than 2^31 samples: the divisions are 32-bit)
        const int l = (int)t & (LPP - 1);
        const int ray = (int)(pt / (unsigned)a.S), i = (int)(pt - (unsigned)ray * (unsigned)a.S);
        const f32x4 b = quad_at(a.points4, pt);
        int ci[3];
        float f[3];
        bool ok;
        grid_cell(a.grid, b[0], b[1], b[2], ci, f, ok);
        if (!ok) continue;
        float d[3], Y[K1];
        sample_dir(a, ray, i, pt, b, d);
        sh_basis<DEG>(d, Y);
        const f32x4 g4 = quad_at(a.g_raw, pt);
        const size_t gx = (size_t)a.grid.g[0], gxy = gx * (size_t)a.grid.g[1];
        const size_t v = (size_t)ci[2] * gxy + (size_t)ci[1] * gx + (size_t)ci[0];
        const float wy[2] = {__fsub_rn(1.0f, f[1]), f[1]}, wz[2] = {__fsub_rn(1.0f, f[2]), f[2]};
#pragma unroll
        for (int r = 0; r < ITERS; ++r) {
            const int e = l + r * LPP;                      // the element of the run: vertex v's channels, then vertex v + 1's
            if (RUN % LPP != 0 && e >= RUN) continue;
            const int dx = e >= C ? 1 : 0, ch = e - dx * C;
            if (USED < C && ch >= USED) continue;           // degree 1: channels 9 .. 11 are never touched
            const int k = ch / 3, c = ch - 3 * k;
            const float yg = rounded(pick_basis<DEG>(Y, k) * pick3(c, g4[0], g4[1], g4[2]));
            const float wx = dx ? f[0] : __fsub_rn(1.0f, f[0]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float w = rounded(rounded(wx * wy[q & 1]) * wz[q >> 1]);
                unsafeAtomicAdd(a.d_sh + (v + (q & 1) * gx + (q >> 1) * gxy) * C + e, rounded(w * yg));
            }
        }
    }
}

template <int DEG, bool HALF>
__global__ void __launch_bounds__(256) sh_point_dir_grad_kernel(const ShGradArgs a) {
    constexpr int K1 = (DEG + 1) * (DEG + 1) - 1, CHUNKS = 3 * DEG, USED = 3 * K1;
    const long long total = (long long)a.n_rays * a.S, step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const int ray = (int)((unsigned)t / (unsigned)a.S), i = (int)((unsigned)t - (unsigned)ray * (unsigned)a.S);      // (fewer than 2^31 samples)
        const f32x4 b = quad_at(a.points4, t);
        Cell cell;
        cell_of(a.grid, b, cell);
        float dp[3] = {0.0f, 0.0f, 0.0f}, dd[3] = {0.0f, 0.0f, 0.0f};          // outside the box, or NaN: no gradient
        if (cell.ok) {
            float d[3], Y[K1];
            sample_dir(a, ray, i, t, b, d);
            sh_basis<DEG>(d, Y);
            const f32x4 g = quad_at(a.g_raw, t);
            float u[8], T[K1];
#pragma unroll
            for (int q = 0; q < 8; ++q) u[q] = 0.0f;
#pragma unroll
            for (int k = 0; k < K1; ++k) T[k] = 0.0f;
#pragma unroll
            for (int j = 0; j < CHUNKS; ++j) {
                GridFetch<HALF> tf;
                cell_fetch<HALF>(a.grid.vol, a.grid, cell, CHUNKS, j, tf);
                const f32x4 val = grid_value<HALF>(tf);                         // the forward's v of these four channels
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ch = 4 * j + e;
                    if (ch < USED) {
                        const int k = ch / 3, c = ch % 3;
                        const float yg = rounded(Y[k] * g[c]);
#pragma unroll
                        for (int q = 0; q < 8; ++q) u[q] = __fmaf_rn(yg, (float)tf.c[q][e], u[q]);
                        T[k] = __fmaf_rn(g[c], val[e], T[k]);
                    }
                }
                // the sums so far are computed HERE, before the next chunk's request (pin, nrnerf_baked_sample.h)
#pragma unroll
                for (int q = 0; q < 8; ++q) asm volatile("" : "+v"(u[q]));
#pragma unroll
                for (int k = 0; k < K1; ++k) asm volatile("" : "+v"(T[k]));
            }
            // the derivative of the trilinear interpolation of the eight scalars (corner q: bit 0 = x, bit 1 = y, bit 2 = z)
            const float* const f = cell.f;
            const float ddx = lerp1(lerp1(__fsub_rn(u[1], u[0]), __fsub_rn(u[3], u[2]), f[1]), lerp1(__fsub_rn(u[5], u[4]), __fsub_rn(u[7], u[6]), f[1]), f[2]);
            const float x00 = lerp1(u[0], u[1], f[0]), x10 = lerp1(u[2], u[3], f[0]), x01 = lerp1(u[4], u[5], f[0]), x11 = lerp1(u[6], u[7], f[0]);
            const float ddy = lerp1(__fsub_rn(x10, x00), __fsub_rn(x11, x01), f[2]);
            const float ddz = lerp1(__fsub_rn(x01, x00), __fsub_rn(x11, x10), f[1]);
            dp[0] = rounded(a.grid.scale[0] * ddx);
            dp[1] = rounded(a.grid.scale[1] * ddy);
            dp[2] = rounded(a.grid.scale[2] * ddz);
            // d_dirs[axis] = sum over k of t_k dY_k / d axis, k ascending
            const float x = d[0], y = d[1], z = d[2];
            dd[0] = rounded(-SH_C1 * T[2]);
            dd[1] = rounded(-SH_C1 * T[0]);
            dd[2] = rounded(SH_C1 * T[1]);
            if constexpr (DEG >= 2) {
                dd[0] = __fmaf_rn(rounded(SH_C2 * y), T[3], dd[0]);
                dd[1] = __fmaf_rn(rounded(SH_C2 * x), T[3], dd[1]);
                dd[1] = __fmaf_rn(rounded(-SH_C2 * z), T[4], dd[1]);
                dd[2] = __fmaf_rn(rounded(-SH_C2 * y), T[4], dd[2]);
                dd[0] = __fmaf_rn(rounded(-2.0f * SH_C20 * x), T[5], dd[0]);
                dd[1] = __fmaf_rn(rounded(-2.0f * SH_C20 * y), T[5], dd[1]);
                dd[2] = __fmaf_rn(rounded(4.0f * SH_C20 * z), T[5], dd[2]);
                dd[0] = __fmaf_rn(rounded(-SH_C2 * z), T[6], dd[0]);
                dd[2] = __fmaf_rn(rounded(-SH_C2 * x), T[6], dd[2]);
                dd[0] = __fmaf_rn(rounded(2.0f * SH_C22 * x), T[7], dd[0]);
                dd[1] = __fmaf_rn(rounded(-2.0f * SH_C22 * y), T[7], dd[1]);
            }
        }
        if (a.d_points) {
            __attribute__((address_space(1))) float* out = gmem(a.d_points) + (size_t)t * 3;
            out[0] = dp[0]; out[1] = dp[1]; out[2] = dp[2];
        }
        if (a.d_dirs) {
            __attribute__((address_space(1))) float* out = gmem(a.d_dirs) + (size_t)t * 3;
            out[0] = dd[0]; out[1] = dd[1]; out[2] = dd[2];
        }
    }
}

// E_i of the difference between samples t and t - 1 of one ray (i >= 1); G_1 takes d_dirs[0] with it
__device__ __forceinline__ void chain_term(const ShGradArgs& a, const long long t, const int i, float (&E)[3]) {
    const f32x4 hi = quad_at(a.points4, t), lo = quad_at(a.points4, t - 1);
    const float e[3] = {__fsub_rn(hi[0], lo[0]), __fsub_rn(hi[1], lo[1]), __fsub_rn(hi[2], lo[2])};
    const __attribute__((address_space(1))) float* gd = gmem(a.d_dirs) + (size_t)t * 3;
    float G[3] = {gd[0], gd[1], gd[2]};
    if (i == 1) { G[0] = __fadd_rn(G[0], gd[-3]); G[1] = __fadd_rn(G[1], gd[-2]); G[2] = __fadd_rn(G[2], gd[-1]); }
    const float n = sqrtf(__fadd_rn(__fadd_rn(rounded(e[0] * e[0]), rounded(e[1] * e[1])), rounded(e[2] * e[2])));      // the forward's n
    const float den = __fadd_rn(n, 1e-6f);
    const float dot = __fmaf_rn(G[2], e[2], __fmaf_rn(G[1], e[1], rounded(G[0] * e[0])));
    const float coef = n == 0.0f ? 0.0f : __fdiv_rn(dot, rounded(rounded(n * den) * den));      // coincident points: the second term is 0
#pragma unroll
    for (int c = 0; c < 3; ++c) E[c] = __fsub_rn(__fdiv_rn(G[c], den), rounded(e[c] * coef));
}

__global__ void __launch_bounds__(256) sh_direction_chain_kernel(const ShGradArgs a) {
    const long long total = (long long)a.n_rays * a.S, step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const int i = (int)((unsigned)t % (unsigned)a.S);
        __attribute__((address_space(1))) float* out = gmem(a.d_points) + (size_t)t * 3;
        float dp[3] = {out[0], out[1], out[2]}, E[3];
        if (i >= 1) {
            chain_term(a, t, i, E);
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[c] = __fadd_rn(dp[c], E[c]);
        }
        if (i <= a.S - 2) {
            chain_term(a, t + 1, i + 1, E);
#pragma unroll
            for (int c = 0; c < 3; ++c) dp[c] = __fsub_rn(dp[c], E[c]);
        }
        out[0] = dp[0]; out[1] = dp[1]; out[2] = dp[2];
    }
}

template <class KERNEL>
hipError_t launch(KERNEL kernel, const ShGradArgs& a, const long long threads, const long long cap, hipStream_t stream) {
    const long long want = (threads + 255) / 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sh_lookup_backward(const ShGradArgs& a, int num_cus, hipStream_t stream) {
    constexpr int LPP = NRN_SH_SCATTER_LANES;
    static_assert(LPP == 8 || LPP == 16 || LPP == 32 || LPP == 64, "NRN_SH_SCATTER_LANES: 8, 16, 32 or 64");
    constexpr int LPP1 = LPP > 32 ? 32 : LPP;          // degree 1: the run is 24 floats, 32 lanes cover it
    if (a.degree != 1 && a.degree != 2) return hipErrorInvalidValue;
    if (!a.d_sh && !a.d_points && !a.d_dirs) return hipErrorInvalidValue;
    if (!a.ray_dirs && (a.S < 2 || (a.d_points && !a.d_dirs))) return hipErrorInvalidValue;
    if (a.n_rays <= 0 || a.S <= 0) return hipSuccess;
    if ((long long)a.n_rays * a.S >= (1ll << 31)) return hipErrorInvalidValue;
    const long long samples = (long long)a.n_rays * a.S, cap = (long long)(num_cus > 0 ? num_cus : 256) * 32;
    hipError_t e = hipSuccess;
    if (a.d_sh) {
        e = a.degree == 1 ? launch(sh_scatter_kernel<1, LPP1>, a, samples * LPP1, cap, stream) : launch(sh_scatter_kernel<2, LPP>, a, samples * LPP, cap, stream);
        if (e != hipSuccess) return e;
    }
    if (a.d_points || a.d_dirs) {
        switch ((a.degree == 2 ? 2 : 0) | (a.grid.half ? 1 : 0)) {
            case 0: e = launch(sh_point_dir_grad_kernel<1, false>, a, samples, cap, stream); break;
            case 1: e = launch(sh_point_dir_grad_kernel<1, true>, a, samples, cap, stream); break;
            case 2: e = launch(sh_point_dir_grad_kernel<2, false>, a, samples, cap, stream); break;
            default: e = launch(sh_point_dir_grad_kernel<2, true>, a, samples, cap, stream); break;
        }
        if (e != hipSuccess) return e;
    }
    if (a.d_points && !a.ray_dirs) e = launch(sh_direction_chain_kernel, a, samples, cap, stream);
    return e;
}

}  // namespace nrn
