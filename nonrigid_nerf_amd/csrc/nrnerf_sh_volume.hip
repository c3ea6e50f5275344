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
#include <hip/hip_runtime.h>

#include "nrnerf_sh_volume.h"
#include "nrnerf_composite_ray.h"
#include "nrnerf_volume_lookup.h"

#ifndef NRN_SH_DEGREE
#error "NRN_SH_DEGREE: 1 or 2"
#endif

namespace nrn {

namespace {

constexpr int SH_WAVES = 4;             // waves (= rays in flight) per workgroup
constexpr int SH_MAXS = 1024;           // NRNERF_MAX_SAMPLES: EPL <= 16

// ---- the bent point.  bend / removed: the text of nrnerf_warp.hip's (tests/test_sh.py holds the two kernels to the same bits)
// (u, m) at p -> (bent xyz, m after the cutoff): rnh:563-570
__device__ __forceinline__ f32x4 bend(const WarpArgs& a, const float (&p)[3], const f32x4 um) {
    float m = um[3];
    if (a.has_cutoff && m <= a.cutoff) m = 0.0f;
    f32x4 b;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float off = rounded(m * um[c]);
        if (a.has_scaling) off = rounded(off * a.scaling);
        b[c] = __fadd_rn(p[c], off);
    }
    b[3] = m;
    return b;
}

// the removal knob on a sample's sigma logit (a product: NaN stays NaN)
__device__ __forceinline__ float removed(const WarpArgs& a, const float sigma, const float m) {
    return (a.has_removal && m >= a.removal) ? rounded(sigma * 0.0f) : sigma;
}

// (bent xyz, m) of sample ic of `ray` in one go: the caller's, the warp's, or the straight sample with m = 0
template <bool WHALF>
__device__ __forceinline__ f32x4 sample_bent(const ShVolumeArgs& a, const int ray, const int ic) {
    if (a.points4_in) return *(const __attribute__((address_space(1))) f32x4*)(gmem(a.points4_in) + ((size_t)ray * a.w.c.S + ic) * 4);
    const __attribute__((address_space(1))) float* rp = gmem(a.w.c.rays) + (size_t)ray * a.w.c.ray_stride;
    float p[3];
    sample_point(rp, sample_depth(a.w.c, rp, ray, ic), p);
    if (a.w.warp.vol) return bend(a.w, p, volume_at<WHALF>(a.w.warp, p[0], p[1], p[2]));
    const f32x4 b = {p[0], p[1], p[2], 0.0f};
    return b;
}

// ---- the direction.  e / (|e| + eps): DIFFERENCES has eps = 1e-6 (rnh:343-346), RAY eps = 0 (no sum is made)
__device__ __forceinline__ void unit_dir(const float ex, const float ey, const float ez, const bool with_eps, float (&d)[3]) {
    const float n = sqrtf(__fadd_rn(__fadd_rn(rounded(ex * ex), rounded(ey * ey)), rounded(ez * ez)));
    const float den = with_eps ? __fadd_rn(n, 1e-6f) : n;
    d[0] = __fdiv_rn(ex, den); d[1] = __fdiv_rn(ey, den); d[2] = __fdiv_rn(ez, den);
}
__device__ __forceinline__ void ray_dir(const __attribute__((address_space(1))) float* rp, float (&d)[3]) { unit_dir(rp[3], rp[4], rp[5], false, d); }
__device__ __forceinline__ void diff_dir(const f32x4 hi, const f32x4 lo, float (&d)[3]) {
    unit_dir(__fsub_rn(hi[0], lo[0]), __fsub_rn(hi[1], lo[1]), __fsub_rn(hi[2], lo[2]), true, d);
}

// ---- the basis: Y[k - 1] = Y_k(d), k = 1 .. (DEG + 1)^2 - 1, every product rounded (include/nrnerf.h)
template <int DEG>
__device__ __forceinline__ void sh_basis(const float (&d)[3], float (&Y)[(DEG + 1) * (DEG + 1) - 1]) {
    const float x = d[0], y = d[1], z = d[2];
    Y[0] = rounded(0.4886025119029199f * -y);
    Y[1] = rounded(0.4886025119029199f * z);
    Y[2] = rounded(0.4886025119029199f * -x);
    if constexpr (DEG >= 2) {
        const float xx = rounded(x * x), yy = rounded(y * y), zz = rounded(z * z);
        Y[3] = rounded(1.0925484305920792f * rounded(x * y));
        Y[4] = rounded(-1.0925484305920792f * rounded(y * z));
        Y[5] = rounded(0.31539156525252005f * __fsub_rn(__fsub_rn(rounded(2.0f * zz), xx), yy));
        Y[6] = rounded(-1.0925484305920792f * rounded(x * z));
        Y[7] = rounded(0.5462742152960396f * __fsub_rn(xx, yy));
    }
}

// ---- a sample's place in the volume's grid, found once: `raw` and every chunk of `sh` are gathered there
struct Cell {
    size_t v;                // the lowest corner's vertex index
    float f[3];
    bool ok;                 // false: the sample is empty
};
__device__ __forceinline__ void cell_of(const GridArgs& g, const f32x4 b, Cell& c) {
    int i[3];
    grid_cell(g, b[0], b[1], b[2], i, c.f, c.ok);
    c.v = (size_t)i[2] * ((size_t)g.g[0] * (size_t)g.g[1]) + (size_t)i[1] * (size_t)g.g[0] + (size_t)i[0];
}

// the requests for the eight corners of the four channels 4 j .. 4 j + 3 of an array with 4 * stride channels per vertex (none for an empty
// sample): grid_fetch's (nrnerf_volume_lookup.h) at a cell that is known, for grid_value to interpolate
template <bool HALF>
__device__ __forceinline__ void cell_fetch(const void* base, const GridArgs& g, const Cell& c, const int stride, const int j, GridFetch<HALF>& t) {
    typedef typename GridFetch<HALF>::vertex vertex;
    t.f[0] = c.f[0]; t.f[1] = c.f[1]; t.f[2] = c.f[2];
    t.ok = c.ok;
#pragma unroll
    for (int k = 0; k < 8; ++k) t.c[k] = vertex{};
    // (a condition of its own per request: the optimiser otherwise merges the requests of all chunks of a sample, which test the same flag, into
    // one block ahead of every interpolation -- 192 registers of corners at degree 2 -- and spills)
    int ok = c.ok;
    asm volatile("" : "+v"(ok));
    if (ok) {
        const size_t gx = (size_t)g.g[0], gxy = gx * (size_t)g.g[1];
        const __attribute__((address_space(1))) vertex* q = (const __attribute__((address_space(1))) vertex*)base + j;
        const size_t s = (size_t)stride;
        t.c[0] = q[c.v * s];                t.c[1] = q[(c.v + 1) * s];
        t.c[2] = q[(c.v + gx) * s];         t.c[3] = q[(c.v + gx + 1) * s];
        t.c[4] = q[(c.v + gxy) * s];        t.c[5] = q[(c.v + gxy + 1) * s];
        t.c[6] = q[(c.v + gxy + gx) * s];   t.c[7] = q[(c.v + gxy + gx + 1) * s];
    }
}

// the sums so far are computed HERE, before the next request's condition (cell_fetch: volatile statements keep their order).  Without it the
// optimiser sinks every chunk's interpolation and sum to the one place that uses the result, behind the last chunk's request, and all chunks'
// corners are live at once
__device__ __forceinline__ void pin(f32x4& col) {
    float c0 = col[0], c1 = col[1], c2 = col[2], c3 = col[3];
    asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
    col[0] = c0; col[1] = c1; col[2] = c2; col[3] = c3;
}

// chunk j's four interpolated channels folded into the colour sums: channel ch = 3 (k - 1) + c, ascending, so every colour sees its k ascending
template <int DEG>
__device__ __forceinline__ void fold(const float (&Y)[(DEG + 1) * (DEG + 1) - 1], const f32x4 v, const int j, f32x4& col) {
    constexpr int USED = 3 * ((DEG + 1) * (DEG + 1) - 1);           // 9 of 12, 24 of 24
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ch = 4 * j + e;
        if (ch < USED) col[ch % 3] = __fmaf_rn(Y[ch / 3], v[e], col[ch % 3]);
    }
    pin(col);
}

// the logits of ONE sample in one go (the lookup kernel): the render kernel's operations in its order
template <int DEG, bool VHALF>
__device__ __forceinline__ f32x4 sample_logits(const ShVolumeArgs& a, const f32x4 b, const float (&d)[3]) {
    constexpr int CHUNKS = 3 * DEG;
    Cell c;
    cell_of(a.w.vol, b, c);
    GridFetch<VHALF> t;
    cell_fetch<VHALF>(a.w.vol.vol, a.w.vol, c, 1, 0, t);
    f32x4 col = grid_value<VHALF>(t);
    col[3] = removed(a.w, col[3], b[3]);
    pin(col);
    float Y[(DEG + 1) * (DEG + 1) - 1];
    sh_basis<DEG>(d, Y);
#pragma unroll
    for (int j = 0; j < CHUNKS; ++j) {
        cell_fetch<VHALF>(a.sh, a.w.vol, c, CHUNKS, j, t);
        fold<DEG>(Y, grid_value<VHALF>(t), j, col);
    }
    return col;
}

template <int DEG, int EPL, bool VHALF, bool WHALF>
__global__ void __launch_bounds__(SH_WAVES * 64, 2) sh_render_kernel(const ShVolumeArgs a) {
    constexpr bool PIPE = EPL <= 4;             // two chunks of `sh` in flight (64 registers of corners in float32), else one
    constexpr bool PARK = EPL == 16;            // the samples' logits wait for composite_ray in LDS (a lane reads what it wrote: no barrier), else in registers
    constexpr bool EARLY = EPL <= 8;            // chunk 0 is requested together with raw's corners, else after raw is interpolated
    constexpr int CHUNKS = 3 * DEG;
    __shared__ f32x4 parked[PARK ? SH_WAVES * 64 * EPL : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = a.w.c.S;
    const bool warped = a.w.warp.vol != nullptr;
    const long long step = (long long)gridDim.x * SH_WAVES;
    for (long long rr = (long long)blockIdx.x * SH_WAVES + wave; rr < a.w.c.n_rays; rr += step) {
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

template <class KERNEL>
hipError_t launch(KERNEL kernel, const ShVolumeArgs& a, const dim3 grid, const dim3 block, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

template <int DEG, int EPL>
hipError_t launch_epl(const ShVolumeArgs& a, int num_cus, hipStream_t stream) {
    const long long want = ((long long)a.w.c.n_rays + SH_WAVES - 1) / SH_WAVES, cap = (long long)(num_cus > 0 ? num_cus : 256) * 16;
    const dim3 grid((unsigned)(want < cap ? want : cap)), block(SH_WAVES * 64);
    switch ((a.w.vol.half ? 2 : 0) | (a.w.warp.half ? 1 : 0)) {
        case 0: return launch(sh_render_kernel<DEG, EPL, false, false>, a, grid, block, stream);
        case 1: return launch(sh_render_kernel<DEG, EPL, false, true>, a, grid, block, stream);
        case 2: return launch(sh_render_kernel<DEG, EPL, true, false>, a, grid, block, stream);
        default: return launch(sh_render_kernel<DEG, EPL, true, true>, a, grid, block, stream);
    }
}

}  // namespace

template <>
hipError_t launch_sh_volume_render_degree<NRN_SH_DEGREE>(const ShVolumeArgs& a, int num_cus, hipStream_t stream) {
    constexpr int DEG = NRN_SH_DEGREE;
    if (a.w.c.S < 1 || a.w.c.S > SH_MAXS || a.degree != DEG || (!a.ray_dirs && a.w.c.S < 2)) return hipErrorInvalidValue;
    if (a.w.warp.vol && a.points4_in) return hipErrorInvalidValue;
    if (a.w.c.n_rays <= 0) return hipSuccess;
    if (!a.w.c.rgb) {                       // the lookup alone
        if (!a.w.raw_out && !a.w.points4_out) return hipErrorInvalidValue;
        const long long want = ((long long)a.w.c.n_rays * a.w.c.S + 255) / 256, cap = (long long)(num_cus > 0 ? num_cus : 256) * 32;
        const dim3 grid((unsigned)(want < cap ? want : cap)), block(256);
        switch ((a.w.vol.half ? 2 : 0) | (a.w.warp.half ? 1 : 0)) {
            case 0: return launch(sh_lookup_kernel<DEG, false, false>, a, grid, block, stream);
            case 1: return launch(sh_lookup_kernel<DEG, false, true>, a, grid, block, stream);
            case 2: return launch(sh_lookup_kernel<DEG, true, false>, a, grid, block, stream);
            default: return launch(sh_lookup_kernel<DEG, true, true>, a, grid, block, stream);
        }
    }
    return with_epl(a.w.c.S, [&](auto epl) { return launch_epl<DEG, epl()>(a, num_cus, stream); });
}

}  // namespace nrn
