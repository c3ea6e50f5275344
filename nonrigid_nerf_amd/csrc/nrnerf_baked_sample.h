// nrnerf_baked_sample.h -- the device functions of ONE sample of a baked render: the bend with its knobs, the removal knob, a sample's bent
// point in one go, its direction, the spherical-harmonic basis, its place in the volume's grid (Cell, with the occupancy mask as a policy:
// NoMask / BlockMask of nrnerf_volume_lookup.h) with the requests made there, the fold of a chunk of coefficients into the colour sums, and a
// sample's logits in one go.  The render kernels of nrnerf_warp.hip, nrnerf_sh_volume.hip, nrnerf_culled_volume.hip and nrnerf_hier_volume.hip stand on these; the
// adjoint of nrnerf_sh_grad.hip takes its cell, direction and basis from here.  The value rules: include/nrnerf.h ("baked warps",
// "view-dependent bakes", "occupancy masks").
// No multiply-add is fused that the rule does not name: every product that feeds a sum goes through rounded() (nrnerf_volume_lookup.h).
#pragma once
#include <hip/hip_runtime.h>

#include "nrnerf_sh_volume.h"
#include "nrnerf_composite_ray.h"
#include "nrnerf_volume_lookup.h"

namespace nrn {

namespace {

// ---- the samples of a lane whose requests are in flight together in a degree-0 gather (nrnerf_warp.hip has the reasoning): all EPL up to 4,
// 3 of 6, 2 of 8 and 12, 1 of 16
constexpr int gather_group(const int EPL) { return EPL <= 4 ? EPL : (EPL == 6 ? 3 : (EPL == 16 ? 1 : 2)); }

// ---- the bent point
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

// the removal knob on a sample's logits (a product: NaN stays NaN)
__device__ __forceinline__ f32x4 removed(const WarpArgs& a, f32x4 r, const float m) {
    if (a.has_removal && m >= a.removal) r[3] = rounded(r[3] * 0.0f);
    return r;
}

// the removal knob on a sample's sigma logit (a product: NaN stays NaN)
__device__ __forceinline__ float removed(const WarpArgs& a, const float sigma, const float m) {
    return (a.has_removal && m >= a.removal) ? rounded(sigma * 0.0f) : sigma;
}

// sample ic of `ray` in one go: (bent xyz, m)
template <bool WHALF>
__device__ __forceinline__ f32x4 sample_bent(const WarpArgs& a, const int ray, const int ic) {
    const __attribute__((address_space(1))) float* rp = gmem(a.c.rays) + (size_t)ray * a.c.ray_stride;
    float p[3];
    sample_point(rp, sample_depth(a.c, rp, ray, ic), p);
    return bend(a, p, volume_at<WHALF>(a.warp, p[0], p[1], p[2]));
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
// (a sample in an empty block of `mask` is an empty sample: the block's bit is in c.ok before the first request)
template <class MASK = NoMask>
__device__ __forceinline__ void cell_of(const GridArgs& g, const f32x4 b, Cell& c, const MASK mask = MASK{}) {
    int i[3];
    grid_cell(g, b[0], b[1], b[2], i, c.f, c.ok);
    c.v = (size_t)i[2] * ((size_t)g.g[0] * (size_t)g.g[1]) + (size_t)i[1] * (size_t)g.g[0] + (size_t)i[0];
    if constexpr (MASK::on) c.ok = c.ok && mask.bit(i);
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

// the logits of ONE sample in one go (the lookup kernel): the render kernel's operations in its order.  Degree 0: raw after the removal knob,
// `d` is not read
template <int DEG, bool VHALF, class MASK = NoMask>
__device__ __forceinline__ f32x4 sample_logits(const ShVolumeArgs& a, const f32x4 b, const float (&d)[3], const MASK mask = MASK{}) {
    constexpr int CHUNKS = 3 * DEG;
    Cell c;
    cell_of(a.w.vol, b, c, mask);
    GridFetch<VHALF> t;
    cell_fetch<VHALF>(a.w.vol.vol, a.w.vol, c, 1, 0, t);
    f32x4 col = grid_value<VHALF>(t);
    col[3] = removed(a.w, col[3], b[3]);
    if constexpr (DEG >= 1) {
        pin(col);
        float Y[(DEG + 1) * (DEG + 1) - 1];
        sh_basis<DEG>(d, Y);
#pragma unroll
        for (int j = 0; j < CHUNKS; ++j) {
            cell_fetch<VHALF>(a.sh, a.w.vol, c, CHUNKS, j, t);
            fold<DEG>(Y, grid_value<VHALF>(t), j, col);
        }
    }
    return col;
}

}  // namespace

}  // namespace nrn
