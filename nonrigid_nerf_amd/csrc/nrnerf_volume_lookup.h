// nrnerf_volume_lookup.h -- the value of a vertex-centred grid of four channels at a point (include/nrnerf.h, "THE VALUE AT A POINT"): device
// functions shared by nrnerf_volume.hip (the canonical volume at ready-made points) and nrnerf_warp.hip (an offset grid, then the canonical
// volume at the bent point).  A grid is a GridArgs (nrnerf_volume.h); where a point falls in it is grid_cell, used by both forms of the lookup.
// The occupancy mask of a baked render is a policy of the two-step form (NoMask / BlockMask): there is one grid_fetch.
// Every multiply-add is spelled __fmaf_rn and every product that feeds a sum or a difference goes through rounded(): this build's
// -ffp-contract=fast would otherwise fuse them per instantiation (nrnerf_composite_ray.h), and every kernel that includes this must give the
// same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "nrnerf_composite_ray.h"
#include "nrnerf_volume.h"

namespace nrn {

namespace {

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

// lerp with exact ends: f = 0 returns a, f = 1 returns b
__device__ __forceinline__ f32x4 lerp4(const f32x4 a, const f32x4 b, const float f) {
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = __fmaf_rn(f, b[c], __fmaf_rn(-f, a[c], a[c]));
    return r;
}

// vertices v and v + 1 (x-neighbours: 32 / 16 contiguous bytes), widened to fp32
template <bool HALF>
__device__ __forceinline__ void load_pair(const void* vol, const size_t v, f32x4& a, f32x4& b) {
    if constexpr (HALF) {
        const __attribute__((address_space(1))) h16x4* p = (const __attribute__((address_space(1))) h16x4*)vol + v;
        const h16x4 ha = p[0], hb = p[1];
        a = __builtin_convertvector(ha, f32x4);
        b = __builtin_convertvector(hb, f32x4);
    } else {
        const __attribute__((address_space(1))) f32x4* p = (const __attribute__((address_space(1))) f32x4*)vol + v;
        a = p[0];
        b = p[1];
    }
}

// where (px, py, pz) falls in the grid: the cell's lowest corner i and the fractions f in it; ok = false: outside the grid (or NaN), an empty
// sample.  (ok is an output parameter, not the return value: returned, hipcc allocates up to 4 more VGPRs in warped_render_kernel)
__device__ __forceinline__ void grid_cell(const GridArgs& a, const float px, const float py, const float pz, int (&i)[3], float (&f)[3], bool& ok) {
    const float p[3] = {px, py, pz};
    ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g = rounded(__fsub_rn(p[c], a.lo[c]) * a.scale[c]);
        const bool in = g >= 0.0f && g <= a.top[c];          // (NaN: false)
        ok = ok && in;
        const float gs = in ? g : 0.0f;
        int ic = (int)floorf(gs);
        ic = ic < a.g[c] - 2 ? ic : a.g[c] - 2;              // 0 <= ic <= g - 2: every corner index is inside the grid
        i[c] = ic;
        f[c] = __fsub_rn(gs, (float)ic);
    }
}

// the grid's value at (px, py, pz): include/nrnerf.h, "THE VALUE AT A POINT"
template <bool HALF>
__device__ __forceinline__ f32x4 volume_at(const GridArgs& a, const float px, const float py, const float pz) {
    int i[3];
    float f[3];
    bool ok;
    grid_cell(a, px, py, pz, i, f, ok);
    f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) {
        const size_t gx = (size_t)a.g[0], gxy = gx * (size_t)a.g[1];
        const size_t v = (size_t)i[2] * gxy + (size_t)i[1] * gx + (size_t)i[0];
        f32x4 c000, c100, c010, c110, c001, c101, c011, c111;
        load_pair<HALF>(a.vol, v, c000, c100);
        load_pair<HALF>(a.vol, v + gx, c010, c110);
        load_pair<HALF>(a.vol, v + gxy, c001, c101);
        load_pair<HALF>(a.vol, v + gxy + gx, c011, c111);
        const f32x4 x00 = lerp4(c000, c100, f[0]), x10 = lerp4(c010, c110, f[0]);
        const f32x4 x01 = lerp4(c001, c101, f[0]), x11 = lerp4(c011, c111, f[0]);
        r = lerp4(lerp4(x00, x10, f[1]), lerp4(x01, x11, f[1]), f[2]);
    }
    return r;
}

// ---- volume_at in two steps, for a kernel that wants the loads of several samples in flight before it interpolates the first one: the same
// operations in the same order, hence the same bits
template <bool HALF>
struct GridFetch {
    typedef typename std::conditional<HALF, h16x4, f32x4>::type vertex;
    vertex c[8];             // the corners as stored: (x, y, z) offsets 000 100 010 110 001 101 011 111
    float f[3];
    bool ok;                 // false: the sample is empty, nothing was loaded
};

// ---- the occupancy mask as a policy of the lookup: NoMask compiles away; BlockMask ANDs the bit of the cell's block into the sample's "not
// empty" flag before any corner is requested (include/nrnerf.h, "occupancy masks")
struct NoMask {
    static constexpr bool on = false;
};
struct BlockMask {
    static constexpr bool on = true;
    const unsigned* occ;     // bit (bz * nb[1] + by) * nb[0] + bx, word index >> 5, bit index & 31
    int k;                   // log2 of the block's cells per axis
    int nb[2];               // blocks along x, y
    // the bit of the block of cell i: the block is i >> k per axis (grid_cell clamps i to 0 .. g - 2, so the block exists whether the sample is
    // inside the box or not)
    __device__ __forceinline__ bool bit(const int (&i)[3]) const {
        const int blk = ((i[2] >> k) * nb[1] + (i[1] >> k)) * nb[0] + (i[0] >> k);
        const unsigned word = ((const __attribute__((address_space(1))) unsigned*)occ)[blk >> 5];
        return ((word >> (blk & 31)) & 1u) != 0u;
    }
};

// where the point falls, and the requests for its eight corners (none for an empty sample, which a sample in an empty block of `mask` is)
template <bool HALF, class MASK = NoMask>
__device__ __forceinline__ void grid_fetch(const GridArgs& a, const float px, const float py, const float pz, GridFetch<HALF>& t,
                                           const MASK mask = MASK{}) {
    typedef typename GridFetch<HALF>::vertex vertex;
    int i[3];
    grid_cell(a, px, py, pz, i, t.f, t.ok);
    if constexpr (MASK::on) t.ok = t.ok && mask.bit(i);
#pragma unroll
    for (int k = 0; k < 8; ++k) t.c[k] = vertex{};
    if (t.ok) {
        const size_t gx = (size_t)a.g[0], gxy = gx * (size_t)a.g[1];
        const size_t v = (size_t)i[2] * gxy + (size_t)i[1] * gx + (size_t)i[0];
        const __attribute__((address_space(1))) vertex* q = (const __attribute__((address_space(1))) vertex*)a.vol;
        t.c[0] = q[v];             t.c[1] = q[v + 1];
        t.c[2] = q[v + gx];        t.c[3] = q[v + gx + 1];
        t.c[4] = q[v + gxy];       t.c[5] = q[v + gxy + 1];
        t.c[6] = q[v + gxy + gx];  t.c[7] = q[v + gxy + gx + 1];
    }
}

// the interpolation of what grid_fetch asked for; zeros for an empty sample
template <bool HALF>
__device__ __forceinline__ f32x4 grid_value(const GridFetch<HALF>& t) {
    f32x4 c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if constexpr (HALF) c[k] = __builtin_convertvector(t.c[k], f32x4);
        else c[k] = t.c[k];
    }
    const f32x4 x00 = lerp4(c[0], c[1], t.f[0]), x10 = lerp4(c[2], c[3], t.f[0]);
    const f32x4 x01 = lerp4(c[4], c[5], t.f[0]), x11 = lerp4(c[6], c[7], t.f[0]);
    const f32x4 r = lerp4(lerp4(x00, x10, t.f[1]), lerp4(x01, x11, t.f[1]), t.f[2]);
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    return t.ok ? r : zero;
}

}  // namespace

}  // namespace nrn
