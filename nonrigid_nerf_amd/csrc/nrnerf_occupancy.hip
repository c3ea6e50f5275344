// nrnerf_occupancy.hip -- the occupancy mask of a baked volume: one bit per block of 2^k cells per axis, set iff some vertex of the block (the
// corners of all its cells: the block's vertices and the first ones of its upper neighbours) has a sigma logit that is not <= threshold, or a
// channel that is not finite.  The rule is stated in include/nrnerf.h ("occupancy masks") and, in numpy, in tests/occupancy_reference.py;
// layout and measurements: DESIGN.md section 3.17.
//
// occupancy_build_kernel<HALF>: ONE WAVE PER OUTPUT WORD.  The wave walks the word's 32 blocks in turn; the lanes stride over a block's
// (2^k + 1)^3 vertices (fewer at the grid's top faces), x fastest, each loading one vertex whole (16 / 8 bytes); a ballot reduces the lanes'
// flags to the block's bit, lane 0 writes the word.  One writer per word, no atomics, no workspace: the same bits on every run, and the unused
// high bits of the last word are zero.  A vertex on a block face is read once per block that shares it -- at most 8 times, (1 + 2^-k)^3 times
// on average (1.42 at the default block of 8 cells): a streaming read of the volume.
#include <hip/hip_runtime.h>

#include "nrnerf_occupancy.h"
#include "nrnerf_composite_ray.h"
#include "nrnerf_volume_lookup.h"

namespace nrn {

namespace {

constexpr int OCC_WAVES = 4;            // waves (= words) per workgroup

__device__ __forceinline__ bool finite_f(const float x) { return fabsf(x) < __builtin_huge_valf(); }          // (NaN: false)

template <bool HALF>
__global__ void __launch_bounds__(OCC_WAVES * 64) occupancy_build_kernel(const OccupancyArgs a) {
    typedef typename GridFetch<HALF>::vertex vertex;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long word = (long long)blockIdx.x * OCC_WAVES + wave;
    if (word >= a.n_words) return;
    const int B = 1 << a.k;
    const int nbx = occupancy_blocks(a.g[0], a.k), nby = occupancy_blocks(a.g[1], a.k), nbz = occupancy_blocks(a.g[2], a.k);
    const long long total = (long long)nbx * nby * nbz;
    const size_t gx = (size_t)a.g[0], gxy = gx * (size_t)a.g[1];
    const __attribute__((address_space(1))) vertex* q = (const __attribute__((address_space(1))) vertex*)a.vol;
    unsigned bits = 0;
    for (int t = 0; t < 32; ++t) {
        const long long blk = word * 32 + t;
        if (blk >= total) break;                    // (the same for every lane)
        const int bx = (int)(blk % nbx), by = (int)((blk / nbx) % nby), bz = (int)(blk / ((long long)nbx * nby));
        // vertices b * B .. min(b * B + B, g - 1) inclusive: every index is inside the grid
        const int x0 = bx * B, y0 = by * B, z0 = bz * B;
        const int nx = (x0 + B < a.g[0] - 1 ? x0 + B : a.g[0] - 1) - x0 + 1;
        const int ny = (y0 + B < a.g[1] - 1 ? y0 + B : a.g[1] - 1) - y0 + 1;
        const int nz = (z0 + B < a.g[2] - 1 ? z0 + B : a.g[2] - 1) - z0 + 1;
        const int n = nx * ny * nz;
        bool occupied = false;
        for (int e = lane; e < n; e += 64) {
            const int x = x0 + e % nx, y = y0 + (e / nx) % ny, z = z0 + e / (nx * ny);
            const vertex c = q[(size_t)z * gxy + (size_t)y * gx + (size_t)x];
            f32x4 r;
            if constexpr (HALF) r = __builtin_convertvector(c, f32x4);
            else r = c;
            const bool empty = r[3] <= a.threshold && finite_f(r[0]) && finite_f(r[1]) && finite_f(r[2]) && finite_f(r[3]);
            occupied = occupied || !empty;
        }
        if (__ballot(occupied) != 0ull) bits |= 1u << t;
    }
    if (lane == 0) ((__attribute__((address_space(1))) unsigned*)a.words)[word] = bits;
}

}  // namespace

hipError_t launch_occupancy_build(const OccupancyArgs& a, hipStream_t stream) {
    if (a.k < OCC_MIN_LOG2_BLOCK || a.k > OCC_MAX_LOG2_BLOCK) return hipErrorInvalidValue;
    if (a.g[0] < 2 || a.g[1] < 2 || a.g[2] < 2 || (long long)a.n_words != occupancy_words(a.g, a.k)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n_words + OCC_WAVES - 1) / OCC_WAVES)), block(OCC_WAVES * 64);
    if (a.half) hipLaunchKernelGGL(occupancy_build_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(occupancy_build_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace nrn
