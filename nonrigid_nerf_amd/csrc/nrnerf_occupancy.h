// nrnerf_occupancy.h -- occupancy masks of a baked volume (include/nrnerf.h, "occupancy masks"): the mask's geometry, stated once for the host
// and the device, and the launch interface of the kernel that builds one (nrnerf_occupancy.hip; what nrnerf_occupancy_build runs).
// No kernel body: the entry points' units include this alone.
#pragma once
#include "nrnerf_kernels.h"
#include "nrnerf_volume.h"

namespace nrn {

constexpr int OCC_MIN_LOG2_BLOCK = 1, OCC_MAX_LOG2_BLOCK = 4;      // blocks of 2 .. 16 cells per axis

// blocks per axis of g vertices (g - 1 cells) at 2^k cells per block
__host__ __device__ inline int occupancy_blocks(int g, int k) { return (g - 1 + (1 << k) - 1) >> k; }
// 32-bit words of the mask of a (gx, gy, gz) grid: one bit per block, bit (bz * nb_y + by) * nb_x + bx
inline long long occupancy_words(const int (&g)[3], int k) {
    const long long n = (long long)occupancy_blocks(g[0], k) * occupancy_blocks(g[1], k) * occupancy_blocks(g[2], k);
    return (n + 31) / 32;
}

struct OccupancyArgs {
    const void* vol;         // [gz,gy,gx,4] logits
    int half;                // 0: float32, 1: IEEE half
    int g[3];                // gx, gy, gz, each >= 2
    int k;                   // log2 of the block's cells per axis, 1 .. 4
    float threshold;         // a vertex is empty iff its four channels are finite and its sigma logit <= threshold
    unsigned* words;         // out [n_words]
    int n_words;
};
// hipErrorInvalidValue for k outside 1 .. 4 or a word count that is not the grid's (nothing is launched)
hipError_t launch_occupancy_build(const OccupancyArgs& a, hipStream_t stream);

}  // namespace nrn
