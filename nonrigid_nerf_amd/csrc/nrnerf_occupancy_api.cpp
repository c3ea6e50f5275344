// nrnerf_occupancy_api.cpp -- nrnerf_occupancy_words / nrnerf_occupancy_build of the C ABI (include/nrnerf.h, "ABI 10 (additions): occupancy
// masks"): model-free -- validate, run the launcher of nrnerf_occupancy.h on the device that owns the words.  The checks come in the order the
// header states them, the ones that need no HIP call first; the entry points keep no state.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_baked_api.h"
#include "nrnerf_occupancy.h"

using namespace nrn;

extern "C" {

int64_t nrnerf_occupancy_words(const int32_t* g, int32_t log2_block) {
    if (!g || g[0] < 2 || g[1] < 2 || g[2] < 2 || log2_block < OCC_MIN_LOG2_BLOCK || log2_block > OCC_MAX_LOG2_BLOCK) return 0;
    const int gg[3] = {g[0], g[1], g[2]};
    return occupancy_words(gg, log2_block);
}

int nrnerf_occupancy_build(const nrnerf_occupancy_build_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_occupancy_build_args)) return NRNERF_ERR_INVALID;
    if (a->g[0] < 2 || a->g[1] < 2 || a->g[2] < 2) return NRNERF_ERR_INVALID;
    if (a->volume_dtype != NRNERF_VOLUME_F32 && a->volume_dtype != NRNERF_VOLUME_F16) return NRNERF_ERR_INVALID;
    if (a->log2_block < OCC_MIN_LOG2_BLOCK || a->log2_block > OCC_MAX_LOG2_BLOCK) return NRNERF_ERR_INVALID;
    if (!(a->threshold >= 0.0f)) return NRNERF_ERR_INVALID;                       // (NaN included)
    if (grid_too_large(a->g)) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_words != nrnerf_occupancy_words(a->g, a->log2_block)) return NRNERF_ERR_INVALID;
    if (!a->volume || !a->words) return NRNERF_ERR_INVALID;
    int dev = 0;
    if (device_of(a->words, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    if (!all_on_device({a->volume}, dev)) return NRNERF_ERR_INVALID;
    if (!grid_aligned(a->volume, a->volume_dtype) || ((uintptr_t)a->words & 3)) return NRNERF_ERR_INVALID;
    OccupancyArgs k{};
    k.vol = a->volume; k.half = a->volume_dtype == NRNERF_VOLUME_F16;
    for (int c = 0; c < 3; ++c) k.g[c] = a->g[c];
    k.k = a->log2_block; k.threshold = a->threshold;
    k.words = (unsigned*)a->words; k.n_words = (int)a->n_words;
    return on_device(dev, [&]() -> int { return status_of(launch_occupancy_build(k, (hipStream_t)hip_stream)); });
} NRN_CATCH

}  // extern "C"
