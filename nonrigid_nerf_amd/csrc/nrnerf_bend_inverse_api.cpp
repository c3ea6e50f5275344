// nrnerf_bend_inverse_api.cpp -- the inverse-bender entry points of the C ABI (include/nrnerf.h, "ABI 10 (additions)"): validate, zero the
// work counter on the stream, run the launcher of nrnerf_bend_inverse_args.h on the model's device.  The checks come in the order the header
// states them, the ones that need no HIP call first; no entry point keeps state.  Its own unit, so that the objects of the existing entry
// points are built from unchanged sources.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_model.h"
#include "nrnerf_bend_inverse_args.h"

using namespace nrn;

namespace {

constexpr size_t INVERSE_COUNTER_BYTES = 256;      // one work counter, a 256-byte slot of its own

// a compiled bender shape with its point-source image in an fp32 handle (the rule of nrnerf_query's bender step)
bool inverse_supported(const nrnerf_model& m) {
    if (m.precision != NRNERF_PREC_F32) return false;
    if (!(m.generic ? m.gen_compiled_bender >= 0 : m.split_ok != 0) || !m.bend_only.stream) return false;
    const int arch = bender_arch_of(&m);
    return arch == 0 || arch == 1;
}

}  // namespace

extern "C" {

size_t nrnerf_bender_inverse_workspace_bytes(const nrnerf_model* m) {
    return (m && m->has_bend && inverse_supported(*m)) ? INVERSE_COUNTER_BYTES : 0;
}

int nrnerf_bender_inverse(const nrnerf_model* m, const nrnerf_bender_inverse_args* a, void* hip_stream) try {
    if (!m || !a || a->struct_size != sizeof(nrnerf_bender_inverse_args)) return NRNERF_ERR_INVALID;
    if (a->n_rows < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->point_stride < 3 || a->latent_stride < 0) return NRNERF_ERR_INVALID;
    if (!(a->tolerance >= 0.0f)) return NRNERF_ERR_INVALID;                                   // (NaN included)
    if (!(a->relaxation > 0.0f && a->relaxation <= 1.0f)) return NRNERF_ERR_INVALID;
    if (a->max_iters < 1 || a->max_iters > 1024) return NRNERF_ERR_INVALID;
    if (a->flags & ~(uint32_t)NRNERF_RENDER_FIXED_SHARES) return NRNERF_ERR_INVALID;
    if (a->n_rows == 0) return NRNERF_OK;
    if (!a->canonical || !a->latents || !a->observed) return NRNERF_ERR_INVALID;
    // (the first read of the handle.  tests/test_unbend_host.py -- as tests/test_query_host.py does for nrnerf_query -- passes zeroed host
    //  memory as a model here: it relies on ModelTraits being the handle's first base and on 0 meaning "no bender")
    if (!m->has_bend) return NRNERF_ERR_INVALID;                                              // nothing to invert
    if (!inverse_supported(*m)) return NRNERF_ERR_UNSUPPORTED;
    if ((long long)a->n_rows * ((a->n_samples + 31) / 32) >= (1ll << 31)) return NRNERF_ERR_UNSUPPORTED;
    if (!a->workspace || a->workspace_bytes < INVERSE_COUNTER_BYTES || ((uintptr_t)a->workspace & 255)) return NRNERF_ERR_WORKSPACE;
    // device memory, all of it on the model's device
    const void* ptrs[] = {a->canonical, a->initial, a->latents, a->observed, a->residual, a->iterations, a->workspace};
    for (const void* p : ptrs) {
        int dev = 0;
        if (p && (device_of(p, dev) != NRNERF_OK || dev != m->device)) return NRNERF_ERR_INVALID;
    }
    BendInverseArgs k{};
    k.canonical = a->canonical; k.stride = a->point_stride; k.initial = a->initial;
    k.latents = a->latents; k.lat_stride = a->latent_stride;
    k.n_rows = a->n_rows; k.n_per_row = a->n_samples;
    k.wstream = m->bend_only.stream; k.bias = m->bend_only.bias;
    k.knobs.has_cutoff = a->has_rigidity_cutoff; k.knobs.cutoff = a->rigidity_cutoff;
    k.knobs.has_scaling = a->has_test_time_scaling; k.knobs.scaling = a->test_time_scaling;
    k.tol = a->tolerance; k.omega = a->relaxation; k.max_iters = a->max_iters;
    k.observed = a->observed; k.residual = a->residual; k.iterations = a->iterations;
    const bool dynamic = !(a->flags & NRNERF_RENDER_FIXED_SHARES);
    k.work_counter = dynamic ? (unsigned*)a->workspace : nullptr;
    hipStream_t stream = (hipStream_t)hip_stream;
    return on_model_device(m, [&]() -> int {
        if (dynamic && hipMemsetAsync(a->workspace, 0, INVERSE_COUNTER_BYTES, stream) != hipSuccess) return NRNERF_ERR_HIP;
        return status_of(launch_bend_inverse(bender_arch_of(m), k, m->num_cus, stream));
    });
} NRN_CATCH

}  // extern "C"
