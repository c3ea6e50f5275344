// nrnerf_volume_api.cpp -- the baked-volume entry points of the C ABI (include/nrnerf.h, "ABI 10 (additions): baked volumes"):
// nrnerf_volume_render (model-free: validate, run the launcher of nrnerf_volume.h on the device that owns the outputs) and nrnerf_bend_points
// (the bender step of nrnerf_query by itself, on the launchers of nrnerf_bend_points.h).  The checks come in the order the header states them,
// the ones that need no HIP call first; no entry point keeps state.  What nrnerf_volume_render shares with nrnerf_warped_volume_render is in
// nrnerf_baked_api.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_baked_api.h"
#include "nrnerf_bend_points.h"

using namespace nrn;

namespace {

// the work counters of the 16x16x32 point-source bender: one per pair of co-resident workgroups, 64 bytes apart (nrnerf_bend_x16.h) -- the
// numbers nrnerf_query's workspace uses for the same launch
constexpr int BEND_POINTS_COUNTERS = 512;
constexpr size_t BEND_POINTS_COUNTER_BYTES = (size_t)BEND_POINTS_COUNTERS * 64;
constexpr unsigned BEND_POINTS_FLAGS = NRNERF_RENDER_NO_X16 | NRNERF_RENDER_BENDER_32X32 | NRNERF_RENDER_FIXED_SHARES;

// the point-source stand-alone bender: a compiled shape with its image in the handle (the rule of nrnerf_query's bender step)
bool bend_points_supported(const nrnerf_model& m) {
    if (!(m.generic ? m.gen_compiled_bender >= 0 : m.split_ok != 0) || !m.bend_only.stream) return false;
    const int arch = bender_arch_of(&m);
    return arch == 0 || arch == 1;
}

}  // namespace

extern "C" {

int nrnerf_volume_render(const nrnerf_volume_render_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_volume_render_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->ray_stride < 8) return NRNERF_ERR_INVALID;
    if (!grid_ok(a->g, a->min_point, a->max_point, a->volume_dtype)) return NRNERF_ERR_INVALID;
    if (grid_too_large(a->g)) return NRNERF_ERR_UNSUPPORTED;
    if ((long long)a->n_rays * a->n_samples >= (1ll << 31)) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || !a->volume) return NRNERF_ERR_INVALID;
    const bool maps = a->rgb && a->disp && a->acc;
    if (!maps && (a->rgb || a->disp || a->acc)) return NRNERF_ERR_INVALID;
    if (!maps && !a->raw) return NRNERF_ERR_INVALID;
    const bool surface = a->surface_pts || a->surface_rigidity || a->median_index;
    if (!maps && (a->weights || a->alpha || surface)) return NRNERF_ERR_INVALID;
    if (!a->points4 && (a->has_removal_threshold || surface)) return NRNERF_ERR_INVALID;
    // device memory, all of it on one device
    const void* const owner = maps ? (const void*)a->rgb : (const void*)a->raw;
    int dev = 0;
    if (device_of(owner, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    if (!all_on_device({a->rays, a->z, a->points4, a->volume, a->rgb, a->disp, a->acc, a->raw, a->weights, a->alpha,
                        a->surface_pts, a->surface_rigidity, a->median_index}, dev)) return NRNERF_ERR_INVALID;
    if (a->points4 && ((uintptr_t)a->points4 & 15)) return NRNERF_ERR_INVALID;
    if (a->raw && ((uintptr_t)a->raw & 15)) return NRNERF_ERR_INVALID;
    if (!grid_aligned(a->volume, a->volume_dtype)) return NRNERF_ERR_INVALID;
    VolumeArgs k{};
    k.c = composite_args_of(*a, maps);
    if (maps && surface) { k.c.bent4 = a->points4; k.c.surf_pts = a->surface_pts; k.c.surf_rig = a->surface_rigidity; k.c.med_idx = a->median_index; }
    k.points4 = a->points4;
    k.grid = grid_of(a->volume, a->volume_dtype, a->g, a->min_point, a->max_point);
    k.has_removal = a->has_removal_threshold; k.removal = a->removal_threshold;
    k.raw_out = a->raw;
    return launch_on(dev, k, launch_volume_render, hip_stream);
} NRN_CATCH

size_t nrnerf_bend_points_workspace_bytes(const nrnerf_model* m) {
    return (m && m->has_bend && bend_points_supported(*m)) ? BEND_POINTS_COUNTER_BYTES : 0;
}

int nrnerf_bend_points(const nrnerf_model* m, const nrnerf_bend_points_args* a, void* hip_stream) try {
    if (!m || !a || a->struct_size != sizeof(nrnerf_bend_points_args)) return NRNERF_ERR_INVALID;
    if (a->n_rows < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->point_stride < 3 || a->latent_stride < 0) return NRNERF_ERR_INVALID;
    if (a->flags & ~BEND_POINTS_FLAGS) return NRNERF_ERR_INVALID;
    if (a->n_rows == 0) return NRNERF_OK;
    if (!a->points || !a->latents || !a->bent4) return NRNERF_ERR_INVALID;
    // (the first read of the handle.  tests/test_volume_host.py -- as tests/test_query_host.py does for nrnerf_query -- passes zeroed host
    //  memory as a model here: it relies on ModelTraits being the handle's first base and on 0 meaning "no bender")
    if (!m->has_bend) return NRNERF_ERR_INVALID;
    if (!bend_points_supported(*m)) return NRNERF_ERR_UNSUPPORTED;
    const int N = a->n_rows, S = a->n_samples;
    if ((long long)N * S >= (1ll << 31) || (long long)N * ((S + 31) / 32) >= (1ll << 31)) return NRNERF_ERR_UNSUPPORTED;
    if (!a->workspace || a->workspace_bytes < BEND_POINTS_COUNTER_BYTES || ((uintptr_t)a->workspace & 255)) return NRNERF_ERR_WORKSPACE;
    const void* ptrs[] = {a->points, a->latents, a->bent4, a->workspace};
    for (const void* p : ptrs) {
        int dev = 0;
        if (device_of(p, dev) != NRNERF_OK || dev != m->device) return NRNERF_ERR_INVALID;
    }
    if ((uintptr_t)a->bent4 & 15) return NRNERF_ERR_INVALID;
    // kernel and shares as plan_query picks them for the query's bender step
    const bool x16 = m->bend_x16.stream && !(a->flags & (NRNERF_RENDER_BENDER_32X32 | NRNERF_RENDER_NO_X16));
    const bool dynamic = x16 && !(a->flags & NRNERF_RENDER_FIXED_SHARES) && m->num_cus <= BEND_POINTS_COUNTERS;
    const ImageDev& bi = x16 ? m->bend_x16 : m->bend_only;
    BendPointArgs b{};
    b.b.latents = a->latents; b.b.lat_stride = a->latent_stride; b.b.n_rays = N; b.b.n_per_ray = S; b.b.out_stride = S;
    b.b.wstream = bi.stream; b.b.bias = bi.bias; b.b.bent4 = a->bent4;
    b.b.knobs.has_cutoff = a->has_rigidity_cutoff; b.b.knobs.cutoff = a->rigidity_cutoff;
    b.b.knobs.has_scaling = a->has_test_time_scaling; b.b.knobs.scaling = a->test_time_scaling;
    b.b.work_counter = dynamic ? (unsigned*)a->workspace : nullptr;
    b.src.points = a->points; b.src.stride = a->point_stride;
    hipStream_t stream = (hipStream_t)hip_stream;
    return on_model_device(m, [&]() -> int {
        if (dynamic && hipMemsetAsync(a->workspace, 0, BEND_POINTS_COUNTER_BYTES, stream) != hipSuccess) return NRNERF_ERR_HIP;
        return status_of(x16 ? launch_bend_points_x16(bender_arch_of(m), b, m->num_cus, stream)
                             : launch_bend_points(m->precision, bender_arch_of(m), b, m->num_cus, stream));
    });
} NRN_CATCH

}  // extern "C"
