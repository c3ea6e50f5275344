// nrnerf_isosurface_api.cpp -- the iso-surface entry points of the C ABI (include/nrnerf.h, "ABI 10 (additions)"): validate, carve the
// workspace, run the launchers of nrnerf_isosurface.h on the device that owns the volume.  Every check comes before the first HIP call; no
// entry point keeps state.  Its own unit, so that the objects of the existing entry points are built from unchanged sources.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrnerf_model.h"
#include "nrnerf_isosurface.h"

using namespace nrn;

namespace {

// more grid vertices than the kernels index (a grid without cells is never too large: nothing runs)
bool iso_too_large(int32_t gx, int32_t gy, int32_t gz) {
    if (gx < 2 || gy < 2 || gz < 2) return false;
    const long long xy = (long long)gx * gy;                        // < 2^62
    return xy > ISO_MAX_VERTICES || xy * gz > ISO_MAX_VERTICES;     // (xy <= 2^30 where the product is formed: no overflow)
}
// grid vertices of a grid WITH cells (call after iso_too_large); 0: no cells
long long iso_vertices(int32_t gx, int32_t gy, int32_t gz) { return (gx < 2 || gy < 2 || gz < 2) ? 0 : (long long)gx * gy * gz; }

// the checks both calls share, in the order the header states them; on NRNERF_OK with `cells`, `k` is ready to launch
int iso_prepare(const nrnerf_isosurface_args* a, bool emit, IsoArgs& k, bool& cells) {
    if (!a || a->struct_size != sizeof(nrnerf_isosurface_args)) return NRNERF_ERR_INVALID;
    if (a->gx < 1 || a->gy < 1 || a->gz < 1 || !a->value) return NRNERF_ERR_INVALID;
    if (!emit && !a->totals) return NRNERF_ERR_INVALID;
    if (emit) {
        if (a->n_vertices < 0 || a->n_triangles < 0) return NRNERF_ERR_INVALID;
        if ((a->n_vertices > 0 && !a->vertices) || (a->n_triangles > 0 && !a->faces)) return NRNERF_ERR_INVALID;
        if (a->n_vertices >= (1ll << 31) || a->n_triangles >= (1ll << 31)) return NRNERF_ERR_UNSUPPORTED;
    }
    if (iso_too_large(a->gx, a->gy, a->gz)) return NRNERF_ERR_UNSUPPORTED;
    const long long n = iso_vertices(a->gx, a->gy, a->gz);
    cells = n > 0;
    if (!cells) return NRNERF_OK;
    if (!a->workspace) return NRNERF_ERR_INVALID;
    k = IsoArgs{};
    k.ws = iso_carve(a->workspace, n);
    if (a->workspace_bytes < k.ws.bytes || ((uintptr_t)a->workspace & 255u)) return NRNERF_ERR_WORKSPACE;
    k.value = a->value;
    k.g[0] = a->gx; k.g[1] = a->gy; k.g[2] = a->gz;
    for (int c = 0; c < 3; ++c) { k.lo[c] = a->min_point[c]; k.hi[c] = a->max_point[c]; }
    k.level = a->level;
    k.totals = (long long*)a->totals;
    k.vertices = a->vertices; k.normals = a->normals; k.faces = a->faces;
    k.n_vertices = a->n_vertices; k.n_triangles = a->n_triangles;
    return NRNERF_OK;
}

}  // namespace

extern "C" {

size_t nrnerf_isosurface_workspace_bytes(int32_t gx, int32_t gy, int32_t gz) try {
    if (iso_too_large(gx, gy, gz)) return 0;
    const long long n = iso_vertices(gx, gy, gz);
    return n > 0 ? iso_carve(nullptr, n).bytes : 0;
} catch (...) { return 0; }

int nrnerf_isosurface_count(const nrnerf_isosurface_args* a, void* hip_stream) try {
    IsoArgs k{};
    bool cells = false;
    const int rc = iso_prepare(a, false, k, cells);
    if (rc != NRNERF_OK) return rc;
    return on_owner_of(a->totals, [&] {
        if (!cells) return status_of(hipMemsetAsync(a->totals, 0, 2 * sizeof(int64_t), (hipStream_t)hip_stream));
        return status_of(launch_isosurface_count(k, (hipStream_t)hip_stream));
    });
} NRN_CATCH

int nrnerf_isosurface_emit(const nrnerf_isosurface_args* a, void* hip_stream) try {
    IsoArgs k{};
    bool cells = false;
    const int rc = iso_prepare(a, true, k, cells);
    if (rc != NRNERF_OK || !cells) return rc;
    return on_owner_of(a->value, [&] { return status_of(launch_isosurface_emit(k, (hipStream_t)hip_stream)); });
} NRN_CATCH

}  // extern "C"
