// nrnerf_baked_api.h -- what the two baked-render entry points (nrnerf_volume_render, nrnerf_warped_volume_render) share on the host: the checks
// of a grid and its kernel record, the one-device check, the CompositeArgs of the common argument fields, the launch.  Inline helpers, no kernel
// body; each entry point keeps the checks particular to it and the order include/nrnerf.h states.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "nrnerf_model.h"
#include "nrnerf_volume.h"

namespace nrn {

inline bool grid_ok(const int32_t (&g)[3], const float (&lo)[3], const float (&hi)[3], int32_t dtype) {
    for (int c = 0; c < 3; ++c)
        if (g[c] < 2 || !(hi[c] > lo[c])) return false;                                                      // (NaN included)
    return dtype == NRNERF_VOLUME_F32 || dtype == NRNERF_VOLUME_F16;
}

inline bool grid_too_large(const int32_t (&g)[3]) {
    return (double)g[0] * (double)g[1] * (double)g[2] > (double)(1ll << 30);      // (in double: three factors below 2^31 overflow 64 bits)
}

// a vertex is 8 (half) or 16 (float32) bytes, loaded whole
inline bool grid_aligned(const void* base, int32_t dtype) { return !((uintptr_t)base & (dtype == NRNERF_VOLUME_F16 ? 7 : 15)); }

inline GridArgs grid_of(const void* base, int32_t dtype, const int32_t (&g)[3], const float (&lo)[3], const float (&hi)[3]) {
    GridArgs k{};
    k.vol = base; k.half = dtype == NRNERF_VOLUME_F16;
    for (int c = 0; c < 3; ++c) {
        k.g[c] = g[c]; k.lo[c] = lo[c];
        k.top[c] = (float)(g[c] - 1);
        volatile float extent = hi[c] - lo[c];          // (each operation rounded to fp32, whatever the host compiler would like to keep wider)
        volatile float scale = k.top[c] / extent;
        k.scale[c] = scale;
    }
    return k;
}

// every pointer that is given is device memory of `dev`
inline bool all_on_device(std::initializer_list<const void*> ptrs, int dev) {
    for (const void* p : ptrs) {
        int d = 0;
        if (p && (device_of(p, d) != NRNERF_OK || d != dev)) return false;
    }
    return true;
}

// the fields nrnerf_volume_render_args and nrnerf_warped_volume_render_args have in common, as composite_ray reads them; the per-ray maps and
// the per-sample details only when the call composites (`maps`)
template <class ARGS>
CompositeArgs composite_args_of(const ARGS& a, bool maps) {
    CompositeArgs c{};
    c.rays = a.rays; c.ray_stride = a.ray_stride; c.z = a.z; c.lindisp = a.lindisp; c.white_bkgd = a.white_bkgd;
    c.n_rays = a.n_rays; c.S = a.n_samples;
    if (maps) { c.rgb = a.rgb; c.disp = a.disp; c.acc = a.acc; c.vis = a.weights; c.alpha = a.alpha; }
    return c;
}

// launch(k, number of CUs of `dev`, stream) with `dev` current
template <class KARGS, class LAUNCH>
int launch_on(int dev, const KARGS& k, LAUNCH launch, void* hip_stream) {
    return on_device(dev, [&]() -> int {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return NRNERF_ERR_HIP;
        return status_of(launch(k, cus, (hipStream_t)hip_stream));
    });
}

}  // namespace nrn
