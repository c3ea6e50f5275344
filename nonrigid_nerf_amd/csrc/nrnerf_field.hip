// nrnerf_field.hip -- the small kernels of the field query (nrnerf_query: the reference's network_query_fn, train.py:57-105) and of the
// grid sampler on top of it: the caller's points into the layouts the network kernels read, the detail tensors out of bent4, the points of
// a regular grid, and raw -> density + 8-bit colour.  Bandwidth-trivial: one thread per sample, every index checked against its count.
#include "nrnerf_field.h"

namespace nrn {
namespace {

constexpr int FIELD_BLOCK = 256;
inline unsigned blocks_for(long long n) { return (unsigned)((n + FIELD_BLOCK - 1) / FIELD_BLOCK); }

__global__ void __launch_bounds__(FIELD_BLOCK) query_pack_kernel(const QueryPackArgs a) {
    const long long i = (long long)blockIdx.x * FIELD_BLOCK + threadIdx.x;
    const long long n = a.n_rows * a.S;
    if (i >= n) return;
    const long long row = i / a.S;
    const float* p = a.points + (size_t)i * a.stride;
    const float x = p[0], y = p[1], z = p[2];
    if (a.pts4) *(float4*)(a.pts4 + (size_t)i * 4) = make_float4(x, y, z, 0.0f);
    if (a.init_pts) { a.init_pts[i * 3] = x; a.init_pts[i * 3 + 1] = y; a.init_pts[i * 3 + 2] = z; }
    if (a.in_pts) { a.in_pts[i * 3] = x; a.in_pts[i * 3 + 1] = y; a.in_pts[i * 3 + 2] = z; }
    if (a.point_records) {
        const float* v = a.viewdirs ? a.viewdirs + (size_t)row * 3 : nullptr;
        float* r = a.point_records + (size_t)i * 11;
        r[0] = x; r[1] = y; r[2] = z;
        for (int c = 3; c < 8; ++c) r[c] = 0.0f;
        for (int c = 0; c < 3; ++c) r[8 + c] = v ? v[c] : 0.0f;
    }
    if (a.latents_out) {
        const float* l = a.latents + (size_t)row * a.lat_stride;
        for (int c = 0; c < a.lat; ++c) a.latents_out[(size_t)i * a.lat + c] = l[c];
    }
    if (a.records && i < a.n_rows) {          // (n_rows <= n: thread i < n_rows writes row i's record)
        const float* v = a.viewdirs ? a.viewdirs + (size_t)i * 3 : nullptr;
        float* r = a.records + (size_t)i * 11;
        for (int c = 0; c < 8; ++c) r[c] = 0.0f;
        for (int c = 0; c < 3; ++c) r[8 + c] = v ? v[c] : 0.0f;
    }
}

__global__ void __launch_bounds__(FIELD_BLOCK) query_unpack_kernel(const QueryUnpackArgs a) {
    const long long i = (long long)blockIdx.x * FIELD_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const float4 q = *(const float4*)(a.bent4 + (size_t)i * 4);
    if (a.in_pts) { a.in_pts[i * 3] = q.x; a.in_pts[i * 3 + 1] = q.y; a.in_pts[i * 3 + 2] = q.z; }
    if (a.rigidity) a.rigidity[i] = q.w;
    if (a.raw && a.has_removal && q.w >= a.removal) {
        float* s = a.raw + (size_t)i * a.raw_ch + 3;
        *s = *s * 0.0f;                                                      // rnh:308-311 (a product, as the network kernels': NaN stays NaN)
    }
}

__global__ void __launch_bounds__(FIELD_BLOCK) grid_points_kernel(const GridArgs a) {
    const long long i = (long long)blockIdx.x * FIELD_BLOCK + threadIdx.x;
    const long long n = (long long)a.n_rows * a.g[0];
    if (i >= n) return;
    const long long row = a.first_row + i / a.g[0];
    const int idx[3] = {(int)(i % a.g[0]), (int)(row % a.g[1]), (int)(row / a.g[1])};
    float p[3];
    for (int c = 0; c < 3; ++c) {
        // min + i * (max - min) / (G - 1) in double, rounded once: within half an ulp of the exact vertex
        const double step = a.g[c] > 1 ? ((double)a.hi[c] - (double)a.lo[c]) / (double)(a.g[c] - 1) : 0.0;
        p[c] = (float)((double)a.lo[c] + (double)idx[c] * step);
    }
    *(float4*)(a.pts4 + (size_t)i * 4) = make_float4(p[0], p[1], p[2], 0.0f);
}

__global__ void __launch_bounds__(FIELD_BLOCK) field_from_raw_kernel(const float* raw, int raw_ch, long long n, float* sigma, uint8_t* rgb8) {
    const long long i = (long long)blockIdx.x * FIELD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float* r = raw + (size_t)i * raw_ch;
    if (sigma) sigma[i] = fmaxf(r[3], 0.0f);                                 // train.py:740-741 (F.relu)
    if (rgb8) {
        for (int c = 0; c < 3; ++c) {
            const float s = 1.0f / (1.0f + expf(-r[c]));                     // torch.sigmoid
            const float v = 255.0f * fminf(fmaxf(s, 0.0f), 1.0f);            // to8b: (255 * clip(x, 0, 1)).astype(uint8), truncating
            rgb8[i * 3 + c] = (uint8_t)v;
        }
    }
}

}  // namespace

hipError_t launch_query_pack(const QueryPackArgs& a, hipStream_t stream) {
    const long long n = a.n_rows * a.S;
    if (n <= 0) return hipSuccess;
    if (!a.points || a.stride < 3 || n >= (1ll << 31) * FIELD_BLOCK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(query_pack_kernel, dim3(blocks_for(n)), dim3(FIELD_BLOCK), 0, stream, a);
    return hipGetLastError();
}
hipError_t launch_query_unpack(const QueryUnpackArgs& a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    if (!a.bent4 || a.n >= (1ll << 31) * FIELD_BLOCK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(query_unpack_kernel, dim3(blocks_for(a.n)), dim3(FIELD_BLOCK), 0, stream, a);
    return hipGetLastError();
}
hipError_t launch_grid_points(const GridArgs& a, hipStream_t stream) {
    const long long n = (long long)a.n_rows * a.g[0];
    if (n <= 0) return hipSuccess;
    if (!a.pts4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grid_points_kernel, dim3(blocks_for(n)), dim3(FIELD_BLOCK), 0, stream, a);
    return hipGetLastError();
}
hipError_t launch_field_from_raw(const float* raw, int raw_ch, long long n, float* sigma, uint8_t* rgb8, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!raw || raw_ch < 4 || n >= (1ll << 31) * FIELD_BLOCK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(field_from_raw_kernel, dim3(blocks_for(n)), dim3(FIELD_BLOCK), 0, stream, raw, raw_ch, n, sigma, rgb8);
    return hipGetLastError();
}

}  // namespace nrn
