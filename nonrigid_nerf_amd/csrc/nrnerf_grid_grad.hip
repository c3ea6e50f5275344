// nrnerf_grid_grad.hip -- the adjoint of "THE VALUE AT A POINT" (include/nrnerf.h): from the cotangent g of a looked-up value, the gradient of the
// grid (d_grid[corner k] += w_k g) and of the point (d_p[axis] = scale[axis] * sum over channels of g_ch dv_ch / df_axis).  The rule is stated in
// include/nrnerf.h ("the adjoint of the lookup") and, in float64, in tests/grid_grad_reference.py; resources and measurements: DESIGN.md
// section 3.15.  Two kernels, each a grid-stride loop without LDS; the cell and the fractions are grid_cell's (nrnerf_volume_lookup.h), the
// function the forward kernels call, so the two directions cannot disagree on the cell.
//
// grid_scatter_kernel (d_grid): EIGHT LANES PER POINT -- lane (dx, c) adds channel c of the four corners with x offset dx, so one atomic
// instruction covers, per point, the 32 contiguous bytes of a pair of x-neighbours: float32 atomic adds to global memory without a return value
// (global_atomic_add_f32, no compare-and-swap loop).  With one lane per point and one dword per lane the same adds took 5.3 times as long
// (DESIGN.md section 3.15): the memory side works in 64-byte requests.  The order of the sums is the order of arrival, so d_grid is NOT the
// same bits on every run.  The grid itself is not read.
// grid_point_grad_kernel<HALF> (d_points): one thread per point; the eight corners are loaded as the forward loads them (four pairs of
// x-neighbours); one writer per element and a fixed operation order: the same bits on every run, with or without d_grid.  Nothing is written to
// a grid.
// Every multiply-add is spelled __fmaf_rn and every product that feeds a sum or a difference goes through rounded(), as in the forward
// (-ffp-contract=fast would otherwise fuse them per instantiation).
#include <hip/hip_runtime.h>

#include "nrnerf_grid_grad.h"
#include "nrnerf_composite_ray.h"
#include "nrnerf_volume_lookup.h"

namespace nrn {

namespace {

__device__ __forceinline__ f32x4 sub4(const f32x4 b, const f32x4 a) {
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = __fsub_rn(b[c], a[c]);
    return r;
}

// sum over the channels of g_ch d_ch, channel 0 first
__device__ __forceinline__ float dot4(const f32x4 g, const f32x4 d) {
    return __fmaf_rn(g[3], d[3], __fmaf_rn(g[2], d[2], __fmaf_rn(g[1], d[1], rounded(g[0] * d[0]))));
}

template <bool HALF>
__global__ void __launch_bounds__(256) grid_point_grad_kernel(const GridGradArgs a) {
    const long long step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < a.n_points; t += step) {
        const __attribute__((address_space(1))) float* pp = gmem(a.points) + (size_t)t * a.point_stride;
        int i[3];
        float f[3];
        bool ok;
        grid_cell(a.grid, pp[0], pp[1], pp[2], i, f, ok);
        float dp[3] = {0.0f, 0.0f, 0.0f};                      // outside the box, or NaN: no gradient
        if (ok) {
            const f32x4 g = *(const __attribute__((address_space(1))) f32x4*)(gmem(a.g_value) + (size_t)t * 4);
            const size_t gx = (size_t)a.grid.g[0], gxy = gx * (size_t)a.grid.g[1];
            const size_t v = (size_t)i[2] * gxy + (size_t)i[1] * gx + (size_t)i[0];
            f32x4 c000, c100, c010, c110, c001, c101, c011, c111;
            load_pair<HALF>(a.grid.vol, v, c000, c100);
            load_pair<HALF>(a.grid.vol, v + gx, c010, c110);
            load_pair<HALF>(a.grid.vol, v + gxy, c001, c101);
            load_pair<HALF>(a.grid.vol, v + gxy + gx, c011, c111);
            // dv / df_x: the differences along x, interpolated along y, then z
            const f32x4 ddx = lerp4(lerp4(sub4(c100, c000), sub4(c110, c010), f[1]), lerp4(sub4(c101, c001), sub4(c111, c011), f[1]), f[2]);
            // dv / df_y, dv / df_z: the forward's x-interpolations, their differences along the axis interpolated along the other one
            const f32x4 x00 = lerp4(c000, c100, f[0]), x10 = lerp4(c010, c110, f[0]);
            const f32x4 x01 = lerp4(c001, c101, f[0]), x11 = lerp4(c011, c111, f[0]);
            const f32x4 ddy = lerp4(sub4(x10, x00), sub4(x11, x01), f[2]);
            const f32x4 ddz = lerp4(sub4(x01, x00), sub4(x11, x10), f[1]);
            dp[0] = rounded(a.grid.scale[0] * dot4(g, ddx));
            dp[1] = rounded(a.grid.scale[1] * dot4(g, ddy));
            dp[2] = rounded(a.grid.scale[2] * dot4(g, ddz));
        }
        __attribute__((address_space(1))) float* out = gmem(a.d_points) + (size_t)t * 3;
        out[0] = dp[0]; out[1] = dp[1]; out[2] = dp[2];
    }
}

// thread t: lane (dx, c) = (bit 2, bits 0 .. 1 of t) of point t / 8; an empty sample (outside the box, or NaN) adds nothing
__global__ void __launch_bounds__(256) grid_scatter_kernel(const GridGradArgs a) {
    const long long total = a.n_points * 8, step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const long long pt = t >> 3;
        const int c = (int)t & 3, dx = ((int)t >> 2) & 1;
        const __attribute__((address_space(1))) float* pp = gmem(a.points) + (size_t)pt * a.point_stride;
        int i[3];
        float f[3];
        bool ok;
        grid_cell(a.grid, pp[0], pp[1], pp[2], i, f, ok);
        if (!ok) continue;
        const float g = gmem(a.g_value)[(size_t)pt * 4 + c];
        const size_t gx = (size_t)a.grid.g[0], gxy = gx * (size_t)a.grid.g[1];
        const size_t v = (size_t)i[2] * gxy + (size_t)i[1] * gx + (size_t)i[0] + dx;
        const float wx = dx ? f[0] : __fsub_rn(1.0f, f[0]);
        const float wy[2] = {__fsub_rn(1.0f, f[1]), f[1]}, wz[2] = {__fsub_rn(1.0f, f[2]), f[2]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float w = rounded(rounded(wx * wy[k & 1]) * wz[k >> 1]);
            unsafeAtomicAdd(a.d_grid + (v + (k & 1) * gx + (k >> 1) * gxy) * 4 + c, rounded(w * g));
        }
    }
}

}  // namespace

hipError_t launch_grid_lookup_backward(const GridGradArgs& a, int num_cus, hipStream_t stream) {
    if (!a.d_grid && !a.d_points) return hipErrorInvalidValue;
    if (a.n_points <= 0) return hipSuccess;
    const long long cap = (long long)(num_cus > 0 ? num_cus : 256) * 32;
    if (a.d_grid) {
        const long long want = (a.n_points * 8 + 255) / 256;
        hipLaunchKernelGGL(grid_scatter_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.d_points) {
        const long long want = (a.n_points + 255) / 256;
        const dim3 grid((unsigned)(want < cap ? want : cap));
        if (a.grid.half) hipLaunchKernelGGL(grid_point_grad_kernel<true>, grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(grid_point_grad_kernel<false>, grid, dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace nrn
