// nrnerf_visualize.hip -- the per-frame images and scores of the reference's free_viewpoint_rendering.py (fvr) on the device
// (include/nrnerf.h, ABI 9): the disparity / rigidity / correspondence maps, PSNR and SSIM with their error maps, and the
// background-stability map of a fixed-camera sequence.
//
// The arithmetic restates the numpy expressions operation by operation, in the dtype numpy computes them in (float32 where it stays
// in float32, double where it promotes), so that the uint8 images match the reference byte for byte.  This unit is compiled with
// -ffp-contract=off: a fused multiply-add would round differently from numpy.  Nothing here needs MFMA; the work is a few tens of
// bytes per pixel.
#include <hip/hip_runtime.h>

#include <math.h>

#include "nrnerf.h"

namespace {

// to8b(matplotlib cm.jet(i)[:3]) for i = 0..255 (rnh:701-715 index the colour map with the uint8 value; fvr then writes to8b of it)
__constant__ uint8_t JET[256 * 3] = {
    0, 0, 127, 0, 0, 132, 0, 0, 136, 0, 0, 141, 0, 0, 145, 0, 0, 150, 0, 0, 154, 0, 0, 159,
    0, 0, 163, 0, 0, 168, 0, 0, 172, 0, 0, 177, 0, 0, 182, 0, 0, 186, 0, 0, 191, 0, 0, 195,
    0, 0, 200, 0, 0, 204, 0, 0, 209, 0, 0, 213, 0, 0, 218, 0, 0, 222, 0, 0, 227, 0, 0, 232,
    0, 0, 236, 0, 0, 241, 0, 0, 245, 0, 0, 250, 0, 0, 254, 0, 0, 255, 0, 0, 255, 0, 0, 255,
    0, 0, 255, 0, 4, 255, 0, 8, 255, 0, 12, 255, 0, 16, 255, 0, 20, 255, 0, 24, 255, 0, 28, 255,
    0, 32, 255, 0, 36, 255, 0, 40, 255, 0, 44, 255, 0, 48, 255, 0, 52, 255, 0, 56, 255, 0, 60, 255,
    0, 64, 255, 0, 68, 255, 0, 72, 255, 0, 76, 255, 0, 80, 255, 0, 84, 255, 0, 88, 255, 0, 92, 255,
    0, 96, 255, 0, 100, 255, 0, 104, 255, 0, 108, 255, 0, 112, 255, 0, 116, 255, 0, 120, 255, 0, 124, 255,
    0, 128, 255, 0, 132, 255, 0, 136, 255, 0, 140, 255, 0, 144, 255, 0, 148, 255, 0, 152, 255, 0, 156, 255,
    0, 160, 255, 0, 164, 255, 0, 168, 255, 0, 172, 255, 0, 176, 255, 0, 180, 255, 0, 184, 255, 0, 188, 255,
    0, 192, 255, 0, 196, 255, 0, 200, 255, 0, 204, 255, 0, 208, 255, 0, 212, 255, 0, 216, 255, 0, 220, 254,
    0, 224, 250, 0, 228, 247, 2, 232, 244, 5, 236, 241, 8, 240, 237, 12, 244, 234, 15, 248, 231, 18, 252, 228,
    21, 255, 225, 24, 255, 221, 28, 255, 218, 31, 255, 215, 34, 255, 212, 37, 255, 208, 41, 255, 205, 44, 255, 202,
    47, 255, 199, 50, 255, 195, 54, 255, 192, 57, 255, 189, 60, 255, 186, 63, 255, 183, 66, 255, 179, 70, 255, 176,
    73, 255, 173, 76, 255, 170, 79, 255, 166, 83, 255, 163, 86, 255, 160, 89, 255, 157, 92, 255, 154, 95, 255, 150,
    99, 255, 147, 102, 255, 144, 105, 255, 141, 108, 255, 137, 112, 255, 134, 115, 255, 131, 118, 255, 128, 121, 255, 125,
    124, 255, 121, 128, 255, 118, 131, 255, 115, 134, 255, 112, 137, 255, 108, 141, 255, 105, 144, 255, 102, 147, 255, 99,
    150, 255, 95, 154, 255, 92, 157, 255, 89, 160, 255, 86, 163, 255, 83, 166, 255, 79, 170, 255, 76, 173, 255, 73,
    176, 255, 70, 179, 255, 66, 183, 255, 63, 186, 255, 60, 189, 255, 57, 192, 255, 54, 195, 255, 50, 199, 255, 47,
    202, 255, 44, 205, 255, 41, 208, 255, 37, 212, 255, 34, 215, 255, 31, 218, 255, 28, 221, 255, 24, 224, 255, 21,
    228, 255, 18, 231, 255, 15, 234, 255, 12, 237, 255, 8, 241, 252, 5, 244, 248, 2, 247, 244, 0, 250, 240, 0,
    254, 237, 0, 255, 233, 0, 255, 229, 0, 255, 226, 0, 255, 222, 0, 255, 218, 0, 255, 215, 0, 255, 211, 0,
    255, 207, 0, 255, 203, 0, 255, 200, 0, 255, 196, 0, 255, 192, 0, 255, 189, 0, 255, 185, 0, 255, 181, 0,
    255, 177, 0, 255, 174, 0, 255, 170, 0, 255, 166, 0, 255, 163, 0, 255, 159, 0, 255, 155, 0, 255, 152, 0,
    255, 148, 0, 255, 144, 0, 255, 140, 0, 255, 137, 0, 255, 133, 0, 255, 129, 0, 255, 126, 0, 255, 122, 0,
    255, 118, 0, 255, 115, 0, 255, 111, 0, 255, 107, 0, 255, 103, 0, 255, 100, 0, 255, 96, 0, 255, 92, 0,
    255, 89, 0, 255, 85, 0, 255, 81, 0, 255, 77, 0, 255, 74, 0, 255, 70, 0, 255, 66, 0, 255, 63, 0,
    255, 59, 0, 255, 55, 0, 255, 52, 0, 255, 48, 0, 255, 44, 0, 255, 40, 0, 255, 37, 0, 255, 33, 0,
    255, 29, 0, 255, 26, 0, 255, 22, 0, 254, 18, 0, 250, 15, 0, 245, 11, 0, 241, 7, 0, 236, 3, 0,
    232, 0, 0, 227, 0, 0, 222, 0, 0, 218, 0, 0, 213, 0, 0, 209, 0, 0, 204, 0, 0, 200, 0, 0,
    195, 0, 0, 191, 0, 0, 186, 0, 0, 182, 0, 0, 177, 0, 0, 172, 0, 0, 168, 0, 0, 163, 0, 0,
    159, 0, 0, 154, 0, 0, 150, 0, 0, 145, 0, 0, 141, 0, 0, 136, 0, 0, 132, 0, 0, 127, 0, 0
};

// scipy.ndimage._gaussian_kernel1d(sigma=1.5, order=0, radius=int(3.5 * 1.5 + 0.5) = 5): the weights skimage's SSIM filters with
constexpr double GW0 = 0.26601172486179436, GW1 = 0.2130055377112537, GW2 = 0.10936068950970002, GW3 = 0.03600077212843083,
                 GW4 = 0.007598758135239185, GW5 = 0.00102838008447911;
constexpr int RAD = 5;
constexpr int TILE = 16;                     // output pixels per side of an SSIM workgroup
constexpr int SPAN = TILE + 2 * RAD;         // with the halo
constexpr int NPART = 4;                     // per-tile partials: sum of S over the crop per channel, sum of d^2

__device__ __forceinline__ uint8_t to8b_f(float x) {          // (255 * np.clip(x, 0, 1)).astype(np.uint8), float32
    x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    return (uint8_t)(int)(255.0f * x);
}
__device__ __forceinline__ uint8_t to8b_d(double x) {         // ... on a float64 array
    x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    return (uint8_t)(int)(255.0 * x);
}
__device__ __forceinline__ void put_jet(uint8_t* o, int idx) {
    o[0] = JET[3 * idx]; o[1] = JET[3 * idx + 1]; o[2] = JET[3 * idx + 2];
}
__device__ __forceinline__ int jet_index_f(float x) {        // rnh:707-711 on float32: clip to [0, 1], / 1, 255. * x, astype uint8
    x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    return (int)(uint8_t)(int)(255.0f * x);
}
__device__ __forceinline__ int jet_index_d(double x) {       // ... on float64
    x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    return (int)(uint8_t)(int)(255.0 * x);
}

// ------------------------------------------------------------------------------------------------------------------------------
// max of the disparity (np.max: NaN propagates).  One workgroup per frame, or one over the whole stack.
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float max_nan(float a, float b) { return a != a ? a : ((b != b || b > a) ? b : a); }

__global__ void __launch_bounds__(1024) frame_max_kernel(const float* __restrict__ disp, int64_t per, float* __restrict__ out, int n_out) {
    __shared__ float red[1024];
    const int64_t base = (int64_t)blockIdx.x * per;
    float m = -INFINITY;
    for (int64_t i = threadIdx.x; i < per; i += blockDim.x) m = max_nan(m, disp[base + i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max_nan(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (n_out == 1) out[blockIdx.x] = red[0];
        else for (int f = 0; f < n_out; ++f) out[f] = red[0];         // the stack's max for every frame
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// point-wise and stencil maps: one thread per pixel, gridDim.y = frames
// ------------------------------------------------------------------------------------------------------------------------------
struct MapArgs {
    uint32_t flags;
    int F, H, W, normalize;
    const float* disp; const float* disp_max;
    const float* pts; double mn[3], mx[3]; int voxels;
    const float* rig;
    uint8_t *o_disp, *o_jet, *o_phong, *o_corr, *o_rig, *o_rig_jet;
};

// rnh:718-791 on the normalised float32 disparity of the pixel (y, x) and its neighbours (np.gradient with spacing 2 / (H - 1) on both axes)
__device__ void blinn_phong(const float* __restrict__ d, float mx, bool norm, int H, int W, int y, int x, uint8_t* o) {
    auto nv = [&](int yy, int xx) -> float { float v = d[(int64_t)yy * W + xx]; return norm ? v / mx : v; };
    const double spacing = 2.0 / (double)(H - 1);
    const float sp1 = (float)spacing, sp2 = (float)(2.0 * spacing);
    float zy, zx;
    if (y == 0) zy = (nv(1, x) - nv(0, x)) / sp1;
    else if (y == H - 1) zy = (nv(H - 1, x) - nv(H - 2, x)) / sp1;
    else zy = (nv(y + 1, x) - nv(y - 1, x)) / sp2;
    if (x == 0) zx = (nv(y, 1) - nv(y, 0)) / sp1;
    else if (x == W - 1) zx = (nv(y, W - 1) - nv(y, W - 2)) / sp1;
    else zx = (nv(y, x + 1) - nv(y, x - 1)) / sp2;
    const float depth = nv(y, x);
    // normal = (-zx, zy, 1) / |.|, float32 (rnh:733-738)
    float n0 = -zx, n1 = zy, n2 = 1.0f;
    const float nl = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
    n0 = n0 / nl; n1 = n1 / nl; n2 = n2 / nl;
    // vertPos = (x / W, y / W, depth), float32 (rnh:740-747)
    const float vi = (float)x / (float)W, vj = (float)y / (float)W;
    // lightDir = lightPos - vertPos, float64 (rnh:749-753)
    double l0 = 1.0 + (double)(-vi), l1 = 1.0 + (double)(-vj), l2 = 1.0 + (double)(-depth);
    double dist = sqrt((l0 * l0 + l1 * l1) + l2 * l2);
    l0 = l0 / dist; l1 = l1 / dist; l2 = l2 / dist;
    dist = (dist + 1.0) * (dist + 1.0);
    double lamb = (l0 * (double)n0 + l1 * (double)n1) + l2 * (double)n2;
    lamb = lamb < 0.0 ? 0.0 : lamb;
    const bool invalid = lamb <= 0.0;
    // viewDir = normalize(-vertPos), float32; halfDir = normalize(lightDir + viewDir), float64 (rnh:766-768)
    const float w0 = -vi, w1 = -vj, w2 = -depth;
    const float wl = sqrtf((w0 * w0 + w1 * w1) + w2 * w2);
    const float v0 = w0 / wl, v1 = w1 / wl, v2 = w2 / wl;
    double h0 = l0 + (double)v0, h1 = l1 + (double)v1, h2 = l2 + (double)v2;
    const double hl = sqrt((h0 * h0 + h1 * h1) + h2 * h2);
    h0 = h0 / hl; h1 = h1 / hl; h2 = h2 / hl;
    double sa = (h0 * (double)(-n0) + h1 * (double)(-n1)) + h2 * (double)(-n2);
    sa = sa < 0.0 ? 0.0 : sa;
    double spec = sa * sa;                                     // shininess 2.0: numpy squares
    if (invalid) spec = 0.0;
    // colorLinear (rnh:776-790): lightColor = specColor = 1, lightPower = 2, diffuse (0.5, 0, 0), ambient (0.1, 0, 0)
    const double specular = ((spec * 1.0) * 1.0) * 2.0 / dist;
    const double diff[3] = {0.5, 0.0, 0.0}, amb[3] = {0.1, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double col = (((lamb * diff[c]) * 1.0) * 2.0 / dist + specular) + amb[c];
        o[c] = to8b_d(col);
    }
}

__global__ void __launch_bounds__(256) maps_kernel(const MapArgs a) {
    const int64_t HW = (int64_t)a.H * a.W;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y;
    if (p >= HW) return;
    const int64_t q = (int64_t)f * HW + p;                  // pixel index in the stack
    const int y = (int)(p / a.W), x = (int)(p % a.W);
    if (a.flags & (NRNERF_VIS_DISP | NRNERF_VIS_DISP_JET | NRNERF_VIS_DISP_PHONG)) {
        const bool norm = a.normalize != NRNERF_VIS_NORM_NONE;
        const float mx = norm ? a.disp_max[f] : 1.0f;
        const float* d = a.disp + (int64_t)f * HW;
        const float v = norm ? d[p] / mx : d[p];             // fvr:355 disparity / np.max(disparity), float32
        if (a.flags & NRNERF_VIS_DISP) a.o_disp[q] = to8b_f(v);
        if (a.flags & NRNERF_VIS_DISP_JET) put_jet(a.o_jet + 3 * q, jet_index_f(v));
        if (a.flags & NRNERF_VIS_DISP_PHONG) blinn_phong(d, mx, norm, a.H, a.W, y, x, a.o_phong + 3 * q);
    }
    if (a.flags & NRNERF_VIS_CORRESPONDENCES) {              // fvr:638-645, float64 (min_point / max_point are float64 arrays)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double r = ((double)a.pts[3 * q + c] - a.mn[c]) / (a.mx[c] - a.mn[c]);
            if (a.voxels > 1) {
                r = r * (double)a.voxels;
                r = r - trunc(r);                            // x - x.astype(int): toward zero, negatives stay negative (to8b clips them)
            }
            a.o_corr[3 * q + c] = to8b_d(r);
        }
    }
    if (a.flags & (NRNERF_VIS_RIGIDITY | NRNERF_VIS_RIGIDITY_JET)) {   // fvr:665-668, normalize=False
        const float v = a.rig[q];
        if (a.flags & NRNERF_VIS_RIGIDITY) a.o_rig[q] = to8b_f(v);
        if (a.flags & NRNERF_VIS_RIGIDITY_JET) put_jet(a.o_rig_jet + 3 * q, jet_index_f(v));
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// PSNR / SSIM: one 16 x 16 tile of one frame per workgroup, the three channels one after the other
// ------------------------------------------------------------------------------------------------------------------------------
struct MetricArgs {
    int F, H, W, tiles_x, tiles;
    const float* gt; const float* ren; const float* mask;
    double* ssim_map; uint8_t* mse_map; uint8_t* ssim_err; double* part;
    double* psnr; double* ssim; double* mse;
};

__device__ __forceinline__ int reflect(int i, int n) {      // scipy.ndimage mode 'reflect': d c b a | a b c d | d c b a, any distance
    if (n == 1) return 0;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}
__device__ __forceinline__ bool masked(const float* m, int64_t pix) {     // fvr:820: np.sum(groundtruth, axis=-1) == 0., float32
    if (!m) return false;
    return ((m[3 * pix] + m[3 * pix + 1]) + m[3 * pix + 2]) == 0.0f;
}
// scipy's correlate1d for a symmetric kernel (ni_filters.c): v(0) * w0, then += (v(-j) + v(j)) * w_j for j = radius .. 1
template <class V>
__device__ __forceinline__ double gsym(V v) {
    double t = v(0) * GW0;
    t += (v(-5) + v(5)) * GW5;
    t += (v(-4) + v(4)) * GW4;
    t += (v(-3) + v(3)) * GW3;
    t += (v(-2) + v(2)) * GW2;
    t += (v(-1) + v(1)) * GW1;
    return t;
}

__global__ void __launch_bounds__(256) ssim_tile_kernel(const MetricArgs a) {
    __shared__ double X[SPAN * SPAN], Y[SPAN * SPAN];
    __shared__ double Q[5][SPAN * TILE];                    // vertical pass: [x, y, xx, yy, xy] for TILE rows x SPAN columns
    __shared__ double red[NPART][256];
    const int f = blockIdx.y, tile = blockIdx.x;
    const int ty0 = (tile / a.tiles_x) * TILE, tx0 = (tile % a.tiles_x) * TILE;
    const int t = threadIdx.x, ly = t / TILE, lx = t % TILE;
    const int y = ty0 + ly, x = tx0 + lx;
    const bool inside = y < a.H && x < a.W;
    const int64_t HW = (int64_t)a.H * a.W;
    const float* g = a.gt + (int64_t)f * HW * 3;
    const float* r = a.ren + (int64_t)f * HW * 3;
    const bool crop = inside && y >= RAD && y < a.H - RAD && x >= RAD && x < a.W - RAD;
    const int64_t pix = (int64_t)y * a.W + x;
    const bool mine_masked = inside && masked(a.mask, pix);
    double part[NPART] = {0.0, 0.0, 0.0, 0.0};
    double s_sum = 0.0;
    float d[3] = {0.0f, 0.0f, 0.0f};
    for (int c = 0; c < 3; ++c) {
        for (int i = t; i < SPAN * SPAN; i += 256) {
            const int gy = reflect(ty0 - RAD + i / SPAN, a.H), gx = reflect(tx0 - RAD + i % SPAN, a.W);
            const int64_t gp = (int64_t)gy * a.W + gx;
            const bool m = masked(a.mask, gp);
            X[i] = m ? 0.0 : (double)g[3 * gp + c];
            Y[i] = m ? 0.0 : (double)r[3 * gp + c];
        }
        __syncthreads();
        // axis 0 first, as scipy's gaussian_filter: rows ty0 .. ty0 + TILE of every halo column
        for (int i = t; i < TILE * SPAN; i += 256) {
            const int oy = i / SPAN, ox = i % SPAN;
            const double* xs = X + (oy + RAD) * SPAN + ox;
            const double* ys = Y + (oy + RAD) * SPAN + ox;
            Q[0][i] = gsym([&](int k) { return xs[k * SPAN]; });
            Q[1][i] = gsym([&](int k) { return ys[k * SPAN]; });
            Q[2][i] = gsym([&](int k) { return xs[k * SPAN] * xs[k * SPAN]; });
            Q[3][i] = gsym([&](int k) { return ys[k * SPAN] * ys[k * SPAN]; });
            Q[4][i] = gsym([&](int k) { return xs[k * SPAN] * ys[k * SPAN]; });
        }
        __syncthreads();
        if (inside) {
            // axis 1: the TILE columns of this row (column lx + RAD of the halo span is the pixel itself)
            const int at = ly * SPAN + lx + RAD;
            const double ux = gsym([&](int k) { return Q[0][at + k]; }), uy = gsym([&](int k) { return Q[1][at + k]; });
            const double uxx = gsym([&](int k) { return Q[2][at + k]; }), uyy = gsym([&](int k) { return Q[3][at + k]; });
            const double uxy = gsym([&](int k) { return Q[4][at + k]; });
            // skimage structural_similarity, use_sample_covariance=False (cov_norm = 1), data_range = 1
            const double vx = 1.0 * (uxx - ux * ux), vy = 1.0 * (uyy - uy * uy), vxy = 1.0 * (uxy - ux * uy);
            const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
            const double A1 = (2.0 * ux) * uy + C1, A2 = 2.0 * vxy + C2;
            const double B1 = (ux * ux + uy * uy) + C1, B2 = (vx + vy) + C2;
            const double S = (A1 * A2) / (B1 * B2);
            if (a.ssim_map) a.ssim_map[((int64_t)f * HW + pix) * 3 + c] = S;
            s_sum = c == 0 ? S : s_sum + S;
            if (crop) part[c] = S;
            // the pixel's own difference, float32 as numpy (groundtruth - generated after the mask)
            const float gv = mine_masked ? 0.0f : g[3 * pix + c], rv = mine_masked ? 0.0f : r[3 * pix + c];
            d[c] = gv - rv;
            part[3] += (double)d[c] * (double)d[c];
        }
        __syncthreads();                                   // X / Y / Q are reloaded for the next channel
    }
    if (inside) {
        const int64_t o = ((int64_t)f * HW + pix) * 3;
        if (a.ssim_err) put_jet(a.ssim_err + o, jet_index_d(1.0 - s_sum / 3.0));       // fvr:858: 1 - np.mean(S, axis=-1)
        if (a.mse_map) {                                                                // fvr:850-853
            const float nrm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            double e = (double)nrm / sqrt(3.0);              // np.linalg.norm (float32) / np.sqrt(1 + 1 + 1) (a float64 scalar)
            e = e * 10.0;
            e = e < 0.0 ? 0.0 : (e > 1.0 ? 1.0 : e);
            put_jet(a.mse_map + o, jet_index_d(e));
        }
    }
    // the tile's partials: a fixed tree over the 256 pixels
#pragma unroll
    for (int k = 0; k < NPART; ++k) red[k][t] = part[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int k = 0; k < NPART; ++k) red[k][t] = red[k][t] + red[k][t + s];
        __syncthreads();
    }
    if (t < NPART) a.part[((int64_t)f * a.tiles + tile) * NPART + t] = red[t][0];
}

__global__ void __launch_bounds__(256) metrics_finish_kernel(const MetricArgs a) {
    __shared__ double red[NPART][256];
    const int f = blockIdx.x, t = threadIdx.x;
    double s[NPART] = {0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < a.tiles; i += 256)                 // tiles in a fixed order per thread, then a fixed tree
#pragma unroll
        for (int k = 0; k < NPART; ++k) s[k] += a.part[((int64_t)f * a.tiles + i) * NPART + k];
#pragma unroll
    for (int k = 0; k < NPART; ++k) red[k][t] = s[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w)
#pragma unroll
            for (int k = 0; k < NPART; ++k) red[k][t] = red[k][t] + red[k][t + w];
        __syncthreads();
    }
    if (t == 0) {
        const double n_crop = (double)(a.H - 2 * RAD > 0 ? a.H - 2 * RAD : 0) * (double)(a.W - 2 * RAD > 0 ? a.W - 2 * RAD : 0);
        const double m0 = red[0][0] / n_crop, m1 = red[1][0] / n_crop, m2 = red[2][0] / n_crop;   // 0 / 0 = NaN for an empty crop
        a.ssim[f] = ((m0 + m1) + m2) / 3.0;
        const double mse = red[3][0] / ((double)a.H * (double)a.W * 3.0);
        if (a.mse) a.mse[f] = mse;
        a.psnr[f] = -10.0 * log10(mse);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// background stability (fvr:767-785)
// ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) stability_acc_kernel(const float* __restrict__ rgb, int64_t n, double* __restrict__ sum, double* __restrict__ sq) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = (double)rgb[i];
    sum[i] = sum[i] + v;
    sq[i] = sq[i] + v * v;
}

__global__ void __launch_bounds__(256) stability_finish_kernel(const double* __restrict__ sum, const double* __restrict__ sq, int F, int64_t n_pix,
                                                               uint8_t* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pix) return;
    const double fn = (double)F;
    double sd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double m = sum[3 * p + c] / fn;
        double var = sq[3 * p + c] / fn - m * m;
        var = var < 0.0 ? 0.0 : var;
        sd[c] = sqrt(var);
    }
    const double v = 10.0 * (((sd[0] + sd[1]) + sd[2]) / 3.0);
    put_jet(out + 3 * p, jet_index_d(v));
}

int device_of(const void* ptr, int& dev) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) { (void)hipGetLastError(); return NRNERF_ERR_INVALID; }
    if (attr.type != hipMemoryTypeDevice) return NRNERF_ERR_INVALID;
    dev = attr.device;
    return NRNERF_OK;
}
struct Guard {                                              // the device that owns the output, for the duration of the call
    int prev = -1;
    bool ok = true;
    explicit Guard(int want) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; prev = -1; return; }
        if (prev != want && hipSetDevice(want) != hipSuccess) ok = false;
        if (prev == want) prev = -1;
    }
    ~Guard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
inline int launched() { return hipGetLastError() == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP; }
inline int tiles_of(int H, int W, int& tx) { tx = (W + TILE - 1) / TILE; return tx * ((H + TILE - 1) / TILE); }

}  // namespace

#define NRN_VIS_CATCH catch (...) { return NRNERF_ERR_INTERNAL; }

extern "C" {

int nrnerf_visualize_frames(const nrnerf_visualize_args* args, void* hip_stream) try {
    if (!args || args->struct_size != sizeof(nrnerf_visualize_args)) return NRNERF_ERR_INVALID;
    const nrnerf_visualize_args& v = *args;
    const uint32_t all = NRNERF_VIS_DISP | NRNERF_VIS_DISP_JET | NRNERF_VIS_DISP_PHONG | NRNERF_VIS_CORRESPONDENCES | NRNERF_VIS_RIGIDITY |
                         NRNERF_VIS_RIGIDITY_JET;
    if ((v.flags & ~all) || v.n_frames < 0 || v.height < 1 || v.width < 1 || v.normalize < 0 || v.normalize > 3) return NRNERF_ERR_INVALID;
    if (v.n_frames == 0 || v.flags == 0) return NRNERF_OK;
    const bool want_disp = v.flags & (NRNERF_VIS_DISP | NRNERF_VIS_DISP_JET | NRNERF_VIS_DISP_PHONG);
    if (want_disp && (!v.disp || (v.normalize != NRNERF_VIS_NORM_NONE && !v.disp_max))) return NRNERF_ERR_INVALID;
    if ((v.flags & NRNERF_VIS_DISP && !v.disp_out) || (v.flags & NRNERF_VIS_DISP_JET && !v.disp_jet) ||
        (v.flags & NRNERF_VIS_DISP_PHONG && (!v.disp_phong || v.height < 2 || v.width < 2)) ||
        (v.flags & NRNERF_VIS_CORRESPONDENCES && (!v.surface_pts || !v.correspondences)) ||
        (v.flags & (NRNERF_VIS_RIGIDITY | NRNERF_VIS_RIGIDITY_JET) && !v.rigidity) ||
        (v.flags & NRNERF_VIS_RIGIDITY && !v.rigidity_out) || (v.flags & NRNERF_VIS_RIGIDITY_JET && !v.rigidity_jet))
        return NRNERF_ERR_INVALID;
    const void* first = v.disp_out ? (const void*)v.disp_out : v.disp_jet ? (const void*)v.disp_jet : v.disp_phong ? (const void*)v.disp_phong
                      : v.correspondences ? (const void*)v.correspondences : v.rigidity_out ? (const void*)v.rigidity_out : (const void*)v.rigidity_jet;
    int dev = 0;
    if (!first || device_of(first, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    Guard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    hipStream_t st = (hipStream_t)hip_stream;
    const int64_t HW = (int64_t)v.height * v.width;
    if (HW > (int64_t)INT32_MAX) return NRNERF_ERR_INVALID;
    if (want_disp && v.normalize == NRNERF_VIS_NORM_FRAME)
        frame_max_kernel<<<v.n_frames, 1024, 0, st>>>(v.disp, HW, v.disp_max, 1);
    else if (want_disp && v.normalize == NRNERF_VIS_NORM_STACK)
        frame_max_kernel<<<1, 1024, 0, st>>>(v.disp, HW * v.n_frames, v.disp_max, v.n_frames);
    MapArgs m{};
    m.flags = v.flags; m.F = v.n_frames; m.H = v.height; m.W = v.width; m.normalize = v.normalize;
    m.disp = v.disp; m.disp_max = v.disp_max; m.pts = v.surface_pts; m.voxels = v.voxels; m.rig = v.rigidity;
    for (int c = 0; c < 3; ++c) { m.mn[c] = v.min_point[c]; m.mx[c] = v.max_point[c]; }
    m.o_disp = v.disp_out; m.o_jet = v.disp_jet; m.o_phong = v.disp_phong; m.o_corr = v.correspondences; m.o_rig = v.rigidity_out;
    m.o_rig_jet = v.rigidity_jet;
    maps_kernel<<<dim3((unsigned)((HW + 255) / 256), v.n_frames), 256, 0, st>>>(m);
    return launched();
} NRN_VIS_CATCH

size_t nrnerf_visualize_workspace_bytes(int32_t n_frames, int32_t height, int32_t width) {
    if (n_frames < 0 || height < 1 || width < 1) return 0;
    int tx = 0;
    return (size_t)n_frames * (size_t)tiles_of(height, width, tx) * NPART * sizeof(double);
}

int nrnerf_image_metrics(const nrnerf_metrics_args* args, void* hip_stream) try {
    if (!args || args->struct_size != sizeof(nrnerf_metrics_args)) return NRNERF_ERR_INVALID;
    const nrnerf_metrics_args& v = *args;
    if (v.n_frames < 0 || v.height < 1 || v.width < 1 || !v.gt || !v.rendered || !v.psnr || !v.ssim) return NRNERF_ERR_INVALID;
    if ((int64_t)v.height * v.width > (int64_t)INT32_MAX / 3) return NRNERF_ERR_INVALID;
    if (v.n_frames == 0) return NRNERF_OK;
    if (!v.workspace || v.workspace_bytes < nrnerf_visualize_workspace_bytes(v.n_frames, v.height, v.width)) return NRNERF_ERR_WORKSPACE;
    int dev = 0;
    if (device_of(v.psnr, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    Guard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    hipStream_t st = (hipStream_t)hip_stream;
    MetricArgs m{};
    m.F = v.n_frames; m.H = v.height; m.W = v.width;
    m.tiles = tiles_of(v.height, v.width, m.tiles_x);
    m.gt = v.gt; m.ren = v.rendered; m.mask = v.mask_ref;
    m.ssim_map = v.ssim_map; m.mse_map = v.mse_error_map; m.ssim_err = v.ssim_error_map; m.part = (double*)v.workspace;
    m.psnr = v.psnr; m.ssim = v.ssim; m.mse = v.mse;
    ssim_tile_kernel<<<dim3(m.tiles, v.n_frames), 256, 0, st>>>(m);
    metrics_finish_kernel<<<v.n_frames, 256, 0, st>>>(m);
    return launched();
} NRN_VIS_CATCH

int nrnerf_stability_accumulate(const float* rgb, int64_t n_values, double* sum, double* sum_sq, void* hip_stream) try {
    if (!rgb || !sum || !sum_sq || n_values < 0) return NRNERF_ERR_INVALID;
    if (n_values == 0) return NRNERF_OK;
    int dev = 0;
    if (device_of(sum, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    Guard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    stability_acc_kernel<<<(unsigned)((n_values + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(rgb, n_values, sum, sum_sq);
    return launched();
} NRN_VIS_CATCH

int nrnerf_stability_finish(const double* sum, const double* sum_sq, int32_t n_frames, int64_t n_pixels, uint8_t* out_rgb, void* hip_stream) try {
    if (!sum || !sum_sq || !out_rgb || n_frames < 1 || n_pixels < 0) return NRNERF_ERR_INVALID;
    if (n_pixels == 0) return NRNERF_OK;
    int dev = 0;
    if (device_of(out_rgb, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    Guard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    stability_finish_kernel<<<(unsigned)((n_pixels + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(sum, sum_sq, n_frames, n_pixels, out_rgb);
    return launched();
} NRN_VIS_CATCH

}  // extern "C"
