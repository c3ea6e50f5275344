// nrnerf_isosurface.hip -- marching tetrahedra over the Kuhn triangulation of a regular grid: count, scan, emit.  The definitions (inside,
// owner / slot of an edge, the sixteen cases, the orders of vertices and triangles) are stated ONCE, in nrnerf_isosurface.h; this file follows
// that text.  Bandwidth-bound: every pass is one thread per grid vertex over consecutive linear indices (x fastest), so a wave's loads of a
// corner are 64 consecutive floats; a value is read eight times by the count pass (its eight cells), from L1 / L2 after the first.  No atomics:
// the same bytes on every run.  Every index is checked against its count and every store against the caller's capacity.
#include "nrnerf_isosurface.h"

namespace nrn {
namespace {

// ---- the triangulation as bit fields (no table in memory, nothing indexed at run time) ------------------------------------------------------
// local corners 1 and 2 of tetrahedron t as cell corner codes (local corner 0 is cell corner 0, local corner 3 is cell corner 7)
__device__ constexpr unsigned tet_c1(int t) { return t < 2 ? 1u : t < 4 ? 2u : 4u; }
__device__ constexpr unsigned tet_c2(int t) { return (0x656353u >> (4 * t)) & 7u; }          // 3 5 3 6 5 6
__device__ constexpr bool tet_odd(int t) { return (0x26u >> t) & 1u; }                       // tetrahedra 1, 2, 5
// tetrahedron edges 0..5 = 01 02 03 12 13 23: their two local corners, two bits each
constexpr unsigned EDGE_I = 0u | 0u << 2 | 0u << 4 | 1u << 6 | 1u << 8 | 2u << 10;
constexpr unsigned EDGE_J = 1u | 2u << 2 | 3u << 4 | 2u << 6 | 3u << 8 | 3u << 10;
constexpr unsigned long long tri(unsigned a, unsigned b, unsigned c) { return a | b << 3 | c << 6; }
enum : unsigned { E01, E02, E03, E12, E13, E23 };
// the cases m = 1 .. 7 of a positively oriented tetrahedron, nine bits per triangle at 9 (m - 1); m >= 8 is row 15 - m with the winding flipped
constexpr unsigned long long TRI0 = tri(E01, E02, E03) | tri(E01, E13, E12) << 9 | tri(E02, E03, E13) << 18 | tri(E02, E12, E23) << 27 |
                                    tri(E01, E12, E23) << 36 | tri(E01, E13, E23) << 45 | tri(E03, E13, E23) << 54;
constexpr unsigned long long TRI1 = tri(E02, E13, E12) << 18 | tri(E01, E23, E03) << 36 | tri(E01, E23, E02) << 45;      // m = 3, 5, 6

// the 7-bit mask of a vertex' active owned edges from its corner byte (a corner outside the grid repeats corner 0 there)
__device__ __forceinline__ unsigned edge_mask(unsigned corners) { return ((corners >> 1) ^ ((corners & 1u) ? 0x7fu : 0u)) & 0x7fu; }
__device__ __forceinline__ unsigned tet_mask(unsigned corners, int t) {
    return (corners & 1u) | ((corners >> tet_c1(t)) & 1u) << 1 | ((corners >> tet_c2(t)) & 1u) << 2 | ((corners >> 7) & 1u) << 3;
}
__device__ __forceinline__ unsigned tet_triangles(unsigned m) {
    const unsigned pc = __popc(m);
    return (pc == 0u || pc == 4u) ? 0u : (pc == 2u ? 2u : 1u);
}

struct GridIndex { unsigned ix, iy, iz; bool px, py, pz; size_t sy, sz; };
__device__ __forceinline__ GridIndex grid_index(const IsoArgs& a, unsigned v) {
    GridIndex q;
    const unsigned gx = (unsigned)a.g[0], gy = (unsigned)a.g[1], row = v / gx;
    q.ix = v - row * gx; q.iz = row / gy; q.iy = row - q.iz * gy;
    q.px = q.ix + 1 < gx; q.py = q.iy + 1 < gy; q.pz = q.iz + 1 < (unsigned)a.g[2];
    q.sy = gx; q.sz = (size_t)gx * gy;
    return q;
}

// ---- pass 1: classify, count, scan inside the block -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ISO_BLOCK) iso_count_kernel(const IsoArgs a, unsigned n) {
    __shared__ unsigned wave_sum[ISO_BLOCK / 64];
    const unsigned v = blockIdx.x * ISO_BLOCK + threadIdx.x;
    unsigned mine = 0;                                       // active owned edges | triangles of the cell << 16
    if (v < n) {
        const GridIndex q = grid_index(a, v);
        const float* p = a.value + v;
        const float f0 = p[0];
        unsigned corners = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool in_grid = (!(c & 1) || q.px) && (!(c & 2) || q.py) && (!(c & 4) || q.pz);
            const float f = in_grid ? p[(c & 1) + ((c >> 1) & 1) * q.sy + ((c >> 2) & 1) * q.sz] : f0;
            corners |= (f >= a.level ? 1u : 0u) << c;        // NaN: outside
        }
        a.ws.corners[v] = (uint8_t)corners;
        unsigned tris = 0;
        if (q.px && q.py && q.pz) {
#pragma unroll
            for (int t = 0; t < 6; ++t) tris += tet_triangles(tet_mask(corners, t));
        }
        mine = __popc(edge_mask(corners)) | tris << 16;
    }
    // exclusive scan over the block: inside each wave of 64 by shuffles, across the four waves through LDS
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned x = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d, 64);
        if (lane >= (unsigned)d) x += y;
    }
    if (lane == 63u) wave_sum[wave] = x;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (unsigned w = 0; w < ISO_BLOCK / 64; ++w) {
        const unsigned s = wave_sum[w];
        if (w < wave) before += s;
        total += s;
    }
    if (v < n) a.ws.offsets[v] = before + x - mine;          // halves cannot carry: <= 7 * 256 edges, <= 12 * 256 triangles per block
    if (threadIdx.x == 0) { a.ws.vsum[blockIdx.x] = total & 0xffffu; a.ws.tsum[blockIdx.x] = total >> 16; }
}

// ---- pass 2: the block sums -> 64-bit block bases and the totals; one workgroup, ISO_SCAN_CHUNK sums at a time ----------------------------------
__global__ void __launch_bounds__(ISO_SCAN_THREADS) iso_scan_kernel(const IsoWorkspace ws, unsigned nb, long long* totals) {
    __shared__ unsigned long long wave_sum[ISO_SCAN_THREADS / 64];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    long long v_carry = 0, t_carry = 0;                      // 7 edges x 2^30 vertices does not fit 32 bits
    for (unsigned c0 = 0; c0 < nb; c0 += ISO_SCAN_CHUNK) {   // (uniform over the workgroup)
        const unsigned i0 = c0 + threadIdx.x * 4;
        unsigned long long before_k[4], mine = 0;            // edges in the low word, triangles in the high one: <= 4096 * 3072 each per chunk
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
            before_k[k] = mine;
            if (i0 + k < nb) mine += (unsigned long long)ws.vsum[i0 + k] | (unsigned long long)ws.tsum[i0 + k] << 32;
        }
        unsigned long long x = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(x, d, 64);
            if (lane >= (unsigned)d) x += y;
        }
        if (lane == 63u) wave_sum[wave] = x;
        __syncthreads();
        unsigned long long before = 0, total = 0;
#pragma unroll
        for (unsigned w = 0; w < ISO_SCAN_THREADS / 64; ++w) {
            const unsigned long long s = wave_sum[w];
            if (w < wave) before += s;
            total += s;
        }
        __syncthreads();                                     // wave_sum is written again by the next chunk
        before += x - mine;
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
            if (i0 + k < nb) {
                const unsigned long long b = before + before_k[k];
                ws.vbase[i0 + k] = v_carry + (long long)(b & 0xffffffffull);
                ws.tbase[i0 + k] = t_carry + (long long)(b >> 32);
            }
        }
        v_carry += (long long)(total & 0xffffffffull);
        t_carry += (long long)(total >> 32);
    }
    if (threadIdx.x == 0) { totals[0] = v_carry; totals[1] = t_carry; }
}

// ---- pass 3: vertices (+ normals) of the active owned edges, triangles of the cell --------------------------------------------------------------
__device__ __forceinline__ long long vertex_index(const IsoWorkspace& ws, unsigned owner, unsigned slot) {
    return ws.vbase[owner / ISO_BLOCK] + (long long)(ws.offsets[owner] & 0xffffu) + __popc(edge_mask(ws.corners[owner]) & ((1u << slot) - 1u));
}

// grad value at grid vertex (i[0], i[1], i[2]): central differences, one-sided at the box faces; an axis with step 0 contributes 0
__device__ __forceinline__ void gradient_at(const IsoArgs& a, const double step[3], const unsigned i[3], const size_t stride[3], double g[3]) {
    const float* p = a.value + (i[0] + i[1] * stride[1] + i[2] * stride[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long below = i[c] > 0 ? -1 : 0, above = i[c] + 1 < (unsigned)a.g[c] ? 1 : 0;       // g >= 2: above - below >= 1
        g[c] = step[c] == 0.0 ? 0.0
                              : ((double)p[above * (long long)stride[c]] - (double)p[below * (long long)stride[c]]) / ((double)(above - below) * step[c]);
    }
}

__global__ void __launch_bounds__(ISO_BLOCK) iso_emit_kernel(const IsoArgs a, unsigned n) {
    const unsigned v = blockIdx.x * ISO_BLOCK + threadIdx.x;
    if (v >= n) return;
    const GridIndex q = grid_index(a, v);
    const unsigned corners = a.ws.corners[v], offsets = a.ws.offsets[v];
    // (the owned edges once more from the grid itself: a workspace no count pass filled cannot send a load outside the volume)
    unsigned owned = 0;
#pragma unroll
    for (unsigned s = 0; s < 7; ++s) {
        const unsigned d = s + 1;
        if ((!(d & 1u) || q.px) && (!(d & 2u) || q.py) && (!(d & 4u) || q.pz)) owned |= 1u << s;
    }
    const unsigned active = edge_mask(corners) & owned;
    if (active) {
        long long vi = a.ws.vbase[blockIdx.x] + (long long)(offsets & 0xffffu);
        const unsigned idx[3] = {q.ix, q.iy, q.iz};
        const size_t stride[3] = {1, q.sy, q.sz};
        double step[3], ga[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < 3; ++c) step[c] = a.g[c] > 1 ? ((double)a.hi[c] - (double)a.lo[c]) / (double)(a.g[c] - 1) : 0.0;
        const double fa = (double)a.value[v];
        if (a.normals) gradient_at(a, step, idx, stride, ga);
        for (unsigned rest = active; rest; rest &= rest - 1u) {              // ascending slots
            const unsigned d = (unsigned)__ffs((int)rest);                  // slot + 1: the direction bits
            const unsigned dir[3] = {d & 1u, (d >> 1) & 1u, (d >> 2) & 1u};
            if ((unsigned long long)vi < (unsigned long long)a.n_vertices) {
                const double fb = (double)a.value[v + dir[0] + dir[1] * q.sy + dir[2] * q.sz];
                double t = ((double)a.level - fa) / (fb - fa);
                t = isfinite(t) ? fmin(fmax(t, 0.0), 1.0) : 0.5;
                float* out = a.vertices + vi * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) out[c] = (float)((double)a.lo[c] + ((double)idx[c] + t * (double)dir[c]) * step[c]);
                if (a.normals) {
                    const unsigned other[3] = {idx[0] + dir[0], idx[1] + dir[1], idx[2] + dir[2]};
                    double gb[3], g[3];
                    gradient_at(a, step, other, stride, gb);
#pragma unroll
                    for (int c = 0; c < 3; ++c) g[c] = ga[c] + t * (gb[c] - ga[c]);
                    const double len = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
                    const bool ok = isfinite(len) && len > 0.0;
                    float* nrm = a.normals + vi * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) nrm[c] = ok ? (float)(-g[c] / len) : 0.0f;
                }
            }
            ++vi;
        }
    }
    if (!(q.px && q.py && q.pz) || corners == 0u || corners == 0xffu) return;
    long long ti = a.ws.tbase[blockIdx.x] + (long long)(offsets >> 16);
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const unsigned m = tet_mask(corners, t);
        if (m == 0u || m == 15u) continue;
        const unsigned row = m >= 8u ? 15u - m : m;
        const bool flip = (m >= 8u) != tet_odd(t);
        const unsigned cell_corner = 0u | tet_c1(t) << 4 | tet_c2(t) << 8 | 7u << 12;      // of local corners 0..3, four bits each
        const unsigned n_tri = tet_triangles(m);
        for (unsigned k = 0; k < n_tri; ++k) {
            const unsigned code = (unsigned)((k ? TRI1 : TRI0) >> (9u * (row - 1u))) & 0x1ffu;
            int at[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned e = (code >> (3 * j)) & 7u;
                const unsigned ca = (cell_corner >> (4u * ((EDGE_I >> (2u * e)) & 3u))) & 7u, cb = (cell_corner >> (4u * ((EDGE_J >> (2u * e)) & 3u))) & 7u;
                const unsigned owner = v + (ca & 1u) + ((ca >> 1) & 1u) * (unsigned)q.sy + ((ca >> 2) & 1u) * (unsigned)q.sz;       // a corner of a cell of the grid
                at[j] = (int)vertex_index(a.ws, owner, (ca ^ cb) - 1u);
            }
            if ((unsigned long long)ti < (unsigned long long)a.n_triangles) {
                int* f = a.faces + ti * 3;
                f[0] = at[0]; f[1] = flip ? at[2] : at[1]; f[2] = flip ? at[1] : at[2];
            }
            ++ti;
        }
    }
}

inline bool grid_ok(const IsoArgs& a, long long& n) {
    if (a.g[0] < 2 || a.g[1] < 2 || a.g[2] < 2) return false;
    n = (long long)a.g[0] * a.g[1] * a.g[2];
    return n <= ISO_MAX_VERTICES;
}

}  // namespace

hipError_t launch_isosurface_count(const IsoArgs& a, hipStream_t stream) {
    long long n = 0;
    if (!grid_ok(a, n) || !a.value || !a.totals || !a.ws.offsets) return hipErrorInvalidValue;
    const unsigned nb = (unsigned)((n + ISO_BLOCK - 1) / ISO_BLOCK);
    hipLaunchKernelGGL(iso_count_kernel, dim3(nb), dim3(ISO_BLOCK), 0, stream, a, (unsigned)n);
    hipLaunchKernelGGL(iso_scan_kernel, dim3(1), dim3(ISO_SCAN_THREADS), 0, stream, a.ws, nb, a.totals);
    return hipGetLastError();
}

hipError_t launch_isosurface_emit(const IsoArgs& a, hipStream_t stream) {
    long long n = 0;
    if (!grid_ok(a, n) || !a.value || !a.ws.offsets || a.n_vertices < 0 || a.n_triangles < 0) return hipErrorInvalidValue;
    if ((a.n_vertices > 0 && !a.vertices) || (a.n_triangles > 0 && !a.faces)) return hipErrorInvalidValue;
    const unsigned nb = (unsigned)((n + ISO_BLOCK - 1) / ISO_BLOCK);
    hipLaunchKernelGGL(iso_emit_kernel, dim3(nb), dim3(ISO_BLOCK), 0, stream, a, (unsigned)n);
    return hipGetLastError();
}

}  // namespace nrn
