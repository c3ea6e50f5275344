// nrnerf_isosurface.h -- launch interface of nrnerf_isosurface.hip: an iso-surface mesh of a float32 volume on a regular grid (the layout of
// sample_grid's "sigma": value[iz][iy][ix]) by MARCHING TETRAHEDRA over the Kuhn triangulation of each cell.  No case table beyond the
// sixteen cases of one tetrahedron (below), no ambiguous configuration: the mesh is closed away from the box faces and consistently oriented
// by construction.  Deterministic: every output index comes from an exclusive scan, none from an atomically claimed offset.
//
// DEFINITIONS (DESIGN.md section 3.11 repeats them; tests/mesh_reference.py restates them in numpy float64)
//   inside      a grid vertex is inside iff value >= level.  NaN is outside.
//   cell        minimum corner (ix, iy, iz), ix < gx - 1, iy < gy - 1, iz < gz - 1; its corners are coded c = dx + 2 dy + 4 dz.
//   tetrahedra  six per cell, one per permutation (p1, p2, p3) of the axes in lexicographic order
//                   0 xyz   1 xzy   2 yxz   3 yzx   4 zxy   5 zyx
//               with LOCAL corners 0..3 = cell corners 0, e_p1, e_p1 + e_p2, 7:
//                   0: 0 1 3 7   1: 0 1 5 7   2: 0 2 3 7   3: 0 2 6 7   4: 0 4 5 7   5: 0 4 6 7
//               Tetrahedra 0, 3, 4 (even permutations) are positively oriented (det [v1 - v0, v2 - v0, v3 - v0] > 0), 1, 2, 5 negatively.
//   edge        every tetrahedron edge joins cell corners a, b with a a subset of b (as bit sets).  Its OWNER is the grid vertex cell + a, its
//               SLOT (b & ~a) - 1 in 0..6: +x, +y, +xy, +z, +xz, +yz, +xyz.  The face diagonals follow from the same rule in every cell, so
//               neighbouring cells agree on them.  A grid vertex owns the edge of slot s iff the vertex at its other end is in the grid.
//   active      an edge is active iff exactly one of its ends is inside; it carries ONE mesh vertex at t = (level - f_a) / (f_b - f_a), a the
//               owner end: computed in double from the two fp32 values, a non-finite t becomes 0.5, else it is clamped to [0, 1].  World
//               position per axis: lo + (i + t * d) * step, d in {0, 1} the edge's direction bit, step = g > 1 ? (hi - lo) / (g - 1) : 0 exactly
//               as grid_points_kernel (nrnerf_field.hip) computes it; evaluated in double, rounded to fp32 once.
//   vertices    ascending (owner linear index (iz * gy + iy) * gx + ix, slot).
//   triangles   ascending (cell linear index -- that of its minimum corner --, tetrahedron 0..5, triangle 0..1).
//   THE SIXTEEN CASES.  mask m = sum of 2^k over the INSIDE local corners k; "ij" is the mesh vertex on the edge of local corners i, j.
//               For a positively oriented tetrahedron:
//                   m =  0  -                                  m = 15  -
//                   m =  1  (01 02 03)                         m = 14  (01 03 02)
//                   m =  2  (01 13 12)                         m = 13  (01 12 13)
//                   m =  3  (02 03 13) (02 13 12)              m = 12  (02 13 03) (02 12 13)
//                   m =  4  (02 12 23)                         m = 11  (02 23 12)
//                   m =  5  (01 12 23) (01 23 03)              m = 10  (01 23 12) (01 03 23)
//                   m =  6  (01 13 23) (01 23 02)              m =  9  (01 23 13) (01 02 23)
//                   m =  7  (03 13 23)                         m =  8  (03 23 13)
//               (the right column is the left one's row 15 - m with the last two vertices of every triangle exchanged).  For a negatively
//               oriented tetrahedron (1, 2, 5) the last two vertices of every triangle are exchanged once more.  One or three inside corners
//               give one triangle, two give a quad as two triangles sharing the diagonal written first and third.
//   orientation every triangle's geometric normal (v1 - v0) x (v2 - v0) points from inside to outside: for a density, towards lower density.
//   normals     (optional) -grad value: central differences at the two ends of the edge, one-sided at the box faces, each divided by its axis'
//               step (an axis with step == 0 contributes 0), interpolated with t, normalised; a zero or non-finite gradient gives (0, 0, 0).
//   degenerate  (zero-area) triangles are KEPT: they arise when a value equals the level exactly, and dropping them would open the mesh.
//
// PASSES.  count (one thread per grid vertex, blocks of ISO_BLOCK consecutive linear indices: x runs fastest, loads coalesce): the eight
// corner values -> one byte of inside bits per vertex (a corner outside the grid repeats corner 0, so its edge is never active), the number of
// active owned edges and of the cell's triangles, their exclusive scan inside the block (two 16-bit halves of one word per vertex) and the
// block's sums.  scan (one workgroup): the block sums in chunks of ISO_SCAN_CHUNK, carried in 64 bits -> 64-bit block bases and the totals.
// emit (one thread per grid vertex): the vertices (+ normals) of its active owned edges and the triangles of its cell; the index of an edge's
// vertex is its owner's base + popcount(owner's edge mask & ((1 << slot) - 1)).  Every store is guarded by its capacity.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrn {

constexpr int ISO_BLOCK = 256;                 // grid vertices per block of the count / emit passes
constexpr int ISO_SCAN_THREADS = 1024;         // the one workgroup of the scan pass ...
constexpr int ISO_SCAN_CHUNK = 4 * ISO_SCAN_THREADS;   // ... and the block sums it takes at once
constexpr long long ISO_MAX_VERTICES = 1ll << 30;      // grid vertices: linear indices stay 32-bit

// the workspace, carved in this order, every part starting on a 256-byte boundary (n = gx gy gz grid vertices, nb = ceil(n / ISO_BLOCK)):
//   offsets  uint32 [n]    low half: active owned edges before this vertex in its block, high half: triangles before its cell in its block
//   vsum     uint32 [nb]   active edges of the block          tsum   uint32 [nb]   triangles of the block
//   vbase    int64  [nb]   mesh vertices before the block     tbase  int64  [nb]   triangles before the block
//   corners  uint8  [n]    inside bits of the eight corners seen from this vertex
struct IsoWorkspace {
    uint32_t* offsets; uint32_t* vsum; uint32_t* tsum; long long* vbase; long long* tbase; uint8_t* corners;
    size_t bytes;
};
inline size_t iso_align(size_t v) { return (v + 255) & ~(size_t)255; }
inline IsoWorkspace iso_carve(void* base, long long n) {
    const size_t nb = (size_t)((n + ISO_BLOCK - 1) / ISO_BLOCK);
    char* p = (char*)base;
    size_t o = 0;
    IsoWorkspace w{};
    w.offsets = (uint32_t*)(p + o); o += iso_align((size_t)n * 4);
    w.vsum = (uint32_t*)(p + o); o += iso_align(nb * 4);
    w.tsum = (uint32_t*)(p + o); o += iso_align(nb * 4);
    w.vbase = (long long*)(p + o); o += iso_align(nb * 8);
    w.tbase = (long long*)(p + o); o += iso_align(nb * 8);
    w.corners = (uint8_t*)(p + o); o += iso_align((size_t)n);
    w.bytes = o;
    return w;
}

struct IsoArgs {
    const float* value;                  // [gz, gy, gx]
    int g[3];                            // gx, gy, gz, each >= 2, gx gy gz <= ISO_MAX_VERTICES
    float lo[3], hi[3], level;
    IsoWorkspace ws;
    long long* totals;                   // count: {vertices, triangles}
    float* vertices; float* normals;     // emit: [n_vertices, 3]; normals may be nullptr
    int* faces;                          // emit: [n_triangles, 3]
    long long n_vertices, n_triangles;   // capacities: nothing is stored at or beyond them
};
hipError_t launch_isosurface_count(const IsoArgs& a, hipStream_t stream);      // passes 1 and 2
hipError_t launch_isosurface_emit(const IsoArgs& a, hipStream_t stream);       // pass 3, from the workspace a count left

}  // namespace nrn
