// nrnerf_bend_inverse.h -- the ray bender walked backwards: for a canonical point c and the code l of a time step, the observed point x with
// bend(x, l) = x + m(x) o(x, l) [scale] = c (reference ray_bending.forward, run_nerf_helpers.py:507-577, read from right to left).
//
// There is no closed form; x is the fixed point of   x <- x - omega (bend(x, l) - c),   started at x0 (the canonical point itself, or the
// caller's guess).  One EVALUATION is the point-source fp32 bender of nrnerf_bend.h -- the same dense_b / Act / pack_act calls in the same order,
// the same __fmul_rn / __fadd_rn statements behind them -- so bend(x) computed here equals what nrnerf_query answers for x bit for bit, and
// the residual this kernel stores is the residual a caller measures.
//
// Per 32-point block (one wave; points of ONE row, so the latent code is wave-uniform):
//     evaluate            bent = bend(x)                               (offset MLP, rigidity MLP, cutoff / scaling knobs)
//     residual            r = max_c |bent_c - c_c|                     (a NaN component makes r NaN)
//     a lane is DONE      when r <= tol                                (NaN: never)
//     otherwise           x_c = x_c - omega (bent_c - c_c)             (not after evaluation number max_iters: the stored residual is the
//                                                                       stored point's)
// until every in-range lane of the block is done or max_iters evaluations were made.  A done lane is FROZEN BY A SELECT: the matrix
// instructions of the next evaluation run for all 64 lanes whatever the data is (the weight fragments are read with
// `asm volatile` LDS reads that do not name the exec mask), and the loop's exit is a wave-uniform vote.  A lane beyond the row's end clamps
// its index, counts as done and stores nothing.  A point's sequence is its own: it does not depend on which points share its block.
//
// Lane halves.  Lane l evaluates sample j = l & 31; the half h = l >> 5 selects which k-index of a first-layer slab the lane provides
// (`h ? v1 : v0`), so BOTH halves need x_j.  The D tile of v_mfma_f32_32x32x2_f32 puts row 8 (r / 4) + 4 h + (r % 4) of column j in register
// r of lane j + 32 h: rows 0..2 (the offsets; the logit is row 0 of its tile) are registers 0..2 of the LOWER half only -- the upper half's
// registers 0..2 are the padding rows 4..6.  The one-shot bender stores from h == 0 and is finished; here the updated x is copied from lane j
// to lane j + 32 (ds_bpermute_b32 with address 4 j) before the next evaluation.
//
// Shares.  Blocks take between one and max_iters evaluations, so the waves take the next block from a device counter as they finish one
// (one atomic per wave and block, lane 0, read with readfirstlane; issued before the iteration, read after it); without a counter every
// wave strides over the blocks.  The outputs are the same bits either way.
#pragma once
#include "nrnerf_bend.h"
#include "nrnerf_bend_inverse_args.h"

namespace nrn {

template <class A, int WAVES>
__global__ void __launch_bounds__(WAVES * 64, 4) bend_inverse_kernel(const BendInverseArgs a) {
    using P = PolF32;
    using PE = PolF32;
    static_assert(WAVES == 4, "fp32 mode: workgroups of four waves, four of them per CU");
    using PL = Plan<P, A, true, false, false>;                  // bender + rigidity layers only
    constexpr int KH = P::KH, SP = P::SP;
    static_assert(KH == 1, "one k-index per lane and slab");
    constexpr int NS_BIN = PL::NS_BIN, NS_RIN = PL::NS_RIN;
    constexpr int NB = PL::NT_BW * SP, NR = PL::NT_RW * SP;
    constexpr bool SPLIT = P::SPLIT;
    using ST = WResident<P, PL::NFRAGS>;

    extern __shared__ __attribute__((aligned(16))) char smem[];     // resident weights | bias table
    float* bias_lds = (float*)(smem + ST::BYTES);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const int j = lane & 31;

    ST st;
    st.init(a.wstream, smem, tid, WAVES * 64, lane);
    for (int i = tid; i < PL::NTILES * 32; i += WAVES * 64) bias_lds[i] = a.bias[i];
    __syncthreads();
    const BiasPtr bias_lane = bias_lane_ptr(bias_lds, h);

    const int n = a.n_per_row;
    const int bpr = (n + 31) >> 5;                 // 32-point blocks per row
    const unsigned nblocks = (unsigned)(a.n_rows * bpr);        // < 2^31 (launch_bend_inverse)
    typedef const __attribute__((address_space(4))) float* cfloat_p;
    const bool c_vec = a.stride == 4 && (((size_t)a.canonical & 15) == 0);
    const bool i_vec = a.stride == 4 && (((size_t)a.initial & 15) == 0);
    const float tol = a.tol, omega = a.omega;
    const int max_iters = a.max_iters;
    const unsigned lower_addr = (unsigned)j * 4u;  // ds_bpermute_b32: this lane reads lane j's register

    const bool dynamic = a.work_counter != nullptr;
    auto grab = [&]() -> unsigned {                // the next block of the counter (lane 0's value: read with readfirstlane)
        unsigned c = 0;
        if (lane == 0) c = __hip_atomic_fetch_add(a.work_counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return c;
    };
    const unsigned blk_step = (unsigned)gridDim.x * WAVES;
    unsigned blk = dynamic ? (unsigned)__builtin_amdgcn_readfirstlane(grab()) : (unsigned)blockIdx.x * WAVES + (unsigned)wave;
    // no barrier below: every wave works through its own blocks
    while (blk < nblocks) {
        unsigned pend = 0;
        if (dynamic) pend = grab();                // the block after this one: requested now, read behind the iteration
        const int row = __builtin_amdgcn_readfirstlane((int)(blk / (unsigned)bpr));
        const int k = ((int)blk - row * bpr) * 32 + j;
        const bool ok = k < n;
        const int kc = ok ? k : n - 1;             // (a lane beyond the row's end re-reads the row's last point and writes nothing)
        const size_t at = (size_t)row * n + kc;
        float c[3], p[3];
        {
            const float* cp = a.canonical + at * a.stride;
            if (c_vec) { const f32x4 q = *(const f32x4*)cp; c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; }
            else { c[0] = cp[0]; c[1] = cp[1]; c[2] = cp[2]; }
            p[0] = c[0]; p[1] = c[1]; p[2] = c[2];
            if (a.initial) {
                const float* ip = a.initial + at * a.stride;
                if (i_vec) { const f32x4 q = *(const f32x4*)ip; p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
                else { p[0] = ip[0]; p[1] = ip[1]; p[2] = ip[2]; }
            }
        }
        float lat[A::LAT];
        {
            cfloat_p lp = (cfloat_p)(a.latents + (size_t)row * a.lat_stride);
#pragma unroll
            for (int q = 0; q < A::LAT; ++q) lat[q] = lp[q];
        }
        auto binval = [&](auto idxc) -> float {
            constexpr int idx = decltype(idxc)::value;
            if constexpr (idx < 3) return p[idx];
            else if constexpr (idx < 8) return 0.0f;
            else if constexpr (idx - 8 < A::LAT) return lat[idx - 8];
            else return 0.0f;
        };
        auto rinval = [&](auto idxc) -> float {
            constexpr int idx = decltype(idxc)::value;
            if constexpr (idx < 3) return p[idx];
            else return 0.0f;
        };

        bool done = !(ok && h == 0);               // the upper half follows the lower one; it has no vote and no output
        float res = 0.0f;
        int evals = 0, n_it = 0;
        bool more;
        do {
            Act<PE, NS_BIN, SPLIT> bin;
            static_for<0, NS_BIN>([&](auto sc_) {
                constexpr int s = decltype(sc_)::value;
                const float v0 = binval(std::integral_constant<int, 2 * s>{});
                const float v1 = binval(std::integral_constant<int, 2 * s + 1>{});
                bin.template set<s, 0>(h ? v1 : v0);
            });
            // ---- offset MLP (run_nerf_helpers.py:525-541)
            Act<PE, NB, SPLIT> ba, bb;
            float off[3];
            dense_b<PE, SPLIT, PL, PL::L_BEND0, NS_BIN>(st, bias_lane, bin, [&](auto tc, const f32x16& acc) {
                pack_act<PE, decltype(tc)::value>(acc, ba);
            });
            static_for<1, A::BD - 1>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if constexpr (i % 2 == 1) {
                    dense_b<PE, SPLIT, PL, PL::L_BEND0 + i, NB>(st, bias_lane, ba, [&](auto tc, const f32x16& acc) {
                        pack_act<PE, decltype(tc)::value>(acc, bb);
                    });
                } else {
                    dense_b<PE, SPLIT, PL, PL::L_BEND0 + i, NB>(st, bias_lane, bb, [&](auto tc, const f32x16& acc) {
                        pack_act<PE, decltype(tc)::value>(acc, ba);
                    });
                }
            });
            auto take_off = [&](auto, const f32x16& acc) { off[0] = acc[0]; off[1] = acc[1]; off[2] = acc[2]; };
            if constexpr ((A::BD - 2) % 2 == 1) dense_b<PE, SPLIT, PL, PL::L_BEND0 + A::BD - 1, NB>(st, bias_lane, bb, take_off);
            else dense_b<PE, SPLIT, PL, PL::L_BEND0 + A::BD - 1, NB>(st, bias_lane, ba, take_off);
            // ---- rigidity MLP (run_nerf_helpers.py:545-561); input = xyz only
            Act<PE, NS_RIN, SPLIT> rin;
            static_for<0, NS_RIN>([&](auto sc_) {
                constexpr int s = decltype(sc_)::value;
                const float v0 = rinval(std::integral_constant<int, 2 * s>{});
                const float v1 = rinval(std::integral_constant<int, 2 * s + 1>{});
                rin.template set<s, 0>(h ? v1 : v0);
            });
            Act<PE, NR, SPLIT> ra, rb;
            float logit;
            dense_b<PE, SPLIT, PL, PL::L_RIG0, NS_RIN>(st, bias_lane, rin, [&](auto tc, const f32x16& acc) {
                pack_act<PE, decltype(tc)::value>(acc, ra);
            });
            static_for<1, A::RD - 1>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if constexpr (i % 2 == 1) {
                    dense_b<PE, SPLIT, PL, PL::L_RIG0 + i, NR>(st, bias_lane, ra, [&](auto tc, const f32x16& acc) {
                        pack_act<PE, decltype(tc)::value>(acc, rb);
                    });
                } else {
                    dense_b<PE, SPLIT, PL, PL::L_RIG0 + i, NR>(st, bias_lane, rb, [&](auto tc, const f32x16& acc) {
                        pack_act<PE, decltype(tc)::value>(acc, ra);
                    });
                }
            });
            auto take_logit = [&](auto, const f32x16& acc) { logit = acc[0]; };
            if constexpr ((A::RD - 2) % 2 == 1) dense_b<PE, SPLIT, PL, PL::L_RIG0 + A::RD - 1, NR>(st, bias_lane, rb, take_logit);
            else dense_b<PE, SPLIT, PL, PL::L_RIG0 + A::RD - 1, NR>(st, bias_lane, ra, take_logit);

            float rig_mask = (tanhf(logit) + 1.0f) / 2.0f;                                       // rnh:559-561
            if (a.knobs.has_cutoff && rig_mask <= a.knobs.cutoff) rig_mask = 0.0f;               // rnh:563-564
            float d[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                float mo = __fmul_rn(rig_mask, off[q]);                                          // rnh:567
                if (a.knobs.has_scaling) mo = __fmul_rn(mo, a.knobs.scaling);                    // rnh:568-569
                d[q] = __fsub_rn(__fadd_rn(p[q], mo), c[q]);                                     // rnh:570, minus the target
            }
            // max_c |d_c|, a NaN component winning (and then staying)
            float r = fabsf(d[0]);
#pragma unroll
            for (int q = 1; q < 3; ++q) {
                const float v = fabsf(d[q]);
                r = (v > r || v != v) ? v : r;
            }
            ++evals;
            if (!done) { res = r; n_it = evals; }              // (selects) the evaluation of a lane that was still iterating
            done = done || (r <= tol);                         // NaN: not done
            const bool last = evals >= max_iters;              // wave-uniform
            const bool step = !done && !last;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                float od = __fmul_rn(omega, d[q]);
                asm volatile("" : "+v"(od));                   // two roundings, as written: hipcc otherwise fuses the product into the difference
                const float xn = __fsub_rn(p[q], od);
                p[q] = step ? xn : p[q];
            }
            // lane j's point to lane j + 32 (and to itself); the counted LDS waits of the next evaluation start from an empty queue
            asm volatile("ds_bpermute_b32 %0, %3, %0\n\tds_bpermute_b32 %1, %3, %1\n\tds_bpermute_b32 %2, %3, %2\n\ts_waitcnt lgkmcnt(0)"
                         : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]) : "v"(lower_addr));
            more = !last && __builtin_amdgcn_ballot_w64(!done) != 0ull;
        } while (more);

        if (ok && h == 0) {
            a.observed[at * 3] = p[0]; a.observed[at * 3 + 1] = p[1]; a.observed[at * 3 + 2] = p[2];
            if (a.residual) a.residual[at] = res;
            if (a.iterations) a.iterations[at] = n_it;
        }
        blk = dynamic ? (unsigned)__builtin_amdgcn_readfirstlane(pend) : blk + blk_step;
    }
}

template <class A, int WAVES>
static hipError_t launch_bend_inverse_one(const BendInverseArgs& a, int num_cus, hipStream_t stream) {
    using PL = Plan<PolF32, A, true, false, false>;
    const size_t lds = (size_t)PL::NFRAGS * PolF32::FRAG_BYTES + (size_t)PL::NTILES * 32 * sizeof(float);
    auto kern = bend_inverse_kernel<A, WAVES>;
    static bool attr_set[64] = {};       // function attributes are per device (idempotent; racing threads set the same value)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    const long long nblocks = (long long)a.n_rows * ((a.n_per_row + 31) / 32);
    if (nblocks >= (1ll << 31)) return hipErrorInvalidValue;
    const long long want = (nblocks + WAVES - 1) / WAVES;
    if (want <= 0) return hipSuccess;
    // persistent: 20-28 KiB of resident weights and < 128 VGPRs per lane, four workgroups per CU (as the one-shot fp32 bender)
    const long long resident = 4ll * num_cus;
    const int grid = (int)(want < resident ? want : resident);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVES * 64), lds, stream, a);
    return hipGetLastError();
}

}  // namespace nrn
