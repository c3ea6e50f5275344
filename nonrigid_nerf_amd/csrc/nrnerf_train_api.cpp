// nrnerf_train_api.cpp -- the training entry points of the C ABI (include/nrnerf.h): the optimiser step, the loss, the trunk's and the
// bender's forward / backward-data / weight-gradient calls, compositing forward / backward and the small reductions between them.  Each
// is "validate, build the launcher's arguments, run" (on_owner_of / on_model_device, nrnerf_model.h); no entry point keeps state.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "nrnerf_model.h"
#include "nrnerf_aux.h"
#include "nrnerf_x16_api.h"
#include "nrnerf_loss.h"
#include "nrnerf_optim.h"
#include "nrnerf_gen_train.h"
#include "nrnerf_gx16_bwd_api.h"
#include "nrnerf_plan.h"

using namespace nrn;

#ifndef NRN_WGRAD_SYNC_DEFAULT
// pairs of blocks between workgroup barriers in trunk_wgrad (WgradArgs::sync_every; env NRNERF_WGRAD_SYNC, 0 = never).  Measured
// at 16 384 rays (tools/experiments/wgrad_sync_sweep.sh): never 3.30 ms per launch, every 2 pairs 2.76, 8: 2.54, 32: 2.55, 128: 2.82,
// 512: 3.09 -- the waves that share a fragment stay within L2's reach of each other, the barrier itself costs nothing because
// the loads already requested stay in flight across it.
#define NRN_WGRAD_SYNC_DEFAULT 16
#endif

namespace {

bool is_f32(const nrnerf_model* m) { return m->precision == NRNERF_PREC_F32; }

// ---- which compiled training kernels a handle runs ------------------------------------------------------------------
// the trunk's: by family (width 128 / width 256 + view-dependent head / width 256) and element type
enum TrunkFamily { TRUNK_NARROW, TRUNK_VIEWS, TRUNK_PLAIN };
TrunkFamily trunk_family(const nrnerf_model* m) { return m->arch_id == 5 ? TRUNK_NARROW : (m->views ? TRUNK_VIEWS : TRUNK_PLAIN); }
struct TrunkKernels {
    hipError_t (*fwd)(const TrunkArgs&, int num_cus, hipStream_t);
    hipError_t (*bwd)(const TrunkArgs&, int num_cus, hipStream_t);
    hipError_t (*wgrad)(const WgradArgs&, hipStream_t);
};
#define NRN_TRUNK_KERNELS(tag) TrunkKernels{launch_trunk_fwd_train_##tag, launch_trunk_bwd_##tag, launch_trunk_wgrad_##tag}
const TrunkKernels TRUNK_KERNELS[3][2] = {        // [family][bf16]
    {NRN_TRUNK_KERNELS(f32_a5), NRN_TRUNK_KERNELS(bf16_a5)}, {NRN_TRUNK_KERNELS(f32_views), NRN_TRUNK_KERNELS(bf16_views)}, {NRN_TRUNK_KERNELS(f32), NRN_TRUNK_KERNELS(bf16)}};
const TrunkKernels& trunk_kernels(const nrnerf_model* m) { return TRUNK_KERNELS[trunk_family(m)][is_f32(m) ? 0 : 1]; }

// the bender's: by compiled bender shape (bender_arch_of); the element type of the saved arrays is an argument of the launch
using BendTrainLaunch = hipError_t (*)(const BendTrainArgs&, int num_cus, hipStream_t, bool bf16_arrays);
using BendDivLaunch = hipError_t (*)(const BendDivArgs&, int num_cus, hipStream_t, bool bf16_arrays);
struct BenderKernels { BendTrainLaunch fwd_train, bwd; BendDivLaunch div_fwd, div_bwd; };
#define NRN_BENDER_KERNELS(tag) BenderKernels{launch_bend_fwd_train_##tag, launch_bend_bwd_##tag, launch_bend_div_fwd_##tag, launch_bend_div_bwd_##tag}
const BenderKernels BENDER_KERNELS[2] = {NRN_BENDER_KERNELS(a0), NRN_BENDER_KERNELS(a1)};
const BenderKernels& bender_kernels(const nrnerf_model* m) { return BENDER_KERNELS[bender_arch_of(m) == 0 ? 0 : 1]; }

// the rigidity knobs of a training call (nrnerf_bender_args / nrnerf_divergence_args: has_rigidity_cutoff and the fields behind it)
template <class ARGS> Knobs rigidity_knobs(const ARGS& a) {
    Knobs k{};
    k.has_cutoff = a.has_rigidity_cutoff; k.cutoff = a.rigidity_cutoff;
    k.has_scaling = a.has_test_time_scaling; k.scaling = a.test_time_scaling;
    return k;
}

// ---- weight gradients of the bender's two MLPs: one chain of BendWgradJobs per MLP -------------------------------------
struct BendChain {
    const void *dz, *acts;            // [depth-1][M][width] gradients wrt the hidden pre-activations / hidden activations, fp32 or bf16 (`b16`)
    const void *dtz, *tacts;          // the same of the tangent chain (divergence regulariser), or nullptr
    int depth, width;
    const float *dz_out, *dtz_out;    // [M][4] fp32, at the chain's column: gradient wrt the MLP's outputs (/ their tangents, or nullptr)
    int n_out;                        // columns of it that are this MLP's
};
// the first layer's input: [M][ldx], its first g columns -- x == nullptr: the row [point, latent code] formed from the ray records --, and
// the tangent input that goes with it (or nullptr)
struct BendInput { const void* x; int ldx, g; const void* x2; };
// appends the chain's jobs: the first layer once per part of its input, hidden layers 1 .. depth-2, the output layer
void add_bend_chain(BendWgradArgs& w, const BendChain& c, std::initializer_list<BendInput> first, size_t M, int b16) {
    const size_t esz = b16 ? 2 : 4, layer = M * (size_t)c.width;
    auto at = [&](const void* base, size_t elems) { return base ? (const void*)((const char*)base + elems * esz) : nullptr; };
    for (const BendInput& in : first)
        w.job[w.njobs++] = BendWgradJob{c.dz, c.width, c.width, in.x, in.ldx, in.g, in.x2 ? c.dtz : nullptr, in.x2, b16, 0};
    for (int i = 1; i <= c.depth - 2; ++i)
        w.job[w.njobs++] = BendWgradJob{at(c.dz, i * layer), c.width, c.width, at(c.acts, (i - 1) * layer), c.width, c.width,
                                        at(c.dtz, i * layer), at(c.tacts, (i - 1) * layer), b16, b16};
    w.job[w.njobs++] = BendWgradJob{c.dz_out, 4, c.n_out, at(c.acts, (c.depth - 2) * layer), c.width, c.width,
                                    c.dtz_out, at(c.tacts, (c.depth - 2) * layer), 0, b16};
}
int bender_depth(const nrnerf_model* m) { return bender_arch_of(m) == 0 ? ArchDefault::BD : ArchDeepBend::BD; }
// 32-bit offsets in bend_wgrad16: M samples of 64 fp32 columns must stay below 4 GiB
bool bend_wgrad_offsets_fit(const nrnerf_model* m, size_t M) { return is_f32(m) || M * 64 * 4 < 0xffffff00ull; }
int run_bend_wgrad(const nrnerf_model* m, const BendWgradArgs& w, hipStream_t stream) { return status_of(launch_bend_wgrad(w, stream, !is_f32(m))); }

// ---- the generic trunk's images: the layer program and the width-class image of a pass, forward or backward-data ------------------
struct GenericTrunkImages { const ImageDev &program, &wclass; };
GenericTrunkImages generic_trunk_images(const nrnerf_model* m, bool fine, bool backward) {
    if (backward) return fine ? GenericTrunkImages{m->gen_fine_bwd, m->gx_fine_bwd} : GenericTrunkImages{m->gen_coarse_bwd, m->gx_coarse_bwd};
    return fine ? GenericTrunkImages{m->gen_fine, m->gx_fine} : GenericTrunkImages{m->gen_coarse, m->gx_coarse};
}

int cus_of_device(int dev) {
    static int cache[64] = {};
    if (dev >= 0 && dev < 64 && cache[dev] > 0) return cache[dev];
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    if (dev >= 0 && dev < 64) cache[dev] = prop.multiProcessorCount;
    return prop.multiProcessorCount;
}
// panels of all jobs and the number of sample chunks (= records of partial sums) a call is cut into: ~2 workgroups per CU, >= 1024 samples each
bool tn_plan(const nrnerf_tn_args* a, int num_cus, long long& n_sub, int& kch) {
    if (!a || a->struct_size != sizeof(nrnerf_tn_args) || a->n_jobs < 1 || !a->jobs || a->n_rows < 1 || a->out_floats < 1) return false;
    n_sub = 0;
    for (int j = 0; j < a->n_jobs; ++j) {
        const nrnerf_tn_job& jb = a->jobs[j];
        if (!jb.a || !jb.b || jb.wo < 1 || jb.wi < 1 || jb.lda < jb.wo || jb.ldb < jb.wi || jb.ldo < jb.wi || jb.out_offset < 0) return false;
        if (jb.out_offset + (long long)(jb.wo - 1) * jb.ldo + jb.wi > a->out_floats) return false;
        if (jb.bias_offset >= 0 && jb.bias_offset + jb.wo > a->out_floats) return false;
        n_sub += (long long)((jb.wo + 255) / 256) * ((jb.wi + 255) / 256);
    }
    long long k = (2ll * (num_cus > 0 ? num_cus : 256) + n_sub - 1) / n_sub;          // (one workgroup per CU at a time: two rounds even out the jobs' sizes)
    const long long by_rows = a->n_rows / 1024 > 1 ? a->n_rows / 1024 : 1;
    if (k > by_rows) k = by_rows;
    if (k > 64) k = 64;
    if (k < 1) k = 1;
    kch = (int)k;
    return true;
}

}  // namespace

extern "C" {

// ---- optimiser step, products over the samples, encodings -------------------------------------------------------------------------
int nrnerf_adam_step(nrnerf_model* m, const nrnerf_adam_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_adam_args) || a->n_segments < 0 || a->n_segments > NRNERF_ADAM_MAX_SEGMENTS || !a->step) return NRNERF_ERR_INVALID;
    if (!(a->beta1 >= 0.0f && a->beta1 < 1.0f && a->beta2 >= 0.0f && a->beta2 < 1.0f && a->eps >= 0.0f)) return NRNERF_ERR_INVALID;
    const bool repack = m && a->flat_params;
    if (repack && a->n_floats != m->flat_floats) return NRNERF_ERR_INVALID;
    if (!m && !a->barrier) return NRNERF_ERR_INVALID;
    AdamKernelArgs k{};
    for (int i = 0; i < a->n_segments; ++i) {
        const nrnerf_adam_segment& s = a->segments[i];
        if (s.n > 0 && (!s.param || !s.grad || !s.exp_avg || !s.exp_avg_sq)) return NRNERF_ERR_INVALID;
        k.seg[i] = AdamSegment{s.param, s.grad, s.exp_avg, s.exp_avg_sq, (unsigned long long)s.n};
        k.gran0[i + 1] = k.gran0[i] + (long long)((s.n + 3) / 4);
    }
    for (int i = a->n_segments; i < ADAM_MAX_SEGMENTS; ++i) k.gran0[i + 1] = k.gran0[i];
    k.n_segments = a->n_segments;
    k.lr = a->lr; k.beta1 = a->beta1; k.beta2 = a->beta2; k.eps = a->eps; k.lr_device = a->lr_device; k.step = a->step;
    int dev = 0, num_cus = 0;
    if (m) { dev = m->device; num_cus = m->num_cus; k.barrier = m->adam_barrier; }
    else {          // without a model: the device that owns the step counter, the caller's barrier words
        if (device_of(a->step, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return NRNERF_ERR_HIP;
        num_cus = prop.multiProcessorCount; k.barrier = a->barrier;
    }
    if (!k.barrier) return NRNERF_ERR_INVALID;
    return on_device(dev, [&] {
        const hipStream_t stream = (hipStream_t)hip_stream;
        if (launch_adam(k, num_cus, stream) != hipSuccess) return (int)NRNERF_ERR_HIP;
        // ... and every packed image from the updated parameters, right behind it on the same stream
        return repack ? repack_batches(m, a->flat_params, stream) : (int)NRNERF_OK;
    });
} NRN_CATCH

size_t nrnerf_tn_workspace_bytes(const nrnerf_tn_args* a) {
    long long n_sub; int kch;
    int dev = 0;
    if (!a || !a->out || device_of(a->out, dev) != NRNERF_OK) { (void)hipGetDevice(&dev); }
    if (!tn_plan(a, cus_of_device(dev), n_sub, kch)) return 0;
    return (size_t)kch * (size_t)a->out_floats * sizeof(float);
}

int nrnerf_tn_products(const nrnerf_tn_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_tn_args) || !a->out || !a->workspace) return NRNERF_ERR_INVALID;
    int dev = 0;
    if (device_of(a->out, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    long long n_sub; int kch;
    if (!tn_plan(a, cus_of_device(dev), n_sub, kch)) return NRNERF_ERR_INVALID;
    if (a->workspace_bytes < (size_t)kch * (size_t)a->out_floats * sizeof(float) || ((uintptr_t)a->workspace & 15)) return NRNERF_ERR_WORKSPACE;
    return on_device(dev, [&] {
        const hipStream_t stream = (hipStream_t)hip_stream;
        float* parts = (float*)a->workspace;
        if (launch_tn_clear(parts, a->out_floats, kch, stream) != hipSuccess) return (int)NRNERF_ERR_HIP;
        TnKernelArgs k{};
        k.kch = kch; k.n_rows = a->n_rows; k.total = a->out_floats; k.partials = parts;
        auto flush = [&]() -> int {           // (a misaligned operand is the caller's: status_of_checked_launch)
            if (k.n_sub == 0) return NRNERF_OK;
            const hipError_t rc = launch_tn_products(k, a->is_bf16 == 0, stream);
            k.n_sub = 0;
            return status_of_checked_launch(rc);
        };
        for (int j = 0; j < a->n_jobs; ++j) {
            const nrnerf_tn_job& jb = a->jobs[j];
            for (int o0 = 0; o0 < jb.wo; o0 += 256)
                for (int k0 = 0; k0 < jb.wi; k0 += 256) {
                    if (k.n_sub == TN_MAX_SUBJOBS)
                        if (const int rc = flush(); rc != NRNERF_OK) return rc;
                    k.sub[k.n_sub++] = TnSubJob{jb.a, jb.b, jb.lda, jb.ldb, jb.wo, jb.wi, o0, k0, jb.ldo, (long long)jb.out_offset, (long long)jb.bias_offset};
                }
        }
        if (const int rc = flush(); rc != NRNERF_OK) return rc;
        return status_of(launch_tn_reduce(parts, a->out_floats, kch, a->out, stream));
    });
} NRN_CATCH

}  // extern "C"
namespace {
int encoding_call(const nrnerf_encoding_args* a, bool backward, void* hip_stream) {
    if (!a || a->struct_size != sizeof(nrnerf_encoding_args) || a->n_rows < 0 || !a->src) return NRNERF_ERR_INVALID;
    if (a->n_rows == 0) return NRNERF_OK;
    const EncodingArgs e{a->src, a->src_stride, (long long)a->n_rows, a->n_freqs, a->enc, a->enc_cols, a->enc_is_bf16, a->codes, a->n_lat, a->rows_per_code,
                         a->d_enc0, a->d_enc1, a->d_enc_stride, a->d_src, a->d_src_stride};
    return on_owner_of(a->src, [&] { return status_of_checked_launch(launch_encoding_rows(e, backward, (hipStream_t)hip_stream)); });
}
}  // namespace
extern "C" {
int nrnerf_encoding_forward(const nrnerf_encoding_args* a, void* hip_stream) try { return encoding_call(a, false, hip_stream); } NRN_CATCH
int nrnerf_encoding_backward(const nrnerf_encoding_args* a, void* hip_stream) try { return encoding_call(a, true, hip_stream); } NRN_CATCH
}  // extern "C"

// ---- the trunk of a non-compiled architecture ------------------------------------------------------------------------------------
namespace {
int generic_trunk_call(const nrnerf_model* m, const nrnerf_generic_trunk_args* a, bool backward, void* hip_stream) {
    if (!m || !a || a->struct_size != sizeof(nrnerf_generic_trunk_args)) return NRNERF_ERR_INVALID;
    if (!m->generic || !m->gen_train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->which < 0 || a->which > 1 || a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || !a->acts) return NRNERF_ERR_INVALID;
    const bool fine = a->which == 1 && !m->fine_is_coarse;
    const GenTrainNet& tn = m->gen_tn[fine ? 1 : 0];
    const GenericTrunkImages im = generic_trunk_images(m, fine, backward);
    if (!backward && (!a->pts4 || !a->raw4 || (tn.views && !a->dirs) || (tn.lat > 0 && !a->latents))) return NRNERF_ERR_INVALID;
    // the epilogue writes channels 0..3 of a row of `raw`, and channel 4 when raw_ch > 4: the row must hold them and the network must have them
    if (!backward && a->raw && (a->raw_ch < 4 || a->raw_ch > im.program.output_ch)) return NRNERF_ERR_INVALID;
    if (backward && (!a->d_raw4 || !a->d_pre || !a->d_enc0 || (tn.skip && !a->d_enc1) || (tn.views && !a->d_encv))) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    return on_model_device(m, [&] {
        const hipStream_t stream = (hipStream_t)hip_stream;
        const long long M = (long long)a->n_rays * a->n_samples;
        GenArgs g = im.program.prog;
        g.wstream = im.program.stream; g.bias = im.program.bias;
        g.n_rays = a->n_rays; g.S = a->n_samples;
        g.save_stride = M * tn.W; g.save_w = tn.W;
        const GxMeta& gm = im.wclass.gx;
        // the width-class 16x16x32 kernels take a trunk with a plain head and no latent input columns (32-bit sample rows and block indices)
        const bool gx_fits = im.wclass.stream && !tn.views && tn.lat == 0 && M < (1ll << 32) && (long long)a->n_rays * ((a->n_samples + 15) / 16) < (1ll << 31);
        if (!backward) {
            // the forward pass on the width-class 16x16x32 kernel (nrnerf_gx16.h, SAVE: activations written from the registers) when it has this
            // trunk: bf16, plain head, no latent input columns; 0.55 of the matrix pipe's peak instead of the run-time-parameterised kernel's 0.07
            if (gx_fits && m->precision == NRNERF_PREC_BF16 && tn.W % 4 == 0) {
                GxArgs x{};
                x.pts4 = a->pts4; x.raw4 = a->raw4; x.raw_out = a->raw; x.raw_ch = a->raw ? a->raw_ch : 4;
                x.n_rays = a->n_rays; x.S = a->n_samples; x.wstream = im.wclass.stream; x.bias = im.wclass.bias;
                x.depth = gm.depth; x.skip = gm.skip; x.L = gm.L; x.n_bias_tiles = gm.n_bias_tiles; x.LV = gm.LV;
                x.save = a->acts; x.save_stride = M * tn.W; x.save_w = tn.W; x.relu_bits = a->relu_bits;
                return status_of(launch_gx16(m->precision, gm.wc, false, x, m->num_cus, stream));
            }
            g.mode = 1;
            g.rays = a->pts4; g.ray_stride = 0;                                              // (points are handed in: the ray record is never read)
            g.latents = tn.lat > 0 ? a->latents : nullptr; g.lat_stride = tn.lat;
            g.z = nullptr; g.lindisp = 0; g.pts4 = a->pts4; g.dirs_from_pts = 0; g.dirs = tn.views ? a->dirs : nullptr;
            g.raw4 = a->raw4; g.raw_out = a->raw; g.raw_ch = a->raw ? a->raw_ch : 4; g.bent4 = nullptr;
            g.save = a->acts; g.mask = nullptr;
        } else {
            // backward-data on the width-class kernel's dataflow (nrnerf_gx16_bwd.h) when the forward call left its relu bits
            if (gx_fits && a->relu_bits) {
                GxBwdArgs b{};
                b.d_raw4 = a->d_raw4; b.relu_bits = a->relu_bits; b.d_pre = a->d_pre; b.save_stride = M * tn.W; b.save_w = tn.W;
                b.d_enc0 = a->d_enc0; b.d_enc1 = a->d_enc1; b.enc_w = tn.in_w;
                b.n_rays = a->n_rays; b.S = a->n_samples; b.wstream = im.wclass.stream; b.bias = im.wclass.bias;
                b.depth = gm.depth; b.skip = gm.skip; b.L = gm.L; b.n_bias_tiles = gm.n_bias_tiles;
                return status_of(launch_gx16_bwd(gm.wc, b, m->num_cus, stream));
            }
            g.mode = 2;
            g.rays = a->d_raw4; g.ray_stride = 0;
            g.draw = a->d_raw4; g.draw_ch = 4; g.draw_col = tn.draw_col;
            g.mask = a->acts; g.save = a->d_pre;
            g.gout[0] = a->d_enc0; g.gout[1] = a->d_enc1; g.gout[2] = a->d_encv; g.gout_w = tn.in_w; g.gout_w2 = tn.dv;
        }
        return status_of(launch_generic_train(m->precision, g, m->num_cus, stream));
    });
}
}  // namespace
extern "C" {
int nrnerf_generic_trunk_forward(const nrnerf_model* m, const nrnerf_generic_trunk_args* a, void* hip_stream) try { return generic_trunk_call(m, a, false, hip_stream); } NRN_CATCH
int nrnerf_generic_trunk_backward(const nrnerf_model* m, const nrnerf_generic_trunk_args* a, void* hip_stream) try { return generic_trunk_call(m, a, true, hip_stream); } NRN_CATCH
int nrnerf_model_trains_generic(const nrnerf_model* m) { return m ? ((m->generic && m->gen_train_ok) ? 1 : 0) : NRNERF_ERR_INVALID; }
size_t nrnerf_generic_trunk_bits_bytes(const nrnerf_model* m, int32_t which, int32_t n_rays, int32_t n_samples) {
    if (!m || !m->generic || which < 0 || which > 1 || n_rays < 1 || n_samples < 1) return 0;
    const ImageDev& gxb = generic_trunk_images(m, which == 1 && !m->fine_is_coarse, true).wclass;
    if (!gxb.stream) return 0;
    return (size_t)gxb.gx.depth * (size_t)n_rays * (size_t)((n_samples + 15) / 16) * 64 * (size_t)gx16_bits_bytes_per_lane(gxb.gx.wc);
}
}  // extern "C"

// ---- the loss and the small kernels between the big ones: no model, the device is the one that owns an output ---------------------
namespace {
int loss_call(const nrnerf_loss_args* a, bool backward, void* hip_stream) {
    if (!a || a->struct_size != sizeof(nrnerf_loss_args) || a->n_rays < 0 || a->n_samples < 0 || !a->rgb_map || !a->target) return NRNERF_ERR_INVALID;
    if (a->weights && (!a->offsets || !a->rigidity)) return NRNERF_ERR_INVALID;
    if (a->divergence && !a->alpha) return NRNERF_ERR_INVALID;
    if ((a->weights || a->divergence) && a->n_samples < 1) return NRNERF_ERR_INVALID;
    if (!backward && !a->loss) return NRNERF_ERR_INVALID;
    if (a->offsets_stride < 0 || a->rigidity_stride < 0 || (a->offsets_stride != 0 && a->offsets_stride < 3)) return NRNERF_ERR_INVALID;
    if (backward && ((!a->g_loss && !a->g_mean) || !a->g_rgb_map || (a->rgb0 && !a->g_rgb0) || (a->weights && (!a->g_offsets || !a->g_rigidity)) ||
                     (a->divergence && !a->g_divergence))) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    const LossArgs l{a->n_rays, a->n_samples, a->rgb_map, a->rgb0, a->target, a->weights, a->offsets, a->rigidity, a->alpha, a->divergence,
                     a->offsets_weight, a->rigidity_weight, a->divergence_weight, a->schedule, a->loss, a->g_loss, a->g_rgb_map, a->g_rgb0, a->g_offsets,
                     a->g_rigidity, a->g_divergence, a->offsets_stride ? a->offsets_stride : 3, a->rigidity_stride ? a->rigidity_stride : 1,
                     backward ? a->g_mean : nullptr};
    // (the backward call's `loss` may be null: its device is the one of the gradient it writes)
    return on_owner_of(backward ? (const void*)a->g_rgb_map : (const void*)a->loss, [&] { return status_of(launch_loss(l, backward, (hipStream_t)hip_stream)); });
}
int reduce_partials_call(const float* partials, int64_t record_stride, int32_t n_partials, int32_t n_short, const int32_t* index,
                         int64_t n_out, float* out, const float* aux, int32_t n_aux, const int64_t* aux_pos, void* hip_stream) {
    if (!partials || !index || !out || n_out < 0 || n_partials < 1 || n_short < 0 || n_short > n_partials || record_stride < 1 ||
        record_stride >= NRNERF_REDUCE_SHORT) return NRNERF_ERR_INVALID;
    if (aux && (n_aux < 0 || !aux_pos)) return NRNERF_ERR_INVALID;
    if (n_out == 0) return NRNERF_OK;
    return on_owner_of(out, [&] {
        ReducePartialsArgs a{partials, record_stride, n_partials, n_short, index, n_out, out, aux, aux ? n_aux : 0, {-1, -1, -1, -1}};
        if (aux)
            for (int c = 0; c < 4; ++c) {
                if (aux_pos[c] >= n_out) return (int)NRNERF_ERR_INVALID;
                a.aux_pos[c] = aux_pos[c];
            }
        return status_of(launch_reduce_partials(a, (hipStream_t)hip_stream));
    });
}
}  // namespace
extern "C" {
int nrnerf_loss_forward(const nrnerf_loss_args* a, void* hip_stream) try { return loss_call(a, false, hip_stream); } NRN_CATCH
int nrnerf_loss_backward(const nrnerf_loss_args* a, void* hip_stream) try { return loss_call(a, true, hip_stream); } NRN_CATCH

int nrnerf_code_gradients(const int64_t* index, const float* g, int32_t n_rays, int32_t latent_size, int32_t n_codes, float* out, void* hip_stream) try {
    if (!index || !g || !out || n_rays < 0 || latent_size < 1 || latent_size > 256 || n_codes < 0) return NRNERF_ERR_INVALID;
    if (n_codes == 0) return NRNERF_OK;
    const CodeGradArgs c{(const long long*)index, g, n_rays, latent_size, n_codes, out};
    return on_owner_of(out, [&] { return status_of(launch_code_gradients(c, (hipStream_t)hip_stream)); });
} NRN_CATCH

int nrnerf_merge_rows(const uint8_t* rank_new, int32_t n_rays, int32_t n_samples, int32_t n_importance, float* coarse_a, float* coarse_b,
                      float* new_a, float* new_b, float* merged_a, float* merged_b, int32_t inverse, void* hip_stream) try {
    if (!rank_new || !coarse_a || !new_a || !merged_a || n_rays < 0 || n_samples < 1 || n_importance < 1 || n_samples + n_importance > 256) return NRNERF_ERR_INVALID;
    if ((coarse_b != nullptr) != (merged_b != nullptr) || (new_b != nullptr) != (merged_b != nullptr)) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    const MergeRowsArgs a{n_rays, n_samples, n_importance, rank_new, coarse_a, coarse_b, new_a, new_b, merged_a, merged_b, inverse ? 1 : 0};
    return on_owner_of(merged_a, [&] { return status_of(launch_merge_rows(a, (hipStream_t)hip_stream)); });
} NRN_CATCH

int nrnerf_reduce_partials(const float* partials, int64_t record_stride, int32_t n_partials, int32_t n_short, const int32_t* index,
                           int64_t n_out, float* out, void* hip_stream) try {
    return reduce_partials_call(partials, record_stride, n_partials, n_short, index, n_out, out, nullptr, 0, nullptr, hip_stream);
} NRN_CATCH
int nrnerf_reduce_partials_aux(const float* partials, int64_t record_stride, int32_t n_partials, int32_t n_short, const int32_t* index,
                               int64_t n_out, float* out, const float* aux, int32_t n_aux, const int64_t* aux_pos, void* hip_stream) try {
    return reduce_partials_call(partials, record_stride, n_partials, n_short, index, n_out, out, aux, n_aux, aux_pos, hip_stream);
} NRN_CATCH

int nrnerf_tile_row_sums(const void* tiles, int64_t n_rows, float* out, void* hip_stream) try {
    if (!tiles || !out || n_rows < 0) return NRNERF_ERR_INVALID;
    if (n_rows == 0) return NRNERF_OK;
    return on_owner_of(out, [&] { return status_of(launch_tile_row_sums(tiles, n_rows, out, (hipStream_t)hip_stream)); });
} NRN_CATCH

int nrnerf_tiles_to_rows(const void* tiles, int32_t n_rays, int32_t n_samples, int32_t width, void* rows, void* hip_stream) try {
    if (!tiles || !rows || n_rays < 0 || n_samples < 1 || n_samples > 256 || (width != 256 && width != 128)) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    return on_owner_of(rows, [&] { return status_of(launch_tiles_to_rows(tiles, n_rays, n_samples, width, rows, (hipStream_t)hip_stream)); });
} NRN_CATCH

int nrnerf_direction_encoding(const float* bent4, int32_t n_rays, int32_t n_samples, int32_t n_freqs, void* enc, int32_t enc_is_bf16,
                              float* g_bent4, void* hip_stream) try {
    if (!bent4 || !enc || n_rays < 0 || n_samples < 2 || n_samples > NRNERF_MAX_SAMPLES || n_freqs < 0 || n_freqs > 10) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    const DirEncodingArgs d{bent4, n_rays, n_samples, n_freqs, enc, enc_is_bf16 ? 1 : 0, g_bent4};
    return on_owner_of(enc, [&] { return status_of(launch_dir_encoding(d, g_bent4 != nullptr, (hipStream_t)hip_stream)); });
} NRN_CATCH
}  // extern "C"

// ---- the compiled trunk (nrnerf_train.h) -------------------------------------------------------------------------------------------
namespace {
int trunk_call(const nrnerf_model* m, const nrnerf_trunk_args* a, bool bwd, void* hip_stream) {
    if (!m || !a || a->struct_size != sizeof(nrnerf_trunk_args)) return NRNERF_ERR_INVALID;
    if (!m->train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || (a->which != 0 && a->which != 1)) return NRNERF_ERR_INVALID;
    if (!a->pts4 || !a->acts) return NRNERF_ERR_INVALID;
    if (!bwd && (!a->raw4 || (a->raw && a->raw_ch != 4 && a->raw_ch != 5))) return NRNERF_ERR_INVALID;
    if (bwd && (!a->d_raw4 || !a->d_pre || !a->d_pts4)) return NRNERF_ERR_INVALID;
    const bool fine = a->which == 1;
    const PassDev& fwd = m->coarse_train.stream ? ((fine && !m->fine_is_coarse) ? m->fine_train : m->coarse_train)
                                  : (m->has_bend ? (fine ? m->fine_trunk : m->coarse_trunk) : (fine ? m->fine : m->coarse));
    const PassDev& bw = (fine && !m->fine_is_coarse) ? m->fine_bwd : m->coarse_bwd;
    TrunkArgs t{};
    t.pts4 = a->pts4; t.n_rays = a->n_rays; t.S = a->n_samples;
    t.wstream = bwd ? bw.stream : fwd.stream; t.bias = fwd.bias;          // (the backward launch takes the forward image's bias table too)
    t.raw4 = a->raw4; t.raw_out = a->raw; t.raw_ch = a->raw_ch;
    t.acts = a->acts; t.d_raw4 = a->d_raw4; t.d_pre = a->d_pre; t.d_pts4 = a->d_pts4; t.ray_bias = a->ray_bias;
    t.mask = (unsigned short*)a->relu_mask;
    if (!is_f32(m) && !t.mask) return NRNERF_ERR_INVALID;
    if (m->views) {             // the colour branch behind the trunk (the *_views kernels)
        if (!a->dirs || !a->hv || (bwd && !a->d_pre_v) || (!is_f32(m) && !a->hv_mask)) return NRNERF_ERR_INVALID;
        t.dirs = a->dirs; t.hv = a->hv; t.hv_mask = (unsigned short*)a->hv_mask; t.d_pre_v = a->d_pre_v; t.d_dirs = a->d_dirs;
    }
    if (a->n_rays == 0) return NRNERF_OK;
    const TrunkKernels& k = trunk_kernels(m);
    return on_model_device(m, [&] { return status_of((bwd ? k.bwd : k.fwd)(t, m->num_cus, (hipStream_t)hip_stream)); });
}
}  // namespace
extern "C" {
int nrnerf_trunk_forward(const nrnerf_model* m, const nrnerf_trunk_args* a, void* hip_stream) try { return trunk_call(m, a, false, hip_stream); } NRN_CATCH
int nrnerf_trunk_backward(const nrnerf_model* m, const nrnerf_trunk_args* a, void* hip_stream) try { return trunk_call(m, a, true, hip_stream); } NRN_CATCH

int nrnerf_trunk_wgrad(const nrnerf_model* m, const nrnerf_wgrad_args* a, void* hip_stream) try {
    if (!m || !a || a->struct_size != sizeof(nrnerf_wgrad_args)) return NRNERF_ERR_INVALID;
    if (!m->train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->n_partials < 1 || a->n_partials > 4096) return NRNERF_ERR_INVALID;
    if (!a->acts || !a->d_pre || !a->pts4 || !a->d_raw4 || !a->enc || !a->g_head || !a->partials) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    const bool f32 = is_f32(m);
    const int W = (m->arch_id == 5) ? ArchNarrow::W : ArchDefault::W, D = ArchDefault::D, SKIP = ArchDefault::SKIP;
    const long long nblocks = (long long)a->n_rays * ((a->n_samples + 31) / 32);
    const long long M = (long long)a->n_rays * a->n_samples;
    // elements of one layer of acts / d_pre: bf16 [block][W][32 samples] tiles, or (fp32 mode) rows [sample][W]
    const size_t layer = f32 ? (size_t)M * W : (size_t)nblocks * W * 32;
    const size_t esz = f32 ? 4 : 2;
    float* const dwh = a->partials;                                 // record layout: NRNERF_WGRAD_STRIDE
    float* const dwe = dwh + (size_t)(D - 1) * W * W;
    float* const dwo = dwe + (size_t)2 * W * 64;
    float* const db = dwo + (size_t)W * 64;
    const char* acts = (const char*)a->acts;
    const char* dpre = (const char*)a->d_pre;
    WgradArgs w{};
    w.nblocks = f32 ? M : nblocks; w.pstride = NRNERF_WGRAD_STRIDE(D, W);
    w.sync_every = NRN_WGRAD_SYNC_DEFAULT;       // (swept in round 3, tools/experiments/README.md; a build-time constant: the library reads no environment)
    // a 64-column job (encoding, head) loads 2 TR + 2 fragments per block and wave, a hidden-to-hidden one 2 TR + 2 TCW:
    // give it that share of the workgroups, so that all workgroups of the launch finish together
    // (fp32 mode: the same split; its 64-column jobs issue a quarter / half of a hidden-to-hidden job's MFMAs per sample and
    //  finish early -- 1.9 of 8.9 n_partials workgroups)
    const int kh = a->n_partials;
    int kl = NRNERF_WGRAD_SHORT_PARTIALS(kh, W);
    kl = kl > kh ? kh : kl;
    int n = 0;
    for (int i = 1; i < D; ++i)                                     // hidden-to-hidden layers: the bulk, first in the grid
        w.job[n++] = WgradJob{dpre + i * layer * esz, acts + (i - 1) * layer * esz, W, dwh + (size_t)(i - 1) * W * W, db + (size_t)i * W, kh, 0, W};
    const bool views = m->views != 0;
    float* const dwf = db + (size_t)(D + 1) * W;                     // view-dependent head: NRNERF_WGRAD_STRIDE_VIEWS
    float* const dwd = dwf + (size_t)(W / 2) * W;
    float* const dwr = dwd + (size_t)(W / 2) * 64;
    float* const dbv = dwr + (size_t)(W / 2) * 64;
    if (views) {
        if (!a->dirs || !a->hv || !a->d_pre_v || !a->encv) return NRNERF_ERR_INVALID;
        w.pstride = NRNERF_WGRAD_STRIDE_VIEWS(D, W);
        // (half the rows of a hidden-to-hidden product per block: its workgroups finish early; kept at kh records so that the
        //  caller's reduction knows two record counts only)
        w.job[n++] = WgradJob{a->d_pre_v, acts + (D - 1) * layer * esz, W, dwf, dbv, kh, 0, W / 2};
    }
    w.job[n++] = WgradJob{dpre, a->enc, 64, dwe, db, kl, 0, W};
    w.job[n++] = WgradJob{dpre + (SKIP + 1) * layer * esz, a->enc, 64, dwe + (size_t)W * 64, db + (size_t)D * W, kl, 0, W};
    w.job[n++] = WgradJob{acts + (D - 1) * layer * esz, a->g_head, 64, dwo, db + (size_t)D * W, kl, 0, W};
    if (views) {        // (their row sums -- of d_pre_v again, of hv -- land in the scratch row db[depth])
        w.job[n++] = WgradJob{a->d_pre_v, a->encv, 64, dwd, db + (size_t)D * W, kl, 0, W / 2};
        w.job[n++] = WgradJob{a->hv, a->g_head, 64, dwr, db + (size_t)D * W, kl, 0, W / 2};
    }
    w.njobs = n;
    for (int j = 0, wg = 0; j < n; ++j) { w.job[j].wg0 = wg; wg += w.job[j].kch; w.nwg = wg; }
    return on_model_device(m, [&] {
        const hipStream_t s = (hipStream_t)hip_stream;
        const WgradOperandArgs ops{a->pts4, a->d_raw4, a->n_rays, a->n_samples, ArchDefault::L, a->enc, a->g_head, f32 ? nullptr : a->head_sums,
                                   views ? a->dirs : nullptr, ArchDefault::LV, views ? a->encv : nullptr};
        if ((f32 ? launch_wgrad_operands_f32(ops, s) : launch_wgrad_operands(ops, s)) != hipSuccess) return (int)NRNERF_ERR_HIP;
        return status_of(trunk_kernels(m).wgrad(w, s));
    });
} NRN_CATCH
}  // extern "C"

// ---- the ray bender (nrnerf_train_bend.h) and its divergence regulariser -------------------------------------------------------------
namespace {
int bender_call(const nrnerf_model* m, const nrnerf_bender_args* a, bool bwd, void* hip_stream) {
    if (!m || !a || a->struct_size != sizeof(nrnerf_bender_args)) return NRNERF_ERR_INVALID;
    if (!m->bend_train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES) return NRNERF_ERR_INVALID;
    if (!a->rays || a->ray_stride < 6 || !a->latents || a->latent_stride < m->latent_size || !a->z) return NRNERF_ERR_INVALID;
    if (!a->bent4 || !a->off4 || !a->acts_offsets || !a->acts_rigidity) return NRNERF_ERR_INVALID;
    if (bwd && (!a->g_bent4 || !a->dz_offsets || !a->dz_rigidity || !a->dz_out4 || !a->d_latents)) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    BendTrainArgs t{};
    t.rays = a->rays; t.ray_stride = a->ray_stride; t.latents = a->latents; t.lat_stride = a->latent_stride; t.z = a->z;
    t.n_rays = a->n_rays; t.S = a->n_samples;
    const PassDev& p = bwd ? m->bend_train_bwd : m->bend_train_fwd;
    t.wstream = p.stream; t.bias = p.bias;
    t.knobs = rigidity_knobs(*a);
    t.bent4 = a->bent4; t.off4 = a->off4; t.acts_b = a->acts_offsets; t.acts_r = a->acts_rigidity;
    t.g_bent4 = a->g_bent4; t.g_bent4_b = a->g_bent4_b; t.g_unmasked = a->g_unmasked_offsets; t.g_mask = a->g_rigidity_mask;
    t.dz_b = a->dz_offsets; t.dz_r = a->dz_rigidity; t.dz_out4 = a->dz_out4; t.d_lat = a->d_latents;
    const BenderKernels& k = bender_kernels(m);
    // (the last argument: the element type of the saved arrays, nrnerf_bender_args)
    return on_model_device(m, [&] { return status_of((bwd ? k.bwd : k.fwd_train)(t, m->num_cus, (hipStream_t)hip_stream, !is_f32(m))); });
}

// the checks both divergence calls make, and the arguments of their kernels
int divergence_common(const nrnerf_model* m, const nrnerf_divergence_args* a, bool bwd, BendDivArgs& t) {
    if (!m || !a || a->struct_size != sizeof(nrnerf_divergence_args)) return NRNERF_ERR_INVALID;
    if (!m->bend_train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_points < 0 || a->n_points >= (1ll << 36)) return NRNERF_ERR_INVALID;
    if (!a->points || !a->probe || !a->latents || (a->latent_stride != 0 && a->latent_stride < m->latent_size)) return NRNERF_ERR_INVALID;
    if (!a->divergence || !a->off4 || !a->toff4 || !a->acts_offsets || !a->tacts_offsets || !a->acts_rigidity || !a->tacts_rigidity)
        return NRNERF_ERR_INVALID;
    if (bwd && ((!a->g_divergence && !a->g_tangent) || !a->dz_offsets || !a->dtz_offsets || !a->dz_rigidity || !a->dtz_rigidity || !a->dz_out4 ||
                !a->dtz_out4 || !a->d_latents || !a->partials || a->n_partials < 4 || a->n_partials > 4096 || a->n_partials % 4))
        return NRNERF_ERR_INVALID;
    t = BendDivArgs{};
    t.pts = a->points; t.latents = a->latents; t.lat_stride = a->latent_stride; t.e = a->probe; t.m = a->n_points;
    const PassDev& p = bwd ? m->bend_train_bwd : m->bend_train_fwd;
    t.wstream = p.stream; t.bias = p.bias;
    t.knobs = rigidity_knobs(*a);
    t.div = a->divergence; t.off4 = a->off4; t.toff4 = a->toff4; t.tvec = a->tangent; t.g_tvec = a->g_tangent;
    t.r_g_bent4 = a->render_g_bent4; t.r_g_bent4_b = a->render_g_bent4_b; t.r_g_unmasked = a->render_g_unmasked_offsets; t.r_g_mask = a->render_g_rigidity_mask;
    t.bent4 = bwd ? nullptr : a->bent4;
    t.acts_b = a->acts_offsets; t.tacts_b = a->tacts_offsets; t.acts_r = a->acts_rigidity; t.tacts_r = a->tacts_rigidity;
    t.g_div = a->g_divergence; t.dz_b = a->dz_offsets; t.dtz_b = a->dtz_offsets; t.dz_r = a->dz_rigidity; t.dtz_r = a->dtz_rigidity;
    t.dz_out4 = a->dz_out4; t.dtz_out4 = a->dtz_out4; t.d_lat = a->d_latents;
    return NRNERF_OK;
}
}  // namespace
extern "C" {
int nrnerf_bender_forward(const nrnerf_model* m, const nrnerf_bender_args* a, void* hip_stream) try { return bender_call(m, a, false, hip_stream); } NRN_CATCH
int nrnerf_bender_backward(const nrnerf_model* m, const nrnerf_bender_args* a, void* hip_stream) try { return bender_call(m, a, true, hip_stream); } NRN_CATCH

int nrnerf_bender_wgrad(const nrnerf_model* m, const nrnerf_bender_wgrad_args* a, void* hip_stream) try {
    if (!m || !a || a->struct_size != sizeof(nrnerf_bender_wgrad_args)) return NRNERF_ERR_INVALID;
    if (!m->bend_train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->n_partials < 4 || a->n_partials > 4096 || a->n_partials % 4) return NRNERF_ERR_INVALID;
    if (!a->rays || a->ray_stride < 6 || !a->latents || a->latent_stride < m->latent_size || !a->z) return NRNERF_ERR_INVALID;
    if (!a->acts_offsets || !a->acts_rigidity || !a->dz_offsets || !a->dz_rigidity || !a->dz_out4 || !a->partials) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    const size_t M = (size_t)a->n_rays * a->n_samples;
    if (!bend_wgrad_offsets_fit(m, M)) return NRNERF_ERR_INVALID;
    const int b16 = is_f32(m) ? 0 : 1;        // the saved arrays' element type; dz_out4 is fp32 in every mode
    const int X0 = 3 + ArchDefault::LAT;      // the first layers read [point, latent code] rows formed from the ray records: network[0] all of it, rigidity_network[0] the point
    BendWgradArgs w{};
    add_bend_chain(w, {a->dz_offsets, a->acts_offsets, nullptr, nullptr, bender_depth(m), ArchDefault::BW, a->dz_out4, nullptr, 3}, {{nullptr, X0, X0, nullptr}}, M, b16);
    add_bend_chain(w, {a->dz_rigidity, a->acts_rigidity, nullptr, nullptr, ArchDefault::RD, ArchDefault::RW, a->dz_out4 + 3, nullptr, 1}, {{nullptr, X0, 3, nullptr}}, M, b16);
    w.nparts = a->n_partials; w.m = (long long)M; w.out = a->partials;
    w.rays = a->rays; w.ray_stride = a->ray_stride; w.latents = a->latents; w.lat_stride = a->latent_stride; w.lat = m->latent_size;
    w.z = a->z; w.S = a->n_samples;
    return on_model_device(m, [&] { return run_bend_wgrad(m, w, (hipStream_t)hip_stream); });
} NRN_CATCH

int nrnerf_bender_divergence_forward(const nrnerf_model* m, const nrnerf_divergence_args* a, void* hip_stream) try {
    BendDivArgs t;
    const int rc = divergence_common(m, a, false, t);
    if (rc != NRNERF_OK) return rc;
    if (a->n_points == 0) return NRNERF_OK;
    return on_model_device(m, [&] { return status_of(bender_kernels(m).div_fwd(t, m->num_cus, (hipStream_t)hip_stream, !is_f32(m))); });
} NRN_CATCH

int nrnerf_bender_divergence_backward(const nrnerf_model* m, const nrnerf_divergence_args* a, void* hip_stream) try {
    BendDivArgs t;
    const int rc = divergence_common(m, a, true, t);
    if (rc != NRNERF_OK) return rc;
    if (a->n_points == 0) return NRNERF_OK;
    const size_t M = (size_t)a->n_points;
    if (!bend_wgrad_offsets_fit(m, M)) return NRNERF_ERR_INVALID;          // nothing is launched
    const int b16 = is_f32(m) ? 0 : 1;        // the saved arrays' element type; points / probes / latents / dz_out4: fp32
    // weight / bias gradients: dW_i = dz_i^T h_{i-1} + dtz_i^T th_{i-1} (two products per job), db_i = column sums of dz_i.  network[0] in two
    // jobs -- its point columns (th_0 = the probe) and its latent columns --, rigidity_network[0] reads the point alone
    BendWgradArgs w{};
    add_bend_chain(w, {a->dz_offsets, a->acts_offsets, a->dtz_offsets, a->tacts_offsets, bender_depth(m), ArchDefault::BW, a->dz_out4, a->dtz_out4, 3},
                   {{a->points, 3, 3, a->probe}, {a->latents, a->latent_stride, m->latent_size, nullptr}}, M, b16);
    add_bend_chain(w, {a->dz_rigidity, a->acts_rigidity, a->dtz_rigidity, a->tacts_rigidity, ArchDefault::RD, ArchDefault::RW, a->dz_out4 + 3, a->dtz_out4 + 3, 1},
                   {{a->points, 3, 3, a->probe}}, M, b16);
    w.nparts = a->n_partials; w.m = (long long)M; w.out = a->partials;
    w.S = 1;
    return on_model_device(m, [&] {
        const hipStream_t stream = (hipStream_t)hip_stream;
        if (bender_kernels(m).div_bwd(t, m->num_cus, stream, b16 != 0) != hipSuccess) return (int)NRNERF_ERR_HIP;
        return run_bend_wgrad(m, w, stream);
    });
} NRN_CATCH

// ---- compositing alone (composite_kernel / composite_bwd_kernel): no model, the device is the one that owns raw4 ------------------
int nrnerf_composite_forward(const nrnerf_composite_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_composite_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 2 || a->n_importance < 0) return NRNERF_ERR_INVALID;
    if (a->n_samples > NRNERF_MAX_SAMPLES || a->n_samples + a->n_importance > NRNERF_MAX_SAMPLES) return NRNERF_ERR_UNSUPPORTED;
    if (a->rank_new && a->n_samples + a->n_importance > 256) return NRNERF_ERR_UNSUPPORTED;       // 8-bit ranks (the split fine bender)
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || a->ray_stride < 8 || !a->raw4 || !a->rgb || !a->disp || !a->acc) return NRNERF_ERR_INVALID;
    if (a->n_importance > 0 && !a->z_merged) return NRNERF_ERR_INVALID;
    if ((a->z_new != nullptr) != (a->rank_new != nullptr)) return NRNERF_ERR_INVALID;
    CompositeArgs c{};
    c.rays = a->rays; c.ray_stride = a->ray_stride; c.raw4 = a->raw4; c.z = a->z; c.lindisp = a->lindisp;
    c.white_bkgd = a->white_bkgd; c.noise = a->noise; c.u = a->u; c.n_rays = a->n_rays; c.S = a->n_samples;
    c.n_importance = a->n_importance; c.rgb = a->rgb; c.disp = a->disp; c.acc = a->acc; c.z_std = a->z_std;
    c.z_out = a->z_merged; c.vis = a->weights; c.alpha = a->alpha;
    if (a->n_importance > 0) { c.z_new = a->z_new; c.rank_new = a->rank_new; }
    return on_owner_of(a->raw4, [&] { return status_of(launch_composite(c, (hipStream_t)hip_stream)); });
} NRN_CATCH

int nrnerf_composite_backward(const nrnerf_composite_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_composite_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 2 || a->n_samples > NRNERF_MAX_SAMPLES) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || a->ray_stride < 8 || !a->raw4 || !a->g_rgb || !a->d_raw4) return NRNERF_ERR_INVALID;
    CompositeBwdArgs c{};
    c.rays = a->rays; c.ray_stride = a->ray_stride; c.raw4 = a->raw4; c.z = a->z; c.lindisp = a->lindisp;
    c.white_bkgd = a->white_bkgd; c.noise = a->noise; c.n_rays = a->n_rays; c.S = a->n_samples;
    c.g_rgb = a->g_rgb; c.g_disp = a->g_disp; c.g_acc = a->g_acc; c.g_w = a->g_weights; c.d_raw4 = a->d_raw4;
    return on_owner_of(a->raw4, [&] { return status_of(launch_composite_bwd(c, (hipStream_t)hip_stream)); });
} NRN_CATCH

}  // extern "C"
