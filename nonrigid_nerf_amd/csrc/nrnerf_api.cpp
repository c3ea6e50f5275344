// nrnerf_api.cpp -- C ABI of libnrnerf_hip.so (include/nrnerf.h), the model and the renderer: model lifetime (upload / refresh / free of the
// weight images nrnerf_pack.cpp builds), workspace carving, kernel sequencing of nrnerf_render, ray generation, profiling.  The training
// entry points: nrnerf_train_api.cpp; what the two share: nrnerf_model.h.
//
// Kernel sequence of one nrnerf_render call (reference render_rays, train.py:792-980):
//   K0  network kernel, coarse weights, z = linspace(near, far, S)        -> raw_c [N,S,4]
//   K1  composite (+ sample_pdf + merge + z_std when I > 0)               -> rgb0/disp0/acc0 or final; z_fine [N,S+I]
//   K2  network kernel, fine weights, z = z_fine                          -> raw_f [N,S+I,4]
//   K3  composite                                                         -> rgb/disp/acc
// nrnerf_query (the reference's network_query_fn, train.py:57-105, 633-649) is ONE pass of that sequence on caller-given points, without
// compositing: plan_query / QueryCall below, on RenderCall's network step.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "nrnerf_model.h"
#include "nrnerf_aux.h"
#include "nrnerf_x16_api.h"
#include "nrnerf_plan.h"
#include "nrnerf_bend_points.h"
#include "nrnerf_field.h"

using namespace nrn;

namespace {

int upload_pass(const PackedPass& pk, PassDev& dev) {
    dev.stream_bytes = pk.stream.size();
    dev.bias_floats = pk.bias.size();
    if (hipMalloc(&dev.stream, pk.stream.size()) != hipSuccess) return NRNERF_ERR_NOMEM;
    if (hipMalloc((void**)&dev.bias, pk.bias.size() * 4) != hipSuccess) return NRNERF_ERR_NOMEM;
    if (hipMemcpy(dev.stream, pk.stream.data(), pk.stream.size(), hipMemcpyHostToDevice) != hipSuccess) return NRNERF_ERR_HIP;
    if (hipMemcpy(dev.bias, pk.bias.data(), pk.bias.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return NRNERF_ERR_HIP;
    if (!pk.src.empty()) {
        dev.n_elems = pk.src.size();
        if (hipMalloc((void**)&dev.src, pk.src.size() * 4) != hipSuccess || hipMalloc((void**)&dev.fmt, pk.fmt.size()) != hipSuccess ||
            hipMalloc((void**)&dev.bias_src, pk.bias_src.size() * 4) != hipSuccess) return NRNERF_ERR_NOMEM;
        if (hipMemcpy(dev.src, pk.src.data(), pk.src.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dev.fmt, pk.fmt.data(), pk.fmt.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dev.bias_src, pk.bias_src.data(), pk.bias_src.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return NRNERF_ERR_HIP;
    }
    return NRNERF_OK;
}
// new weights of the same architecture into the buffers the kernels already read (stream-ordered)
int refresh_pass(const PackedPass& pk, PassDev& dev, hipStream_t stream) {
    if (pk.stream.size() != dev.stream_bytes || pk.bias.size() != dev.bias_floats) return NRNERF_ERR_INVALID;
    if (hipMemcpyAsync(dev.stream, pk.stream.data(), pk.stream.size(), hipMemcpyHostToDevice, stream) != hipSuccess) return NRNERF_ERR_HIP;
    if (hipMemcpyAsync(dev.bias, pk.bias.data(), pk.bias.size() * 4, hipMemcpyHostToDevice, stream) != hipSuccess) return NRNERF_ERR_HIP;
    return NRNERF_OK;
}
void free_pass(PassDev& dev) {
    if (dev.stream) (void)hipFree(dev.stream);
    if (dev.bias) (void)hipFree(dev.bias);
    if (dev.src) (void)hipFree(dev.src);
    if (dev.fmt) (void)hipFree(dev.fmt);
    if (dev.bias_src) (void)hipFree(dev.bias_src);
    dev = PassDev{};
}

}  // namespace

extern "C" {

int nrnerf_abi_version(void) { return NRNERF_ABI_VERSION; }

const char* nrnerf_strerror(int status) {
    switch (status) {
        case NRNERF_OK: return "ok";
        case NRNERF_ERR_INVALID: return "invalid argument";
        case NRNERF_ERR_UNSUPPORTED: return "unsupported architecture or flag combination (no kernel compiled for it)";
        case NRNERF_ERR_HIP: return "HIP runtime error (no device, or a launch/copy failed)";
        case NRNERF_ERR_WORKSPACE: return "workspace too small or misaligned";
        case NRNERF_ERR_NOMEM: return "out of memory (device, or host while packing weights)";
        case NRNERF_ERR_INTERNAL: return "internal error (an exception was caught at the C ABI)";
    }
    return "unknown status";
}

int nrnerf_pack_host(const nrnerf_model_desc* desc, int which, nrnerf_packed_info* info, void* stream_out,
                     size_t stream_cap, uint32_t* unit_table_out, float* bias_table_out) try {
    if (!desc || desc->struct_size != sizeof(nrnerf_model_desc) || !desc->coarse) return NRNERF_ERR_INVALID;
    PackedPass pk;
    const int rc = pack_host_image(desc, which, pk);
    if (rc != NRNERF_OK) return rc;
    if (info) {
        info->stream_bytes = pk.stream.size();
        info->n_units = (uint32_t)pk.nunits;
        info->n_bias_tiles = (uint32_t)pk.ntiles;
        info->frag_bytes = (uint32_t)pk.frag_bytes;
        info->slot_bytes = (uint32_t)pk.slot_bytes;
        info->mfma_per_block = (uint32_t)pk.mfma_per_block;
    }
    if (stream_out) {
        if (stream_cap < pk.stream.size()) return NRNERF_ERR_INVALID;
        std::memcpy(stream_out, pk.stream.data(), pk.stream.size());
    }
    if (unit_table_out) std::memcpy(unit_table_out, pk.unit_off.data(), pk.unit_off.size() * 4);
    if (bias_table_out) std::memcpy(bias_table_out, pk.bias.data(), pk.bias.size() * 4);
    return NRNERF_OK;
} NRN_CATCH

int nrnerf_model_create(const nrnerf_model_desc* desc, nrnerf_model** out) try {
    if (!out) return NRNERF_ERR_INVALID;
    *out = nullptr;
    if (!desc || desc->struct_size != sizeof(nrnerf_model_desc) || !desc->coarse) return NRNERF_ERR_INVALID;
    const FlatLayout lay = flat_layout(*desc);
    ModelTraits traits;
    std::vector<Image> images;
    int rc = pack_images(*desc, &lay, traits, images);
    if (rc != NRNERF_OK) return rc;
    DeviceGuard guard(desc->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    // owns the handle until it is handed to the caller: every early return (and an exception caught by NRN_CATCH) frees
    // what was uploaded so far
    struct Owner {
        nrnerf_model* m;
        ~Owner() { if (m) nrnerf_model_destroy(m); }
    } own{new (std::nothrow) nrnerf_model(traits)};
    nrnerf_model* m = own.m;
    if (!m) return NRNERF_ERR_NOMEM;
    m->device = desc->device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, desc->device) != hipSuccess) return NRNERF_ERR_HIP;
    m->num_cus = prop.multiProcessorCount;
    if (hipMalloc((void**)&m->adam_barrier, 2 * sizeof(unsigned)) != hipSuccess || hipMemset(m->adam_barrier, 0, 2 * sizeof(unsigned)) != hipSuccess) return NRNERF_ERR_NOMEM;
    m->flat_floats = lay.total;
    for (const Image& im : images) {
        ImageDev& dev = m->img[im.slot];
        rc = upload_pass(im.pk, dev);
        if (rc != NRNERF_OK) return rc;
        dev.algo_flops_per_sample = im.algo_flops;
        dev.mfma_flops_per_sample = im.mfma_flops;
        dev.output_ch = im.output_ch;
        dev.prog = im.proto;
        dev.gx = im.gx;
    }
    own.m = nullptr;
    *out = m;
    return NRNERF_OK;
} NRN_CATCH

int nrnerf_model_update(nrnerf_model* m, const nrnerf_model_desc* desc, void* hip_stream) try {
    if (!m || !desc || desc->struct_size != sizeof(nrnerf_model_desc) || !desc->coarse) return NRNERF_ERR_INVALID;
    if (desc->device != m->device) return NRNERF_ERR_INVALID;
    ModelTraits traits;
    std::vector<Image> images;
    int rc = pack_images(*desc, nullptr, traits, images);
    if (rc == NRNERF_ERR_UNSUPPORTED) return NRNERF_ERR_INVALID;
    if (rc != NRNERF_OK) return rc;
    // a different model (architecture, precision, shape: other traits or another set of images): create a new handle instead
    size_t n_resident = 0;
    for (const ImageDev& dev : m->img) n_resident += dev.stream != nullptr;
    if (!same_traits(traits, *m) || images.size() != n_resident) return NRNERF_ERR_INVALID;
    for (const Image& im : images)
        if (!m->img[im.slot].stream) return NRNERF_ERR_INVALID;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    hipStream_t stream = (hipStream_t)hip_stream;
    for (size_t i = 0; i < images.size() && rc == NRNERF_OK; ++i) rc = refresh_pass(images[i].pk, m->img[images[i].slot], stream);
    // the packed host images die with this call: wait until the copies have consumed them
    if (hipStreamSynchronize(stream) != hipSuccess && rc == NRNERF_OK) rc = NRNERF_ERR_HIP;
    return rc;
} NRN_CATCH

int64_t nrnerf_model_flat_size(const nrnerf_model* m) { return m ? m->flat_floats : -1; }

int nrnerf_model_precision(const nrnerf_model* m) { return m ? m->precision : NRNERF_ERR_INVALID; }

int nrnerf_model_trains_bender(const nrnerf_model* m) { return m ? (m->bend_train_ok ? 1 : 0) : NRNERF_ERR_INVALID; }
int nrnerf_model_is_generic(const nrnerf_model* m) { return m ? (m->generic ? 1 : 0) : NRNERF_ERR_INVALID; }

int nrnerf_model_update_device(nrnerf_model* m, const float* flat_params, int64_t n_floats, void* hip_stream) try {
    if (!m || !flat_params || n_floats != m->flat_floats) return NRNERF_ERR_INVALID;
    // every image (weight stream + bias table) as one segment of ONE launch
    return on_model_device(m, [&] { return repack_batches(m, flat_params, (hipStream_t)hip_stream); });
} NRN_CATCH

void nrnerf_model_destroy(nrnerf_model* m) {
    if (!m) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(m->device);
    for (auto& e : m->prof_events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (ImageDev& im : m->img) free_pass(im);
    if (m->adam_barrier) (void)hipFree(m->adam_barrier);
    (void)hipSetDevice(prev);
    delete m;
}

}  // extern "C"
namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// work counters of the 16x16x32 stand-alone bender (BendArgs::work_counter): two launches per call, up to 512 counters each, 64 bytes apart
constexpr int BEND_COUNTERS_PER_LAUNCH = 512;
// ... and behind them one counter per 16x16x32 trunk launch (NetArgs::work_counter), 64 bytes apart
constexpr size_t BEND_COUNTER_BYTES = (size_t)2 * BEND_COUNTERS_PER_LAUNCH * 64 + 256;

// The workspace of a render call: ten slots, each 256-byte aligned, and the work counters behind them.  Byte offsets from the workspace's
// base; a slot the call does not have (`present` false) takes no room.  nrnerf_workspace_bytes answers `total`, nrnerf_render takes its
// pointers from the same object.
struct WorkspaceLayout {
    size_t raw_c, z_fine, raw_f, bent4, z_coarse, bent_c, z_new, rank_new, jdirs, counters, total = 0;
    WorkspaceLayout(int n_rays, int n_samples, int n_importance, bool jacobian_dirs) {
        const size_t N = (size_t)n_rays, S = (size_t)n_samples, I = (size_t)n_importance, SF = S + I;
        auto slot = [&](size_t bytes, bool present = true) {
            const size_t at = total;
            if (present) total += align_up(bytes, 256);
            return at;
        };
        raw_c = slot(N * S * 4 * sizeof(float));                    // raw outputs of the coarse pass
        z_fine = slot(N * SF * sizeof(float), I > 0);               // merged depths ...
        raw_f = slot(N * SF * 4 * sizeof(float), I > 0);            // ... and raw outputs of the fine pass
        bent4 = slot(N * SF * 4 * sizeof(float));                   // bent point + rigidity of the final pass (surface reduction, split-bender path)
        z_coarse = slot(N * S * sizeof(float));                     // jittered coarse depths (perturb > 0)
        bent_c = slot(N * S * 4 * sizeof(float), I > 0);            // split-bender path: coarse bent points,
        z_new = slot(N * I * sizeof(float), I > 0);                 //   depths ...
        rank_new = slot(N * I, I > 0);                              //   ... and rows of the new samples
        jdirs = slot(N * SF * 3 * sizeof(float), jacobian_dirs);    // per-sample Jacobian directions of a pass (generic handle, exact view directions)
        counters = slot(BEND_COUNTER_BYTES);                        // work counters of the stand-alone bender and 16x16x32 trunk launches
    }
    template <class T> T* at(void* base, size_t offset, bool present = true) const { return present ? (T*)((char*)base + offset) : nullptr; }
};

}  // namespace
extern "C" {

size_t nrnerf_workspace_bytes(const nrnerf_model* model, int32_t n_rays, int32_t n_samples, int32_t n_importance) {
    if (n_rays <= 0 || n_samples <= 0 || n_importance < 0) return 0;
    return WorkspaceLayout(n_rays, n_samples, n_importance, model && model->generic && model->exact).total;
}

}  // extern "C"
namespace {
// ---- nrnerf_render decides, then launches: plan_render says which kernels a call takes (no HIP call, no side effect, no device pointer),
// RenderCall launches them -- per pass a bender step, a network step, a compositing step.  A new kernel route touches: the family enum,
// one rule in plan_render, one case in the executor.
#ifndef NRN_COARSE_EPILOGUE_DEFAULT
#define NRN_COARSE_EPILOGUE_DEFAULT 0
#endif
enum class BendStep { None, Fused, Compiled, Program };      // no bender / inside the network kernel / stand-alone compiled kernel / generic bender program
// net_kernel with its fused bender / without one (a model without bender, the split path's trunk-only pass) / the 16x16x32 trunk (nrnerf_net_x16.h) /
// the width-class 16x16x32 trunk (nrnerf_gx16.h) / the run-time-parameterised kernel (nrnerf_generic.h) / the same on exact Jacobian directions
enum class NetFamily { NetBender, NetTrunk, NetX16, Gx16, Gen, GenExact };
enum class CompStep { Launch, Epilogue, EpilogueSample };    // composite_kernel's own launch / the network kernel's epilogue / ... with sample_pdf and the merge
struct PassPlan {
    bool exists = false;
    bool final = false;            // its maps are the call's outputs (the only pass, or the fine one); else rgb0 / disp0 / acc0, sample_pdf, merged depths
    int which = 0, S = 0;          // 0: coarse, 1: fine; samples per ray
    BendStep bend = BendStep::None;
    int bend_n = 0, bend_stride = 0, bend_slot = 0;          // stand-alone bender: n_per_ray samples of every ray to rows of out_stride; profile slot 5 / 4
    bool bend_rank = false, bend_dynamic = false;            // ... at row rank[.] of the ray (the importance samples); blocks handed out by a work counter
    NetFamily net = NetFamily::NetTrunk;
    ImageSlot image = IMG_COARSE;                            // the packed weights the network kernel reads (and the profile's flops per sample)
    int dispatch = 0, net_slot = 0;                          // the launcher's architecture index / width class; profile slot 0 / 2 (composite: + 1)
    const char* name = "";                                   // profile display name
    bool trunk_counter = false;                              // net_kernel_x16: ray groups handed out by a work counter
    CompStep comp = CompStep::Launch;
};
struct RenderPlan {
    bool generic = false, split = false, surface = false;
    bool bend_x16 = false;         // the stand-alone bender is the 16x16x32 kernel (else the 32x32x16 one)
    bool counters_first = false;   // the work counters' memset node goes ahead of every launch of the call (else: with the first launch that takes one)
    PassPlan coarse, fine;
};

bool no_detail_outputs(const nrnerf_sample_outputs& o) {
    return !(o.visibility_weights || o.opacity_alpha || o.initial_input_pts || o.unmasked_offsets || o.masked_offsets || o.input_pts || o.rigidity_mask);
}
// the stand-alone bender kernels index their 32-sample blocks with 32 bits: beyond 2^31 blocks a pass stays on the other kernels
bool block_index_fits(int N, int S) { return (long long)N * ((S + 31) / 32) < (1ll << 31); }
// A pass' compositing as its network kernel's epilogue: at most 256 samples, and at least one GROUP of rays per CU -- a fused pass hands out whole
// groups of rays (4 rays = 24 blocks at 192 samples) where the plain mapping hands out 8-block tiles, so below that the plain mapping fills more
// of the chip.  The group is the kernel family's own.
bool enough_rays_to_fuse(const nrnerf_model& m, const PassPlan& p, int N) {
    long long group;
    if (p.net == NetFamily::NetX16) group = x16_rays_per_group(p.dispatch, p.S);
    else if (p.net == NetFamily::Gx16) group = gx16_rays_per_group(p.dispatch, p.S);
    // waves per workgroup x rays per wave: fp32 kernels 4 x 1; 16-bit two-blocks-per-wave kernels 4 x (1 or 2); 16-bit one-block-per-wave
    // kernels (architecture 5) 8 x 1
    else group = (m.precision == NRNERF_PREC_F32) ? 4 : (m.arch_id == 5 ? 8 : ((((p.S + 31) / 32) & 1) ? 8 : 4));
    return p.S <= 256 && (long long)N >= group * m.num_cus;
}

RenderPlan plan_render(const nrnerf_model& m, const nrnerf_render_args& a) {
    const int N = a.n_rays, S = a.n_samples, I = a.n_importance;
    auto flag = [&](unsigned f) { return (a.flags & f) != 0; };
    const bool plain = !a.detailed_output, unfused = flag(NRNERF_RENDER_UNFUSED_COMPOSITE), dynamic = !flag(NRNERF_RENDER_FIXED_SHARES);
    RenderPlan r;
    r.generic = m.generic != 0;
    r.surface = a.surface_pts || a.surface_rigidity || a.median_index;
    // Split-bender path: bender, no view-dependent head, a fine pass, no per-sample detail outputs (those are written by the fused kernels), 8-bit
    // ranks among the merged depths (<= 256 samples per ray).  NRNERF_RENDER_FUSED_FINE_BENDER keeps the fused fine pass (A/B and bit-identity tests).
    r.split = m.split_ok && I > 0 && plain && no_detail_outputs(a.coarse) && no_detail_outputs(a.fine) && !flag(NRNERF_RENDER_FUSED_FINE_BENDER) &&
              block_index_fits(N, imax(S, I)) && S + I <= 256;
    // the stand-alone bender: the 16x16x32 kernel (nrnerf_bend_x16.h; "bf16" mode's single-product bender) unless the call asks for the 32x32x16
    // one (NRNERF_RENDER_BENDER_32X32: the bit-identity tests against the fused-bender kernels)
    r.bend_x16 = m.bend_x16.stream && !flag(NRNERF_RENDER_BENDER_32X32 | NRNERF_RENDER_NO_X16);
    const bool bend_counters = r.bend_x16 && dynamic && m.num_cus <= BEND_COUNTERS_PER_LAUNCH;      // (one counter per pair of co-resident workgroups)
    r.counters_first = bend_counters;
    for (int which = 0; which < (I > 0 ? 2 : 1); ++which) {
        PassPlan& p = which ? r.fine : r.coarse;
        const nrnerf_sample_outputs& so = which ? a.fine : a.coarse;
        p.exists = true; p.which = which; p.final = which == 1 || I == 0; p.S = which ? S + I : S;
        p.net_slot = 2 * which; p.bend_slot = 5 - which;
        bool trunk_only = false;
        if (m.generic) {
            // architecture outside the compiled set (nrnerf_generic.h): per pass the bender over ALL its samples (no split-bender trick: this route
            // trades speed for generality), the canonical network on the bent points, compositing
            if (m.has_bend) {
                // the reference's own bender shape: the compiled stand-alone kernel (weights resident in LDS) when the pass wants no detail outputs.
                // Fixed shares here: with all samples of a ray in one launch the counters measured SLOWER -- width 192: 1.72 -> 1.82 ms per fine
                // pass, profiles/r06_dynamic_shares_ab.txt -- where the split path's launches gain 8 %
                p.bend = (m.gen_compiled_bender >= 0 && no_detail_outputs(so) && block_index_fits(N, p.S)) ? BendStep::Compiled : BendStep::Program;
                p.bend_n = p.bend_stride = p.S;
            }
            const bool own = which && !m.fine_is_coarse;        // (one network for both passes: the fine pass runs on the coarse images)
            const ImageDev& gx = m.img[own ? IMG_GX_FINE : IMG_GX_COARSE];
            p.net = NetFamily::Gen; p.image = own ? IMG_GEN_FINE : IMG_GEN_COARSE; p.name = "gen_kernel";
            if (m.exact) {
                p.net = NetFamily::GenExact; p.name = "gen_kernel (exact Jacobian directions)";
            } else if (m.has_bend && gx.stream && !flag(NRNERF_RENDER_NO_X16) && no_detail_outputs(so) && plain && (long long)N * p.S < (1ll << 32)) {
                // the width-class 16x16x32 trunk when the pass runs on ready-made points and wants no detail outputs (32-bit sample rows).  A FINAL
                // pass takes its compositing as the epilogue; NRNERF_RENDER_UNFUSED_COMPOSITE keeps the launch (bit-identity tests)
                p.net = NetFamily::Gx16; p.image = own ? IMG_GX_FINE : IMG_GX_COARSE; p.dispatch = gx.gx.wc;
                if (p.final && !unfused && enough_rays_to_fuse(m, p, N)) p.comp = CompStep::Epilogue;
                p.name = p.comp == CompStep::Epilogue ? "gx16_kernel + fused compositing" : "gx16_kernel";
            }
            continue;
        }
        // The 16x16x32 trunk-only kernel (nrnerf_net_x16.h) for the passes of the split path.  Per call (nrnerf_render_args::flags; the parity tests
        // run the kernels side by side in one process): NRNERF_RENDER_NO_X16 = the 32x32x16 kernels of nrnerf_net_mb.h, NRNERF_RENDER_X16_FINE_ONLY =
        // the fine pass only, default = the coarse pass too -- stand-alone bender over the S coarse samples + 16x16x32 trunk instead of the
        // fused-bender 32x32x16 kernel.
        const ImageSlot x16_image = which ? IMG_FINE_TRUNK_X16 : IMG_COARSE_TRUNK_X16;
        const bool x16 = r.split && !flag(NRNERF_RENDER_NO_X16) && (which || !flag(NRNERF_RENDER_X16_FINE_ONLY)) && m.img[x16_image].stream && plain;
        // The coarse pass stays fused by default: measured on MI355X (round 2), bender kernel 1.56 ms + trunk-only coarse kernel 8.72 ms = 10.28 ms
        // against 10.22 ms fused -- nothing is saved there, unlike in the fine pass where a third of the samples skips the bender (only the I
        // importance samples go through it; the coarse samples' bent points are already in place).  NRNERF_RENDER_SPLIT_COARSE splits it as well (A/B).
        const bool split_pass = r.split && (which || flag(NRNERF_RENDER_SPLIT_COARSE) || x16);
        p.image = (which && !m.fine_is_coarse) ? IMG_FINE : IMG_COARSE;
        p.dispatch = m.exact ? 3 + m.arch_id : m.arch_id;
        p.bend = m.has_bend ? BendStep::Fused : BendStep::None;
        p.net = m.has_bend ? NetFamily::NetBender : NetFamily::NetTrunk;
        if (split_pass) {
            p.bend = BendStep::Compiled; p.bend_n = which ? I : S; p.bend_stride = p.S; p.bend_rank = which == 1; p.bend_dynamic = bend_counters;
            p.net = x16 ? NetFamily::NetX16 : NetFamily::NetTrunk; p.dispatch = trunk_arch(m.arch_id); p.trunk_counter = x16 && dynamic;
            p.image = x16 ? x16_image : (which ? IMG_FINE_TRUNK : IMG_COARSE_TRUNK);
            trunk_only = !x16;
        }
        // Compositing fused into the FINAL pass' network kernel (north_star: "compositing fused into the ray loop"; the reference calls
        // raw2outputs inline, train.py:943-950): the kernel variants without a fused bender let each wave own whole rays, keep their raw outputs
        // in LDS and composite them itself (nrnerf_composite_ray.h: the composite kernel's own code, so the same bits).  The pass' raw array never
        // exists and one launch goes.  NRNERF_RENDER_UNFUSED_COMPOSITE keeps the separate launch (A/B and bit-identity tests).
        if (p.final && p.bend != BendStep::Fused && !unfused && enough_rays_to_fuse(m, p, N)) p.comp = CompStep::Epilogue;
        // The coarse pass of a hierarchical render keeps its composite kernel (sample_pdf and the merge follow it there) -- unless it runs on the
        // 16x16x32 trunk, where they can be its epilogue too (net_kernel_x16<.., SAMPLE>, train.py:889-920; raw_c never reaches HBM).
        // NRNERF_RENDER_COARSE_EPILOGUE_ON / _OFF select per call; the default (off) follows the A/B on one box.
        const bool epilogue_wanted = !flag(NRNERF_RENDER_COARSE_EPILOGUE_OFF) && (flag(NRNERF_RENDER_COARSE_EPILOGUE_ON) || NRN_COARSE_EPILOGUE_DEFAULT != 0);
        if (!p.final && x16 && epilogue_wanted && !unfused && S <= x16_coarse_epilogue_max_samples() && enough_rays_to_fuse(m, p, N)) p.comp = CompStep::EpilogueSample;
        const bool fused = p.comp != CompStep::Launch;
        if (x16) p.name = p.comp == CompStep::EpilogueSample ? "net_kernel_x16 + fused compositing, sample_pdf, merge" : (fused ? "net_kernel_x16 + fused compositing" : "net_kernel_x16");
        else if (trunk_only) p.name = fused ? "net_kernel (trunk only) + fused compositing" : "net_kernel (trunk only)";
        else p.name = m.has_bend ? "net_kernel (fused bender)" : (fused ? "net_kernel + fused compositing" : "net_kernel");
    }
    return r;
}

// The launches of one call: the workspace carved once, then per pass (run_pass) a bender step, a network step and a compositing step.
struct RenderCall {
    const nrnerf_model* const m;
    const nrnerf_render_args* const a;
    const RenderPlan& plan;
    const hipStream_t stream;
    const int N = a->n_rays, I = a->n_importance;
    Knobs kn{};
    bool prof = false;
    float *raw_c, *z_fine, *raw_f, *bent4_ws, *z_coarse, *bent_c, *z_new, *jdirs;
    uint8_t* rank_new;
    unsigned* counters;            // one counter per stand-alone bender launch of the call and per 16x16x32 trunk launch, 64 bytes apart
    bool counters_zeroed = false;
    const float* zc = nullptr;     // explicit coarse depths (stratified jitter), or null: the coarse spacing
    const float* given_pts = nullptr;      // nrnerf_query without a bender: the pass' ready-made points [N, S, 4] (else: what a bender step wrote)

    // nrnerf_query: one pass on a workspace of its own -- the pass' raw rows, its points, the work counters (`a`: the call as a render call)
    RenderCall(const nrnerf_model* m_, const nrnerf_render_args* a_, const RenderPlan& plan_, hipStream_t stream_, float* raw4, float* pts4, unsigned* counters_)
        : m(m_), a(a_), plan(plan_), stream(stream_) {
        raw_c = raw_f = raw4; bent4_ws = bent_c = pts4; counters = counters_;
        z_fine = z_coarse = z_new = jdirs = nullptr; rank_new = nullptr;
        kn.has_cutoff = a->has_rigidity_cutoff; kn.cutoff = a->rigidity_cutoff;
        kn.has_scaling = a->has_test_time_scaling; kn.scaling = a->test_time_scaling;
        kn.has_removal = a->has_removal_threshold; kn.removal = a->removal_threshold;
        kn.detailed = a->detailed_output;
        std::lock_guard<std::mutex> g(m->prof_mu);
        prof = m->prof_on;
    }
    RenderCall(const nrnerf_model* m_, const nrnerf_render_args* a_, const RenderPlan& plan_, const WorkspaceLayout& lay, hipStream_t stream_)
        : m(m_), a(a_), plan(plan_), stream(stream_) {
        void* const ws = a->workspace;
        raw_c = lay.at<float>(ws, lay.raw_c);
        z_fine = lay.at<float>(ws, lay.z_fine, I > 0);
        raw_f = lay.at<float>(ws, lay.raw_f, I > 0);
        bent4_ws = lay.at<float>(ws, lay.bent4);
        z_coarse = lay.at<float>(ws, lay.z_coarse);
        bent_c = lay.at<float>(ws, lay.bent_c, I > 0);
        z_new = lay.at<float>(ws, lay.z_new, I > 0);
        rank_new = lay.at<uint8_t>(ws, lay.rank_new, I > 0);
        jdirs = lay.at<float>(ws, lay.jdirs, m->generic && m->exact);      // [N, S + I | S, 3]: exact Jacobian directions of the pass in flight
        counters = lay.at<unsigned>(ws, lay.counters);
        kn.has_cutoff = a->has_rigidity_cutoff; kn.cutoff = a->rigidity_cutoff;
        kn.has_scaling = a->has_test_time_scaling; kn.scaling = a->test_time_scaling;
        kn.has_removal = a->has_removal_threshold; kn.removal = a->removal_threshold;
        kn.detailed = a->detailed_output;
        std::lock_guard<std::mutex> g(m->prof_mu);
        prof = m->prof_on;
    }
    // a launch's work counter(s), `at` words into the block -- zeroed by ONE memset node per call, ahead of its first use; nullptr: fixed shares
    unsigned* counter(bool wanted, size_t at) {
        if (!wanted || (!counters_zeroed && hipMemsetAsync(counters, 0, BEND_COUNTER_BYTES, stream) != hipSuccess)) return nullptr;
        counters_zeroed = true;
        return counters + at;
    }
    // the profile record of a launch over `samples` samples per ray on image `im`
    nrnerf_model::Ev work(int slot, const char* name, const ImageDev& im, int samples) const {
        const double n = (double)N * samples;
        return {slot, nullptr, nullptr, n * im.algo_flops_per_sample, n * im.mfma_flops_per_sample, name};
    }
    template <class F> hipError_t timed(nrnerf_model::Ev ev, F&& launch) {
        if (!prof) return launch();
        // device-scope events (no system-scope cache write-back with every record).  Measured A/B against default events on
        // one box: no difference (36.00 / 36.04 vs 36.14 / 35.99 ms per step) -- the kernels' event times add up to the step
        // time within 0.05 ms either way, i.e. there are no launch gaps to recover between the five kernels of a render
        if (hipEventCreateWithFlags(&ev.a, hipEventDisableSystemFence) != hipSuccess ||
            hipEventCreateWithFlags(&ev.b, hipEventDisableSystemFence) != hipSuccess) return hipErrorUnknown;
        (void)hipEventRecord(ev.a, stream);
        const hipError_t e = launch();
        (void)hipEventRecord(ev.b, stream);
        std::lock_guard<std::mutex> g(m->prof_mu);
        m->prof_events.push_back(ev);
        return e;
    }
    // a layer program of a generic handle (the bender's, a network's) on the run-time-parameterised kernel
    hipError_t run_program(const nrnerf_model::Ev& ev, const GenArgs& g) { return timed(ev, [&] { return launch_generic(m->precision, g, m->num_cus, stream); }); }
    static SampleOut sample_out(const nrnerf_sample_outputs& o) {
        return SampleOut{o.visibility_weights, o.opacity_alpha, o.initial_input_pts, o.unmasked_offsets, o.masked_offsets, o.input_pts, o.rigidity_mask};
    }
    const nrnerf_sample_outputs& outputs_of(const PassPlan& p) const { return p.which ? a->fine : a->coarse; }
    const float* depths_of(const PassPlan& p) const { return p.which ? z_fine : zc; }
    float* points_of(const PassPlan& p) const { return p.final ? bent4_ws : bent_c; }      // [N, S, 4]: a coarse pass has its own array when a fine pass follows
    float* raw_of(const PassPlan& p) const { return p.which ? raw_f : raw_c; }              // [N, S, 4]: rgb + sigma, network kernel to composite kernel

    // bend_n samples of every ray through the bender (the compiled stand-alone kernel or the generic bender program), bent points to points_of(p)
    // -- at row rank_new[.] of the ray for the importance samples of the split path, else in order
    hipError_t bender_step(const PassPlan& p) {
        const float* const zv = p.bend_rank ? z_new : depths_of(p);
        if (p.bend == BendStep::Program) {
            const ImageDev& im = m->gen_bend;
            GenArgs g = im.prog;
            g.rays = a->rays; g.ray_stride = a->ray_stride; g.latents = a->latents; g.lat_stride = a->latent_stride;
            g.z = zv; g.lindisp = a->lindisp; g.n_rays = N; g.S = p.bend_n;
            g.wstream = im.stream; g.bias = im.bias;
            g.bent4 = points_of(p); g.ex = sample_out(outputs_of(p)); g.knobs = kn;
            return run_program(work(p.bend_slot, "gen_kernel (bender program)", im, p.bend_n), g);
        }
        const ImageDev& im = plan.bend_x16 ? m->bend_x16 : m->bend_only;
        BendArgs b{};
        b.rays = a->rays; b.ray_stride = a->ray_stride; b.latents = a->latents; b.lat_stride = a->latent_stride;
        b.z = zv; b.lindisp = a->lindisp; b.rank = p.bend_rank ? rank_new : nullptr; b.n_rays = N; b.n_per_ray = p.bend_n; b.out_stride = p.bend_stride;
        b.wstream = im.stream; b.bias = im.bias; b.bent4 = points_of(p); b.knobs = kn;
        b.work_counter = counter(p.bend_dynamic, (size_t)16 * BEND_COUNTERS_PER_LAUNCH * p.which);
        return timed(work(p.bend_slot, plan.bend_x16 ? "bend_kernel_x16" : "bend_kernel", im, p.bend_n), [&] {
            return plan.bend_x16 ? launch_bend_x16(bender_arch_of(m), b, m->num_cus, stream) : launch_bend(m->precision, bender_arch_of(m), b, m->num_cus, stream);
        });
    }
    // The compositing arguments of a pass: the call's maps for a final pass; else rgb0 / disp0 / acc0, sample_pdf and the merged depths of the fine pass
    CompositeArgs composite_args(const PassPlan& p) const {
        const bool fine = p.which == 1;
        const nrnerf_sample_outputs& so = outputs_of(p);
        CompositeArgs c{};
        c.rays = a->rays; c.ray_stride = a->ray_stride;
        c.raw4 = raw_of(p); c.z = depths_of(p); c.n_rays = N; c.S = p.S; c.n_importance = p.final ? 0 : I;
        c.lindisp = a->lindisp; c.white_bkgd = a->white_bkgd; c.noise = fine ? a->noise_fine : a->noise_coarse;
        c.vis = so.visibility_weights; c.alpha = so.opacity_alpha;
        if (p.final) {
            c.rgb = a->rgb_map; c.disp = a->disp_map; c.acc = a->acc_map; c.z_user = a->z_vals;
            if (plan.surface) { c.bent4 = bent4_ws; c.surf_pts = a->surface_pts; c.surf_rig = a->surface_rigidity; c.med_idx = a->median_index; }
        } else {
            // rgb0/disp0/acc0 are optional for the caller but the kernel always writes them: park them in raw_f
            // (not yet written) when the caller passed NULL.
            c.u = a->u_fine;
            c.rgb = a->rgb0 ? a->rgb0 : raw_f; c.disp = a->disp0 ? a->disp0 : raw_f + (size_t)N * 3; c.acc = a->acc0 ? a->acc0 : raw_f + (size_t)N * 4;
            c.z_std = a->z_std; c.z_out = z_fine;
            // split-bender path: the coarse samples' bent points move to their rows among the merged depths, the new samples are listed for the bender
            if (plan.split) { c.split_bent_in = bent_c; c.split_bent_out = bent4_ws; c.z_new = z_new; c.rank_new = rank_new; }
        }
        return c;
    }
    // the network kernel of the pass; `c` (its compositing arguments) becomes the kernel's epilogue when the plan says so -- the pass' raw array
    // (16 B per sample written and read back) then never exists
    hipError_t network_step(const PassPlan& p, const CompositeArgs& c) {
        const bool fused = p.comp != CompStep::Launch;
        const ImageDev& im = m->img[p.image];
        const nrnerf_sample_outputs& so = outputs_of(p);
        const float* const pts = given_pts ? given_pts : ((p.bend == BendStep::Compiled || p.bend == BendStep::Program) ? points_of(p) : nullptr);      // ready-made points
        // without them the kernel reports the points it evaluates where a later step reads them: the surface reduction, the split fine pass
        float* const pts_out = (!pts && (p.final ? plan.surface : plan.split)) ? points_of(p) : nullptr;
        float* const raw4 = fused ? nullptr : raw_of(p);
        float* const raw_out = p.final ? a->raw : nullptr;
        CompositeArgs fuse = fused ? c : CompositeArgs{};
        fuse.raw4 = nullptr;
        const nrnerf_model::Ev ev = work(p.net_slot, p.name, im, p.S);
        switch (p.net) {
        case NetFamily::NetBender: case NetFamily::NetTrunk: case NetFamily::NetX16: {
            NetArgs n{};
            n.rays = a->rays; n.ray_stride = a->ray_stride; n.latents = a->latents; n.lat_stride = a->latent_stride;
            n.z = depths_of(p); n.lindisp = a->lindisp; n.pts4 = pts; n.n_rays = N; n.S = p.S;
            n.wstream = im.stream; n.bias = im.bias;
            n.raw4 = raw4; n.raw_out = raw_out; n.raw_ch = im.output_ch; n.bent4 = pts_out;
            n.ex = sample_out(so); n.knobs = kn; n.fuse_on = fused; n.fuse = fuse;
            return timed(ev, [&] {
                if (p.net != NetFamily::NetX16) return launch_net(m->precision, p.net == NetFamily::NetBender, m->views, p.dispatch, n, m->num_cus, stream);
                n.work_counter = counter(p.trunk_counter, (size_t)16 * BEND_COUNTERS_PER_LAUNCH * 2 + 16 * p.which);
                n.no_resident = (a->flags & NRNERF_RENDER_NO_RESIDENT_SLICE) ? 1 : 0;
                if (x16_takes_resident(m->precision, p.dispatch, m->views, n)) {      // (the launcher's own rule; the display name stays)
                    std::lock_guard<std::mutex> g(m->prof_mu);
                    ++m->resident_launches[p.net_slot];
                }
                return launch_net_x16(m->precision, p.dispatch, m->views, n, m->num_cus, stream);
            });
        }
        case NetFamily::Gx16: {
            const GxMeta& gm = im.gx;
            GxArgs x{};
            x.pts4 = pts; x.raw4 = raw4; x.raw_out = raw_out; x.raw_ch = im.output_ch;
            x.n_rays = N; x.S = p.S; x.wstream = im.stream; x.bias = im.bias;
            x.depth = gm.depth; x.skip = gm.skip; x.L = gm.L; x.n_bias_tiles = gm.n_bias_tiles; x.LV = gm.LV;
            x.fuse_on = fused; x.fuse = fuse;
            return timed(ev, [&] { return launch_gx16(m->precision, p.dispatch, gm.views != 0, x, m->num_cus, stream); });
        }
        case NetFamily::Gen: {
            GenArgs g = im.prog;
            g.rays = a->rays; g.ray_stride = a->ray_stride; g.latents = a->latents; g.lat_stride = a->latent_stride;
            g.z = depths_of(p); g.lindisp = a->lindisp; g.n_rays = N; g.S = p.S;
            g.pts4 = pts; g.dirs_from_pts = (pts && m->views && m->has_bend) ? 1 : 0;      // (ready-made points without a bender -- nrnerf_query -- keep the rays' directions)
            g.wstream = im.stream; g.bias = im.bias;
            g.raw4 = raw4; g.raw_out = raw_out; g.raw_ch = im.output_ch;
            g.bent4 = pts ? const_cast<float*>(pts) : pts_out;          // with a bender: read (removal knob); without: written (points of the pass)
            g.knobs = kn;
            if (!pts) g.ex = sample_out(so);                             // without a bender the network kernel reports the points
            return run_program(ev, g);
        }
        case NetFamily::GenExact: {
            // exact Jacobian view directions (rnh:291-294, 358-385): J d of every sample from the bender's divergence kernel in ray mode
            // (value + tangent chain, fp32), then the network program on the per-sample directions (its training instantiation takes
            // them; nothing is saved)
            BendDivArgs t{};
            t.latents = a->latents; t.lat_stride = a->latent_stride; t.m = (long long)N * p.S;
            t.wstream = m->bend_train_fwd.stream; t.bias = m->bend_train_fwd.bias;
            t.knobs.has_cutoff = kn.has_cutoff; t.knobs.cutoff = kn.cutoff; t.knobs.has_scaling = kn.has_scaling; t.knobs.scaling = kn.scaling;
            t.rays = a->rays; t.ray_stride = a->ray_stride; t.zr = depths_of(p); t.S = p.S; t.lindisp = a->lindisp; t.dirs_out = jdirs;
            const bool b16 = m->precision != NRNERF_PREC_F32;
            const hipError_t je = (m->gen_compiled_bender == 0) ? launch_bend_div_fwd_a0(t, m->num_cus, stream, b16) : launch_bend_div_fwd_a1(t, m->num_cus, stream, b16);
            if (je != hipSuccess) return je;
            GenArgs g = im.prog;
            g.mode = 1;
            g.rays = pts; g.ray_stride = 0; g.latents = nullptr; g.lat_stride = 0;
            g.z = nullptr; g.lindisp = 0; g.n_rays = N; g.S = p.S;
            g.pts4 = pts; g.dirs_from_pts = 0; g.dirs = jdirs;
            g.wstream = im.stream; g.bias = im.bias;
            g.raw4 = raw4; g.raw_out = raw_out; g.raw_ch = im.output_ch; g.bent4 = const_cast<float*>(pts);        // (read: the removal knob, rnh:308-311)
            g.save = nullptr; g.mask = nullptr; g.save_stride = 0; g.save_w = 0;
            g.knobs = kn;
            return timed(ev, [&] { return launch_generic_train(m->precision, g, m->num_cus, stream); });
        }
        }
        return hipErrorUnknown;
    }
    int run_pass(const PassPlan& p) {
        if ((p.bend == BendStep::Compiled || p.bend == BendStep::Program) && bender_step(p) != hipSuccess) return NRNERF_ERR_HIP;
        const CompositeArgs c = composite_args(p);
        if (network_step(p, c) != hipSuccess) return NRNERF_ERR_HIP;
        if (p.comp != CompStep::Launch) return NRNERF_OK;      // (the network kernel took it as its epilogue)
        const nrnerf_model::Ev ev{p.net_slot + 1, nullptr, nullptr, 0, 0, "composite_kernel"};
        return status_of(timed(ev, [&] { return launch_composite(c, stream); }));
    }
};
}  // namespace
extern "C" {

int nrnerf_render(const nrnerf_model* m, const nrnerf_render_args* a, void* hip_stream) try {
    if (!m || !a || a->struct_size != sizeof(nrnerf_render_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 2 || a->n_importance < 0) return NRNERF_ERR_INVALID;
    if (a->n_samples > NRNERF_MAX_SAMPLES || a->n_samples + a->n_importance > NRNERF_MAX_SAMPLES) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || a->ray_stride < 8 || !a->rgb_map || !a->disp_map || !a->acc_map) return NRNERF_ERR_INVALID;
    if (m->needs_latents && (!a->latents || a->latent_stride < 0)) return NRNERF_ERR_INVALID;
    if (m->views && (!m->has_bend || m->exact) && a->ray_stride < 11) return NRNERF_ERR_INVALID;   // needs the unit view directions
    const size_t need = nrnerf_workspace_bytes(m, a->n_rays, a->n_samples, a->n_importance);      // (= WorkspaceLayout::total below)
    if (!a->workspace || a->workspace_bytes < need || ((uintptr_t)a->workspace & 255)) return NRNERF_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)hip_stream;
    // launches go to the model's device whatever the calling thread's current device is (restored on every exit path)
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    const WorkspaceLayout lay(a->n_rays, a->n_samples, a->n_importance, m->generic && m->exact);
    if ((a->u_fine || a->noise_fine) && a->n_importance == 0) return NRNERF_ERR_INVALID;
    const RenderPlan plan = plan_render(*m, *a);
    RenderCall call(m, a, plan, lay, stream);
    if (plan.counters_first) (void)call.counter(true, 0);      // (the memset node ahead of every timed launch)
    // ---- stratified jitter of the coarse depths (perturb > 0): both coarse kernels then read explicit depths
    if (a->u_coarse) {
        JitterArgs ja{a->rays, a->ray_stride, a->u_coarse, a->n_rays, a->n_samples, a->lindisp, call.z_coarse};
        if (launch_zjitter(ja, stream) != hipSuccess) return NRNERF_ERR_HIP;
        call.zc = call.z_coarse;
    }
    const int rc = call.run_pass(plan.coarse);
    return (rc == NRNERF_OK && plan.fine.exists) ? call.run_pass(plan.fine) : rc;
} NRN_CATCH

}  // extern "C"
namespace {
// ---- nrnerf_query: the networks on caller-given points (run_network, train.py:57-105).  plan_query decides (no HIP call), QueryCall launches:
// a packing step, a bender step (the point-source stand-alone bender), RenderCall's network step, the detail tensors.
constexpr unsigned QUERY_FLAGS = NRNERF_RENDER_NO_X16 | NRNERF_RENDER_BENDER_32X32 | NRNERF_RENDER_FIXED_SHARES;
struct QueryPlan {
    int status = NRNERF_OK;
    PassPlan pass;                 // bend: None or Compiled; net: NetX16 / NetTrunk / Gx16 / Gen; comp unused (nothing is composited)
    bool bend_x16 = false;
    // A compiled view-dependent head WITHOUT a bender: its trunk-only kernels take the direction of ready-made points from the points' finite
    // differences (the split path's contract), which is not what run_network computes here (the row's viewdirs, train.py:73-76).  Such a query runs
    // on ray records instead -- one record per POINT (origin = the point, direction 0, near = far = 0, the row's unit direction), a "ray" of one
    // sample at depth 0: the kernel's o + d z is the point itself.
    bool per_point = false;
    bool point_latents = false;    // ... with the row's latent code copied per point (time-conditioned baseline)
};
// the workspace of a query: 256-byte aligned slots, as WorkspaceLayout
struct QueryLayout {
    size_t raw4, pts4, records, point_records, point_latents, counters, total = 0;
    QueryLayout(const nrnerf_model& m, const QueryPlan& q, int n_rows, int n_samples) {
        const size_t N = (size_t)n_rows, M = N * (size_t)n_samples;
        auto slot = [&](size_t bytes, bool present = true) {
            const size_t at = total;
            if (present) total += align_up(bytes, 256);
            return at;
        };
        raw4 = slot(M * 4 * sizeof(float));                          // rgb + sigma rows of the network kernel
        pts4 = slot(M * 4 * sizeof(float));                          // the points of the pass: packed input, or bent point + rigidity
        records = slot(N * 11 * sizeof(float));                      // a ray record per row: zeros + the unit direction
        point_records = slot(M * 11 * sizeof(float), q.per_point);
        point_latents = slot(M * (size_t)m.latent_size * sizeof(float), q.point_latents);
        counters = slot(BEND_COUNTER_BYTES);
    }
};

QueryPlan plan_query(const nrnerf_model& m, int which, int N, int S, unsigned flags) {
    QueryPlan q;
    PassPlan& p = q.pass;
    auto flag = [&](unsigned f) { return (flags & f) != 0; };
    const bool dynamic = !flag(NRNERF_RENDER_FIXED_SHARES);
    p.exists = true; p.final = true; p.which = which; p.S = S;
    p.net_slot = 2 * which; p.bend_slot = 5 - which;
    const bool own = which && !m.fine_is_coarse;            // (one network for both passes: `which` = 1 runs on the coarse images)
    if (m.exact) { q.status = NRNERF_ERR_UNSUPPORTED; return q; }       // exact Jacobian directions: fused / divergence kernels only
    if ((long long)N * S >= (1ll << 31) || !block_index_fits(N, S)) { q.status = NRNERF_ERR_UNSUPPORTED; return q; }
    if (m.has_bend) {
        // the point-source stand-alone bender: a compiled shape with its image in the handle
        if (!(m.generic ? m.gen_compiled_bender >= 0 : m.split_ok != 0) || !m.bend_only.stream) { q.status = NRNERF_ERR_UNSUPPORTED; return q; }
        p.bend = BendStep::Compiled; p.bend_n = p.bend_stride = S;
        q.bend_x16 = m.bend_x16.stream && !flag(NRNERF_RENDER_BENDER_32X32 | NRNERF_RENDER_NO_X16);
        p.bend_dynamic = q.bend_x16 && dynamic && m.num_cus <= BEND_COUNTERS_PER_LAUNCH;
    }
    const bool rows_give_dirs = m.views && !m.has_bend;     // the row's viewdirs, not finite differences
    if (m.generic) {
        const ImageDev& gx = m.img[own ? IMG_GX_FINE : IMG_GX_COARSE];
        p.net = NetFamily::Gen; p.image = own ? IMG_GEN_FINE : IMG_GEN_COARSE; p.name = "gen_kernel";
        if (gx.stream && !flag(NRNERF_RENDER_NO_X16) && !rows_give_dirs) {
            p.net = NetFamily::Gx16; p.image = own ? IMG_GX_FINE : IMG_GX_COARSE; p.dispatch = gx.gx.wc; p.name = "gx16_kernel";
        }
        return q;
    }
    if (m.has_bend) {
        // (a handle without a fine network keeps its only 16x16x32 trunk image in the fine slot, pack_images)
        const ImageSlot x16_image = (which || m.fine_is_coarse) ? IMG_FINE_TRUNK_X16 : IMG_COARSE_TRUNK_X16;
        const bool x16 = !flag(NRNERF_RENDER_NO_X16) && m.img[x16_image].stream;
        p.net = x16 ? NetFamily::NetX16 : NetFamily::NetTrunk; p.dispatch = trunk_arch(m.arch_id); p.trunk_counter = x16 && dynamic;
        p.image = x16 ? x16_image : (which ? IMG_FINE_TRUNK : IMG_COARSE_TRUNK);
        p.name = x16 ? "net_kernel_x16" : "net_kernel (trunk only)";
        return q;
    }
    p.net = NetFamily::NetTrunk; p.image = own ? IMG_FINE : IMG_COARSE; p.dispatch = m.arch_id; p.name = "net_kernel";
    if (rows_give_dirs) {
        q.per_point = true; q.point_latents = m.needs_latents != 0;
        p.S = 1; p.name = "net_kernel (a record per point)";
    }
    return q;
}
}  // namespace
extern "C" {

size_t nrnerf_query_workspace_bytes(const nrnerf_model* m, int32_t which, int32_t n_rows, int32_t n_samples) {
    if (!m || (which != 0 && which != 1) || n_rows <= 0 || n_samples <= 0 || n_samples > NRNERF_MAX_SAMPLES) return 0;
    const QueryPlan q = plan_query(*m, which, n_rows, n_samples, 0);
    return q.status == NRNERF_OK ? QueryLayout(*m, q, n_rows, n_samples).total : 0;
}

int nrnerf_query(const nrnerf_model* m, const nrnerf_query_args* a, void* hip_stream) try {
    if (!m || !a || a->struct_size != sizeof(nrnerf_query_args)) return NRNERF_ERR_INVALID;
    if (a->which != 0 && a->which != 1) return NRNERF_ERR_INVALID;
    if (a->n_rows < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->point_stride < 3 || a->latent_stride < 0) return NRNERF_ERR_INVALID;
    if (a->flags & ~QUERY_FLAGS) return NRNERF_ERR_INVALID;
    const nrnerf_sample_outputs& d = a->details;
    if (d.visibility_weights || d.opacity_alpha) return NRNERF_ERR_INVALID;          // compositing's tensors: nothing is composited here
    if (a->n_rows == 0) return NRNERF_OK;
    if (!a->points || !a->raw) return NRNERF_ERR_INVALID;
    if (m->needs_latents && !a->latents) return NRNERF_ERR_INVALID;
    if (!m->has_bend && (d.unmasked_offsets || d.masked_offsets || d.rigidity_mask)) return NRNERF_ERR_INVALID;
    if (m->views && !m->has_bend && !a->viewdirs) return NRNERF_ERR_INVALID;
    if (m->views && m->has_bend && !m->exact && a->n_samples == 1) return NRNERF_ERR_INVALID;      // no neighbour to difference against (rnh:339-351)
    const int N = a->n_rows, S = a->n_samples;
    const QueryPlan q = plan_query(*m, a->which, N, S, a->flags);
    if (q.status != NRNERF_OK) return q.status;
    const PassPlan& p = q.pass;
    const ImageDev& im = m->img[p.image];
    if (!im.stream) return NRNERF_ERR_UNSUPPORTED;
    if (a->raw_ch != im.output_ch) return NRNERF_ERR_INVALID;
    const QueryLayout lay(*m, q, N, S);
    if (!a->workspace || a->workspace_bytes < lay.total || ((uintptr_t)a->workspace & 255)) return NRNERF_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)hip_stream;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    char* const ws = (char*)a->workspace;
    float* const raw4 = (float*)(ws + lay.raw4);
    float* const pts4 = (float*)(ws + lay.pts4);
    float* const records = (float*)(ws + lay.records);
    const long long M = (long long)N * S;

    // ---- the inputs in the kernels' layouts: a ray record per row (zeros + the unit direction), and -- no bender -- the points as rows of four
    QueryPackArgs pk{};
    pk.points = a->points; pk.stride = a->point_stride; pk.viewdirs = a->viewdirs; pk.n_rows = N; pk.S = S;
    pk.init_pts = d.initial_input_pts; pk.records = records;
    if (!m->has_bend) { pk.pts4 = pts4; pk.in_pts = d.input_pts; }
    if (q.per_point) {
        pk.point_records = (float*)(ws + lay.point_records);
        if (q.point_latents) { pk.latents_out = (float*)(ws + lay.point_latents); pk.latents = a->latents; pk.lat_stride = a->latent_stride; pk.lat = m->latent_size; }
    }
    if (launch_query_pack(pk, stream) != hipSuccess) return NRNERF_ERR_HIP;

    // the call as a render call of one pass: RenderCall's network step, profile records and work counters
    nrnerf_render_args r{};
    r.struct_size = sizeof(r);
    r.n_rays = N; r.n_samples = S; r.rays = records; r.ray_stride = 11; r.latents = a->latents; r.latent_stride = a->latent_stride;
    r.has_rigidity_cutoff = a->has_rigidity_cutoff; r.rigidity_cutoff = a->rigidity_cutoff;
    r.has_test_time_scaling = a->has_test_time_scaling; r.test_time_scaling = a->test_time_scaling;
    r.has_removal_threshold = m->has_bend ? a->has_removal_threshold : 0; r.removal_threshold = a->removal_threshold;
    r.detailed_output = a->detailed_output; r.raw = a->raw; r.flags = a->flags;
    if (q.per_point) {
        r.n_rays = (int32_t)M; r.n_samples = 1; r.rays = pk.point_records;
        if (q.point_latents) { r.latents = pk.latents_out; r.latent_stride = m->latent_size; }
    }
    RenderPlan rp;
    rp.generic = m->generic != 0; rp.bend_x16 = q.bend_x16;
    RenderCall call(m, &r, rp, stream, raw4, pts4, (unsigned*)(ws + lay.counters));
    if (p.bend_dynamic) (void)call.counter(true, 0);           // (the memset node ahead of every timed launch)
    if (!q.per_point && !m->has_bend) call.given_pts = pts4;

    if (p.bend == BendStep::Compiled) {
        const ImageDev& bi = q.bend_x16 ? m->bend_x16 : m->bend_only;
        BendPointArgs b{};
        b.b.latents = a->latents; b.b.lat_stride = a->latent_stride; b.b.n_rays = N; b.b.n_per_ray = S; b.b.out_stride = S;
        b.b.wstream = bi.stream; b.b.bias = bi.bias; b.b.bent4 = pts4; b.b.knobs = call.kn;
        b.b.work_counter = call.counter(p.bend_dynamic, (size_t)16 * BEND_COUNTERS_PER_LAUNCH * p.which);
        b.src.points = a->points; b.src.stride = a->point_stride; b.src.unmasked = d.unmasked_offsets; b.src.masked = d.masked_offsets;
        const hipError_t e = call.timed(call.work(p.bend_slot, q.bend_x16 ? "bend_kernel_x16 (point source)" : "bend_kernel (point source)", bi, S), [&] {
            return q.bend_x16 ? launch_bend_points_x16(bender_arch_of(m), b, m->num_cus, stream)
                              : launch_bend_points(m->precision, bender_arch_of(m), b, m->num_cus, stream);
        });
        if (e != hipSuccess) return NRNERF_ERR_HIP;
    }
    if (call.network_step(p, CompositeArgs{}) != hipSuccess) return NRNERF_ERR_HIP;
    if (m->has_bend) {
        // input_pts / rigidity_mask are bent4's columns; the removal knob (only under detailed_output, rnh:308-311) on the caller's raw rows
        QueryUnpackArgs u{};
        u.bent4 = pts4; u.n = M; u.in_pts = d.input_pts; u.rigidity = d.rigidity_mask;
        u.raw = a->raw; u.raw_ch = a->raw_ch; u.has_removal = a->detailed_output && a->has_removal_threshold; u.removal = a->removal_threshold;
        if ((u.in_pts || u.rigidity || u.has_removal) && launch_query_unpack(u, stream) != hipSuccess) return NRNERF_ERR_HIP;
    }
    return NRNERF_OK;
} NRN_CATCH

int nrnerf_grid_points(const float min_point[3], const float max_point[3], int32_t gx, int32_t gy, int32_t gz, int64_t first_row,
                       int32_t n_rows, float* pts4, void* hip_stream) try {
    if (!min_point || !max_point || gx < 1 || gy < 1 || gz < 1 || first_row < 0 || n_rows < 0) return NRNERF_ERR_INVALID;
    if (first_row + n_rows > (int64_t)gy * gz) return NRNERF_ERR_INVALID;
    if (n_rows == 0) return NRNERF_OK;
    if (!pts4) return NRNERF_ERR_INVALID;
    GridArgs g{};
    for (int c = 0; c < 3; ++c) { g.lo[c] = min_point[c]; g.hi[c] = max_point[c]; }
    g.g[0] = gx; g.g[1] = gy; g.g[2] = gz; g.first_row = first_row; g.n_rows = n_rows; g.pts4 = pts4;
    return on_owner_of(pts4, [&] { return status_of(launch_grid_points(g, (hipStream_t)hip_stream)); });
} NRN_CATCH

int nrnerf_field_from_raw(const float* raw, int32_t raw_ch, int64_t n, float* sigma, uint8_t* rgb8, void* hip_stream) try {
    if (n < 0 || raw_ch < 4) return NRNERF_ERR_INVALID;
    if (n == 0 || (!sigma && !rgb8)) return NRNERF_OK;
    if (!raw) return NRNERF_ERR_INVALID;
    return on_owner_of(raw, [&] { return status_of(launch_field_from_raw(raw, raw_ch, n, sigma, rgb8, (hipStream_t)hip_stream)); });
} NRN_CATCH

int nrnerf_generate_rays(const nrnerf_camera* cam, float near_plane, float far_plane, float* rays_out,
                         int32_t ray_stride, void* hip_stream) try {
    if (!cam || !rays_out || (ray_stride != 8 && ray_stride != 11)) return NRNERF_ERR_INVALID;
    if (cam->height <= 0 || cam->width <= 0 || cam->focal_x == 0.0f || cam->focal_y == 0.0f) return NRNERF_ERR_INVALID;
    RayGenArgs a{};
    std::memcpy(a.c2w, cam->c2w, sizeof(a.c2w));
    a.fx = cam->focal_x; a.fy = cam->focal_y; a.cx = cam->center_x; a.cy = cam->center_y;
    a.H = cam->height; a.W = cam->width; a.near = near_plane; a.far = far_plane;
    a.rays = rays_out; a.ray_stride = ray_stride;
    // the launch goes to the device that owns rays_out, whatever the calling thread's current device is (as nrnerf_render)
    return on_owner_of(rays_out, [&] { return status_of(launch_raygen(a, (hipStream_t)hip_stream)); });
} NRN_CATCH

int nrnerf_sample_depths(const float* rays, int32_t ray_stride, const float* uniforms, int32_t n_rays, int32_t n_samples,
                         int32_t lindisp, float* z_out, void* hip_stream) try {
    if (!rays || !z_out || ray_stride < 8 || n_rays < 0 || n_samples < 2 || n_samples > NRNERF_MAX_SAMPLES) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    const JitterArgs j{rays, ray_stride, uniforms, n_rays, n_samples, lindisp, z_out};
    return on_owner_of(z_out, [&] { return status_of(launch_zjitter(j, (hipStream_t)hip_stream)); });
} NRN_CATCH
int nrnerf_sample_depths_points(const float* rays, int32_t ray_stride, const float* uniforms, int32_t n_rays, int32_t n_samples,
                                int32_t lindisp, float* z_out, float* points_out, void* hip_stream) try {
    if (!rays || !z_out || !points_out || ray_stride < 8 || n_rays < 0 || n_samples < 2 || n_samples > NRNERF_MAX_SAMPLES) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    const SamplePointsArgs j{rays, ray_stride, uniforms, n_rays, n_samples, lindisp, z_out, points_out};
    return on_owner_of(z_out, [&] { return status_of(launch_sample_points(j, (hipStream_t)hip_stream)); });
} NRN_CATCH

int nrnerf_profile_begin(nrnerf_model* m) try {
    if (!m) return NRNERF_ERR_INVALID;
    std::lock_guard<std::mutex> g(m->prof_mu);
    for (auto& e : m->prof_events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    m->prof_events.clear();
    for (int& n : m->resident_launches) n = 0;
    m->prof_on = true;
    return NRNERF_OK;
} NRN_CATCH

int nrnerf_resident_launches(const nrnerf_model* m, int32_t out[6]) try {
    if (!m || !out) return NRNERF_ERR_INVALID;
    std::lock_guard<std::mutex> g(m->prof_mu);
    for (int i = 0; i < NRNERF_NUM_KERNELS; ++i) out[i] = m->resident_launches[i];
    return NRNERF_OK;
} NRN_CATCH

size_t nrnerf_trunk_kernel_lds_bytes(int32_t precision, int32_t n_samples, int32_t fused, int32_t resident) {
    const int prec = precision == NRNERF_PREC_BF16 ? PREC_BF16 : (precision == NRNERF_PREC_F16 ? PREC_F16 : -1);
    if (prec < 0 || n_samples < 1 || n_samples > NRNERF_MAX_SAMPLES) return 0;
    return x16_lds_request(prec, 0, false, n_samples, fused != 0, false, resident != 0);
}

int nrnerf_profile_end(nrnerf_model* m, nrnerf_profile* out) try {
    if (!m || !out) return NRNERF_ERR_INVALID;
    std::lock_guard<std::mutex> g(m->prof_mu);
    m->prof_on = false;
    std::memset(out, 0, sizeof(*out));
    int rc = NRNERF_OK;
    for (auto& e : m->prof_events) {
        float ms = 0.f;
        if (hipEventSynchronize(e.b) != hipSuccess || hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) rc = NRNERF_ERR_HIP;
        out->ms[e.kernel] += ms;
        out->launches[e.kernel] += 1;
        out->flops[e.kernel] += e.flops;
        out->mfma_flops[e.kernel] += e.mfma;
        if (e.name) std::snprintf(out->kernel_name[e.kernel], sizeof(out->kernel_name[e.kernel]), "%s", e.name);
        (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b);
    }
    m->prof_events.clear();
    return rc;
} NRN_CATCH

}  // extern "C"
