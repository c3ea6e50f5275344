// nrnerf_api.cpp -- C ABI of libnrnerf_hip.so (include/nrnerf.h): model lifetime (upload / refresh / free of the weight images
// nrnerf_pack.cpp builds), workspace carving, kernel sequencing.
//
// Kernel sequence of one nrnerf_render call (reference render_rays, train.py:792-980):
//   K0  network kernel, coarse weights, z = linspace(near, far, S)        -> raw_c [N,S,4]
//   K1  composite (+ sample_pdf + merge + z_std when I > 0)               -> rgb0/disp0/acc0 or final; z_fine [N,S+I]
//   K2  network kernel, fine weights, z = z_fine                          -> raw_f [N,S+I,4]
//   K3  composite                                                         -> rgb/disp/acc
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "nrnerf.h"
#include "nrnerf_kernels.h"
#include "nrnerf_aux.h"
#include "nrnerf_x16_api.h"
#include "nrnerf_bend_x16_plan.h"
#include "nrnerf_loss.h"
#include "nrnerf_optim.h"
#include "nrnerf_gen_train.h"
#include "nrnerf_gx16_bwd_api.h"
#include "nrnerf_gx16_plan.h"
#include "nrnerf_plan.h"
#include "nrnerf_pack.h"

// the run-time-parameterised kernel's TRAINING instantiations (nrnerf_generic.hip; the rendering ones: launch_generic, nrnerf_kernels.h)
namespace nrn { hipError_t launch_generic_train(int precision, const GenArgs& a, int num_cus, hipStream_t stream); }
using namespace nrn;

#ifndef NRN_WGRAD_SYNC_DEFAULT
// pairs of blocks between workgroup barriers in trunk_wgrad (WgradArgs::sync_every; env NRNERF_WGRAD_SYNC, 0 = never).  Measured
// at 16 384 rays (tools/experiments/wgrad_sync_sweep.sh): never 3.30 ms per launch, every 2 pairs 2.76, 8: 2.54, 32: 2.55, 128: 2.82,
// 512: 3.09 -- the waves that share a fragment stay within L2's reach of each other, the barrier itself costs nothing because
// the loads already requested stay in flight across it.
#define NRN_WGRAD_SYNC_DEFAULT 16
#endif

// Nothing throws across the C ABI (include/nrnerf.h): every extern "C" body is a function-try-block that turns
// std::bad_alloc (the packer's std::vector growth) into NRNERF_ERR_NOMEM and anything else -- the packer's
// plan-consistency checks throw std::logic_error -- into NRNERF_ERR_INTERNAL.
#define NRN_CATCH catch (const std::bad_alloc&) { return NRNERF_ERR_NOMEM; } catch (...) { return NRNERF_ERR_INTERNAL; }

namespace {

struct PassDev {
    void* stream = nullptr;
    float* bias = nullptr;
    size_t stream_bytes = 0, bias_floats = 0;
    double algo_flops_per_sample = 0;      // 2 * MAC
    double mfma_flops_per_sample = 0;      // issued, incl. padding
    int output_ch = 4;
    // device copies of the packer's source maps (nrnerf_model_update_device); null when not recorded
    int32_t* src = nullptr; int32_t* bias_src = nullptr; uint8_t* fmt = nullptr;
    size_t n_elems = 0;
};

// a packed weight image (Image, nrnerf_pack.h) on the device
struct ImageDev : PassDev { GenArgs prog{}; GxMeta gx{}; };

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

// makes `want` the calling thread's current device for the lifetime of the guard (restored on every exit path)
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int want) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; prev = -1; return; }
        if (prev != want && hipSetDevice(want) != hipSuccess) ok = false;
        if (prev == want) prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

struct nrnerf_model : ModelTraits {
    // `fine` / `gen_fine` resolve to the coarse network's image when the model has no fine network (one network for both passes)
    explicit nrnerf_model(const ModelTraits& t)
        : ModelTraits(t), fine(img[t.fine_is_coarse ? IMG_COARSE : IMG_FINE]), gen_fine(img[t.fine_is_coarse ? IMG_GEN_COARSE : IMG_GEN_FINE]) {}
    int device = 0, num_cus = 0;
    ImageDev img[IMG_COUNT];      // every packed weight image, by slot (pack_images says which exist); the names below are what the launch code uses
    ImageDev &coarse = img[IMG_COARSE], &fine;
    // split-bender path (bender; finite-difference view directions if any): the fine network WITHOUT the bender layers (its input points
    // come from the stand-alone bender kernel) and the bender + rigidity layers alone
    ImageDev &fine_trunk = img[IMG_FINE_TRUNK], &coarse_trunk = img[IMG_COARSE_TRUNK], &bend_only = img[IMG_BEND_ONLY];
    // the fine network's trunk once more, packed for the 16x16x32 kernel (nrnerf_net_x16.h): what the split-bender path's fine pass
    // runs when the call asks for no detail outputs
    ImageDev &fine_trunk_x16 = img[IMG_FINE_TRUNK_X16], &coarse_trunk_x16 = img[IMG_COARSE_TRUNK_X16];
    ImageDev &bend_x16 = img[IMG_BEND_X16];             // the bender + rigidity MLPs packed for the 16x16x32 stand-alone bender ("bf16" mode)
    // training (nrnerf_train.h): transposed trunk weights of both networks; train_ok: see training_eligible, fp32 or bf16
    ImageDev &coarse_bwd = img[IMG_COARSE_BWD], &fine_bwd = img[IMG_FINE_BWD];
    // view-dependent head / time-conditioned baseline: bender-less forward images for trunk_fwd_train (with both branches of the head /
    // without the latent columns)
    ImageDev &coarse_train = img[IMG_COARSE_TRAIN], &fine_train = img[IMG_FINE_TRAIN];
    // training of the ray bender (nrnerf_train_bend.h): its layers alone in fp32 (whatever the model's precision) and
    // their transposes; bend_train_ok: train_ok and a bender
    ImageDev &bend_train_fwd = img[IMG_BEND_TRAIN_FWD], &bend_train_bwd = img[IMG_BEND_TRAIN_BWD];
    // generic architecture (nrnerf_generic.h): layer programs (ImageDev::prog) instead of compiled plans
    ImageDev &gen_bend = img[IMG_GEN_BEND], &gen_coarse = img[IMG_GEN_COARSE], &gen_fine;
    // the trunks of a generic model packed for the width-class 16x16x32 kernel (nrnerf_gx16.h; ImageDev::gx): 16-bit modes
    ImageDev &gx_coarse = img[IMG_GX_COARSE], &gx_fine = img[IMG_GX_FINE];
    // training of a generic model with a plain head (fp32 / bf16): the backward-data programs (transposed weights); the forward is
    // gen_coarse / gen_fine run with GenArgs::save set
    ImageDev &gen_coarse_bwd = img[IMG_GEN_COARSE_BWD], &gen_fine_bwd = img[IMG_GEN_FINE_BWD];
    ImageDev &gx_coarse_bwd = img[IMG_GX_COARSE_BWD], &gx_fine_bwd = img[IMG_GX_FINE_BWD];          // backward-data programs of the width-class trunks (nrnerf_gx16_bwd.h), when gx16_trainable
    int64_t flat_floats = 0;      // length of the flat parameter vector nrnerf_model_update_device expects
    unsigned* adam_barrier = nullptr;   // two words of device memory: the grid barrier of nrnerf_adam_step (nrnerf_optim.hip)
    // profiling (guarded; the render path itself is otherwise read-only on the handle)
    mutable std::mutex prof_mu;
    mutable bool prof_on = false;
    struct Ev { int kernel; hipEvent_t a, b; double flops, mfma; const char* name; };
    mutable std::vector<Ev> prof_events;
};

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

namespace {
// which compiled bender shape (0: 5 x 64, 1: 7 x 64) the bender's training kernels run: the handle's architecture, or -- a generic handle --
// the compiled shape its bender happens to have (the reference's hard-coded one next to an odd trunk, rnh:406-407)
int bender_arch_of(const nrnerf_model* m) { return m->generic ? m->gen_compiled_bender : bender_arch(m->arch_id); }
}  // namespace
int nrnerf_model_trains_bender(const nrnerf_model* m) { return m ? (m->bend_train_ok ? 1 : 0) : NRNERF_ERR_INVALID; }
int nrnerf_model_is_generic(const nrnerf_model* m) { return m ? (m->generic ? 1 : 0) : NRNERF_ERR_INVALID; }

}  // extern "C"
namespace {
int device_of(const void* ptr, int& dev);
// every packed image of the handle (weight stream + bias table) as segments of repack launches over `flat_params`; `emit(batch, last)` is
// called per full batch of REPACK_MAX_SEGMENTS and once for the last (possibly empty) one
template <class EMIT>
int repack_batches(nrnerf_model* m, const float* flat_params, EMIT&& emit) {
    for (const ImageDev& p : m->img)
        if (p.stream && !p.src) return NRNERF_ERR_UNSUPPORTED;          // (before anything is launched)
    RepackBatchArgs b{};
    b.flat = flat_params;
    auto add = [&](const int32_t* src, const uint8_t* fmt, void* dst, long long n) -> bool {
        if (n <= 0) return true;
        if (b.n_segments == REPACK_MAX_SEGMENTS) {
            if (!emit(b, false)) return false;
            b.n_segments = 0;
        }
        const int k = b.n_segments++;
        if (k == 0) b.block0[0] = 0;
        b.src[k] = src; b.fmt[k] = fmt; b.dst[k] = dst; b.n[k] = n;
        b.block0[k + 1] = b.block0[k] + (unsigned)((n + 255) / 256);
        return true;
    };
    for (const ImageDev& p : m->img) {
        if (!p.stream) continue;
        if (!add(p.src, p.fmt, p.stream, (long long)p.n_elems) || !add(p.bias_src, nullptr, p.bias, (long long)p.bias_floats)) return NRNERF_ERR_HIP;
    }
    return emit(b, true) ? NRNERF_OK : NRNERF_ERR_HIP;
}
}  // namespace
extern "C" {

int nrnerf_model_update_device(nrnerf_model* m, const float* flat_params, int64_t n_floats, void* hip_stream) try {
    if (!m || !flat_params || n_floats != m->flat_floats) return NRNERF_ERR_INVALID;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    hipStream_t stream = (hipStream_t)hip_stream;
    // every image (weight stream + bias table) as one segment of ONE launch
    return repack_batches(m, flat_params, [&](const RepackBatchArgs& b, bool) { return launch_repack_batch(b, stream) == hipSuccess; });
} NRN_CATCH

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
    else {
        if (device_of(a->step, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return NRNERF_ERR_HIP;
        num_cus = prop.multiProcessorCount; k.barrier = a->barrier;
    }
    if (!k.barrier) return NRNERF_ERR_INVALID;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (launch_adam(k, num_cus, stream) != hipSuccess) return NRNERF_ERR_HIP;
    if (!repack) return NRNERF_OK;
    // ... and every packed image from the updated parameters, right behind it on the same stream
    return repack_batches(m, a->flat_params, [&](const RepackBatchArgs& b, bool) { return launch_repack_batch(b, stream) == hipSuccess; });
} NRN_CATCH

namespace {
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
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    hipStream_t stream = (hipStream_t)hip_stream;
    float* parts = (float*)a->workspace;
    if (launch_tn_clear(parts, a->out_floats, kch, stream) != hipSuccess) return NRNERF_ERR_HIP;
    bool misaligned = false;
    TnKernelArgs k{};
    k.kch = kch; k.n_rows = a->n_rows; k.total = a->out_floats; k.partials = parts;
    auto flush = [&]() -> bool {
        if (k.n_sub == 0) return true;
        const hipError_t rc = launch_tn_products(k, a->is_bf16 == 0, stream);
        k.n_sub = 0;
        if (rc == hipErrorInvalidValue) misaligned = true;
        return rc == hipSuccess;
    };
    for (int j = 0; j < a->n_jobs; ++j) {
        const nrnerf_tn_job& jb = a->jobs[j];
        for (int o0 = 0; o0 < jb.wo; o0 += 256)
            for (int k0 = 0; k0 < jb.wi; k0 += 256) {
                if (k.n_sub == TN_MAX_SUBJOBS && !flush()) return misaligned ? NRNERF_ERR_INVALID : NRNERF_ERR_HIP;
                k.sub[k.n_sub++] = TnSubJob{jb.a, jb.b, jb.lda, jb.ldb, jb.wo, jb.wi, o0, k0, jb.ldo, (long long)jb.out_offset, (long long)jb.bias_offset};
            }
    }
    if (!flush()) return misaligned ? NRNERF_ERR_INVALID : NRNERF_ERR_HIP;
    return launch_tn_reduce(parts, a->out_floats, kch, a->out, stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

namespace {
int encoding_call(const nrnerf_encoding_args* a, bool backward, void* hip_stream) {
    if (!a || a->struct_size != sizeof(nrnerf_encoding_args) || a->n_rows < 0 || !a->src) return NRNERF_ERR_INVALID;
    if (a->n_rows == 0) return NRNERF_OK;
    int dev = 0;
    if (device_of(a->src, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    EncodingArgs e{a->src, a->src_stride, (long long)a->n_rows, a->n_freqs, a->enc, a->enc_cols, a->enc_is_bf16, a->codes, a->n_lat, a->rows_per_code,
                   a->d_enc0, a->d_enc1, a->d_enc_stride, a->d_src, a->d_src_stride};
    const hipError_t rc = launch_encoding_rows(e, backward, (hipStream_t)hip_stream);
    return rc == hipSuccess ? NRNERF_OK : (rc == hipErrorInvalidValue ? NRNERF_ERR_INVALID : NRNERF_ERR_HIP);
}
}  // namespace
int nrnerf_encoding_forward(const nrnerf_encoding_args* a, void* hip_stream) try { return encoding_call(a, false, hip_stream); } NRN_CATCH
int nrnerf_encoding_backward(const nrnerf_encoding_args* a, void* hip_stream) try { return encoding_call(a, true, hip_stream); } NRN_CATCH

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
        const float* const pts = (p.bend == BendStep::Compiled || p.bend == BendStep::Program) ? points_of(p) : nullptr;      // ready-made points
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
            g.pts4 = pts; g.dirs_from_pts = (pts && m->views) ? 1 : 0;
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
        return timed(ev, [&] { return launch_composite(c, stream); }) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
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
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, rays_out) != hipSuccess) { (void)hipGetLastError(); return NRNERF_ERR_INVALID; }
    if (attr.type != hipMemoryTypeDevice) return NRNERF_ERR_INVALID;
    DeviceGuard guard(attr.device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    return launch_raygen(a, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_sample_depths(const float* rays, int32_t ray_stride, const float* uniforms, int32_t n_rays, int32_t n_samples,
                         int32_t lindisp, float* z_out, void* hip_stream) try {
    if (!rays || !z_out || ray_stride < 8 || n_rays < 0 || n_samples < 2 || n_samples > NRNERF_MAX_SAMPLES) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, z_out) != hipSuccess) { (void)hipGetLastError(); return NRNERF_ERR_INVALID; }
    if (attr.type != hipMemoryTypeDevice) return NRNERF_ERR_INVALID;
    DeviceGuard guard(attr.device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    JitterArgs j{rays, ray_stride, uniforms, n_rays, n_samples, lindisp, z_out};
    return launch_zjitter(j, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH
int nrnerf_sample_depths_points(const float* rays, int32_t ray_stride, const float* uniforms, int32_t n_rays, int32_t n_samples,
                                int32_t lindisp, float* z_out, float* points_out, void* hip_stream) try {
    if (!rays || !z_out || !points_out || ray_stride < 8 || n_rays < 0 || n_samples < 2 || n_samples > NRNERF_MAX_SAMPLES) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, z_out) != hipSuccess) { (void)hipGetLastError(); return NRNERF_ERR_INVALID; }
    if (attr.type != hipMemoryTypeDevice) return NRNERF_ERR_INVALID;
    DeviceGuard guard(attr.device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    SamplePointsArgs j{rays, ray_stride, uniforms, n_rays, n_samples, lindisp, z_out, points_out};
    return launch_sample_points(j, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

namespace {
// the device that owns `ptr` (device memory): NRNERF_OK and `dev`, or NRNERF_ERR_INVALID
int device_of(const void* ptr, int& dev) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) { (void)hipGetLastError(); return NRNERF_ERR_INVALID; }
    if (attr.type != hipMemoryTypeDevice) return NRNERF_ERR_INVALID;
    dev = attr.device;
    return NRNERF_OK;
}
}  // namespace

namespace {
int generic_trunk_call(const nrnerf_model* m, const nrnerf_generic_trunk_args* a, bool backward, void* hip_stream) {
    if (!m || !a || a->struct_size != sizeof(nrnerf_generic_trunk_args)) return NRNERF_ERR_INVALID;
    if (!m->generic || !m->gen_train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->which < 0 || a->which > 1 || a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || !a->acts) return NRNERF_ERR_INVALID;
    const bool fine = a->which == 1 && !m->fine_is_coarse;
    const GenTrainNet& tn = m->gen_tn[fine ? 1 : 0];
    if (!backward && (!a->pts4 || !a->raw4 || (tn.views && !a->dirs) || (tn.lat > 0 && !a->latents))) return NRNERF_ERR_INVALID;
    // the epilogue writes channels 0..3 of a row of `raw`, and channel 4 when raw_ch > 4: the row must hold them and the network must have them
    if (!backward && a->raw && (a->raw_ch < 4 || a->raw_ch > (fine ? m->gen_fine : m->gen_coarse).output_ch)) return NRNERF_ERR_INVALID;
    if (backward && (!a->d_raw4 || !a->d_pre || !a->d_enc0 || (tn.skip && !a->d_enc1) || (tn.views && !a->d_encv))) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    const long long M = (long long)a->n_rays * a->n_samples;
    GenArgs g = backward ? (fine ? m->gen_fine_bwd.prog : m->gen_coarse_bwd.prog) : (fine ? m->gen_fine.prog : m->gen_coarse.prog);
    const PassDev& pd = backward ? (fine ? m->gen_fine_bwd : m->gen_coarse_bwd) : (fine ? m->gen_fine : m->gen_coarse);
    g.wstream = pd.stream; g.bias = pd.bias;
    g.n_rays = a->n_rays; g.S = a->n_samples;
    g.save_stride = M * tn.W; g.save_w = tn.W;
    if (!backward) {
        // the forward pass on the width-class 16x16x32 kernel (nrnerf_gx16.h, SAVE: activations written from the registers) when it has this
        // trunk: bf16, plain head, no latent input columns; 0.55 of the matrix pipe's peak instead of the run-time-parameterised kernel's 0.07
        const PassDev& gx = (fine ? m->gx_fine : m->gx_coarse);
        const GxMeta& gm = (fine ? m->gx_fine.gx : m->gx_coarse.gx);
        if (gx.stream && m->precision == NRNERF_PREC_BF16 && !tn.views && tn.lat == 0 && tn.W % 4 == 0 && M < (1ll << 32) &&
            (long long)a->n_rays * ((a->n_samples + 15) / 16) < (1ll << 31)) {
            GxArgs x{};
            x.pts4 = a->pts4; x.raw4 = a->raw4; x.raw_out = a->raw; x.raw_ch = a->raw ? a->raw_ch : 4;
            x.n_rays = a->n_rays; x.S = a->n_samples; x.wstream = gx.stream; x.bias = gx.bias;
            x.depth = gm.depth; x.skip = gm.skip; x.L = gm.L; x.n_bias_tiles = gm.n_bias_tiles; x.LV = gm.LV;
            x.save = a->acts; x.save_stride = M * tn.W; x.save_w = tn.W; x.relu_bits = a->relu_bits;
            return launch_gx16(m->precision, gm.wc, false, x, m->num_cus, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
        }
        g.mode = 1;
        g.rays = a->pts4; g.ray_stride = 0;                                              // (points are handed in: the ray record is never read)
        g.latents = tn.lat > 0 ? a->latents : nullptr; g.lat_stride = tn.lat;
        g.z = nullptr; g.lindisp = 0; g.pts4 = a->pts4; g.dirs_from_pts = 0; g.dirs = tn.views ? a->dirs : nullptr;
        g.raw4 = a->raw4; g.raw_out = a->raw; g.raw_ch = a->raw ? a->raw_ch : 4; g.bent4 = nullptr;
        g.save = a->acts; g.mask = nullptr;
    } else {
        // backward-data on the width-class kernel's dataflow (nrnerf_gx16_bwd.h) when the forward call left its relu bits
        const PassDev& gxb = (fine ? m->gx_fine_bwd : m->gx_coarse_bwd);
        const GxMeta& gmb = (fine ? m->gx_fine_bwd.gx : m->gx_coarse_bwd.gx);
        if (gxb.stream && a->relu_bits && !tn.views && tn.lat == 0 && M < (1ll << 32) && (long long)a->n_rays * ((a->n_samples + 15) / 16) < (1ll << 31)) {
            GxBwdArgs b{};
            b.d_raw4 = a->d_raw4; b.relu_bits = a->relu_bits; b.d_pre = a->d_pre; b.save_stride = M * tn.W; b.save_w = tn.W;
            b.d_enc0 = a->d_enc0; b.d_enc1 = a->d_enc1; b.enc_w = tn.in_w;
            b.n_rays = a->n_rays; b.S = a->n_samples; b.wstream = gxb.stream; b.bias = gxb.bias;
            b.depth = gmb.depth; b.skip = gmb.skip; b.L = gmb.L; b.n_bias_tiles = gmb.n_bias_tiles;
            return launch_gx16_bwd(gmb.wc, b, m->num_cus, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
        }
        g.mode = 2;
        g.rays = a->d_raw4; g.ray_stride = 0;
        g.draw = a->d_raw4; g.draw_ch = 4; g.draw_col = tn.draw_col;
        g.mask = a->acts; g.save = a->d_pre;
        g.gout[0] = a->d_enc0; g.gout[1] = a->d_enc1; g.gout[2] = a->d_encv; g.gout_w = tn.in_w; g.gout_w2 = tn.dv;
    }
    return launch_generic_train(m->precision, g, m->num_cus, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
}
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
    int dev = 0;
    if (device_of(backward ? (const void*)a->g_rgb_map : (const void*)a->loss, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    LossArgs l{a->n_rays, a->n_samples, a->rgb_map, a->rgb0, a->target, a->weights, a->offsets, a->rigidity, a->alpha, a->divergence,
               a->offsets_weight, a->rigidity_weight, a->divergence_weight, a->schedule, a->loss, a->g_loss, a->g_rgb_map, a->g_rgb0, a->g_offsets,
               a->g_rigidity, a->g_divergence, a->offsets_stride ? a->offsets_stride : 3, a->rigidity_stride ? a->rigidity_stride : 1,
               backward ? a->g_mean : nullptr};
    return launch_loss(l, backward, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
}
}  // namespace
int nrnerf_generic_trunk_forward(const nrnerf_model* m, const nrnerf_generic_trunk_args* a, void* hip_stream) try { return generic_trunk_call(m, a, false, hip_stream); } NRN_CATCH
int nrnerf_generic_trunk_backward(const nrnerf_model* m, const nrnerf_generic_trunk_args* a, void* hip_stream) try { return generic_trunk_call(m, a, true, hip_stream); } NRN_CATCH
int nrnerf_model_trains_generic(const nrnerf_model* m) { return m ? ((m->generic && m->gen_train_ok) ? 1 : 0) : NRNERF_ERR_INVALID; }
size_t nrnerf_generic_trunk_bits_bytes(const nrnerf_model* m, int32_t which, int32_t n_rays, int32_t n_samples) {
    if (!m || !m->generic || which < 0 || which > 1 || n_rays < 1 || n_samples < 1) return 0;
    const bool fine = which == 1 && !m->fine_is_coarse;
    const PassDev& gxb = fine ? m->gx_fine_bwd : m->gx_coarse_bwd;
    const GxMeta& gmb = fine ? m->gx_fine_bwd.gx : m->gx_coarse_bwd.gx;
    if (!gxb.stream) return 0;
    return (size_t)gmb.depth * (size_t)n_rays * (size_t)((n_samples + 15) / 16) * 64 * (size_t)gx16_bits_bytes_per_lane(gmb.wc);
}
int nrnerf_loss_forward(const nrnerf_loss_args* a, void* hip_stream) try { return loss_call(a, false, hip_stream); } NRN_CATCH
int nrnerf_code_gradients(const int64_t* index, const float* g, int32_t n_rays, int32_t latent_size, int32_t n_codes, float* out, void* hip_stream) try {
    if (!index || !g || !out || n_rays < 0 || latent_size < 1 || latent_size > 256 || n_codes < 0) return NRNERF_ERR_INVALID;
    if (n_codes == 0) return NRNERF_OK;
    int dev = 0;
    if (device_of(out, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    CodeGradArgs c{(const long long*)index, g, n_rays, latent_size, n_codes, out};
    return launch_code_gradients(c, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH
int nrnerf_loss_backward(const nrnerf_loss_args* a, void* hip_stream) try { return loss_call(a, true, hip_stream); } NRN_CATCH

int nrnerf_merge_rows(const uint8_t* rank_new, int32_t n_rays, int32_t n_samples, int32_t n_importance, float* coarse_a, float* coarse_b,
                      float* new_a, float* new_b, float* merged_a, float* merged_b, int32_t inverse, void* hip_stream) try {
    if (!rank_new || !coarse_a || !new_a || !merged_a || n_rays < 0 || n_samples < 1 || n_importance < 1 || n_samples + n_importance > 256) return NRNERF_ERR_INVALID;
    if ((coarse_b != nullptr) != (merged_b != nullptr) || (new_b != nullptr) != (merged_b != nullptr)) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    int dev = 0;
    if (device_of(merged_a, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    MergeRowsArgs a{n_rays, n_samples, n_importance, rank_new, coarse_a, coarse_b, new_a, new_b, merged_a, merged_b, inverse ? 1 : 0};
    return launch_merge_rows(a, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

namespace {
int reduce_partials_call(const float* partials, int64_t record_stride, int32_t n_partials, int32_t n_short, const int32_t* index,
                         int64_t n_out, float* out, const float* aux, int32_t n_aux, const int64_t* aux_pos, void* hip_stream) {
    if (!partials || !index || !out || n_out < 0 || n_partials < 1 || n_short < 0 || n_short > n_partials || record_stride < 1 ||
        record_stride >= NRNERF_REDUCE_SHORT) return NRNERF_ERR_INVALID;
    if (aux && (n_aux < 0 || !aux_pos)) return NRNERF_ERR_INVALID;
    if (n_out == 0) return NRNERF_OK;
    int dev = 0;
    if (device_of(out, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    ReducePartialsArgs a{partials, record_stride, n_partials, n_short, index, n_out, out, aux, aux ? n_aux : 0, {-1, -1, -1, -1}};
    if (aux)
        for (int c = 0; c < 4; ++c) {
            if (aux_pos[c] >= n_out) return NRNERF_ERR_INVALID;
            a.aux_pos[c] = aux_pos[c];
        }
    return launch_reduce_partials(a, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
}
}  // namespace
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
    int dev = 0;
    if (device_of(out, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    return launch_tile_row_sums(tiles, n_rows, out, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_tiles_to_rows(const void* tiles, int32_t n_rays, int32_t n_samples, int32_t width, void* rows, void* hip_stream) try {
    if (!tiles || !rows || n_rays < 0 || n_samples < 1 || n_samples > 256 || (width != 256 && width != 128)) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    int dev = 0;
    if (device_of(rows, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    return launch_tiles_to_rows(tiles, n_rays, n_samples, width, rows, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_direction_encoding(const float* bent4, int32_t n_rays, int32_t n_samples, int32_t n_freqs, void* enc, int32_t enc_is_bf16,
                              float* g_bent4, void* hip_stream) try {
    if (!bent4 || !enc || n_rays < 0 || n_samples < 2 || n_samples > NRNERF_MAX_SAMPLES || n_freqs < 0 || n_freqs > 10) return NRNERF_ERR_INVALID;
    if (n_rays == 0) return NRNERF_OK;
    int dev = 0;
    if (device_of(enc, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    DirEncodingArgs d{bent4, n_rays, n_samples, n_freqs, enc, enc_is_bf16 ? 1 : 0, g_bent4};
    return launch_dir_encoding(d, g_bent4 != nullptr, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

// ---- training entry points (nrnerf_train.h, composite_bwd_kernel) -------------------------------------------------
namespace {
int trunk_common(const nrnerf_model* m, const nrnerf_trunk_args* a, bool bwd, TrunkArgs& t) {
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
    t = TrunkArgs{};
    t.pts4 = a->pts4; t.n_rays = a->n_rays; t.S = a->n_samples;
    t.wstream = bwd ? bw.stream : fwd.stream; t.bias = fwd.bias;
    t.raw4 = a->raw4; t.raw_out = a->raw; t.raw_ch = a->raw_ch;
    t.acts = a->acts; t.d_raw4 = a->d_raw4; t.d_pre = a->d_pre; t.d_pts4 = a->d_pts4; t.ray_bias = a->ray_bias;
    t.mask = (unsigned short*)a->relu_mask;
    if (m->precision != NRNERF_PREC_F32 && !t.mask) return NRNERF_ERR_INVALID;
    if (m->views) {             // the colour branch behind the trunk (the *_views kernels)
        if (!a->dirs || !a->hv || (bwd && !a->d_pre_v) || (m->precision != NRNERF_PREC_F32 && !a->hv_mask)) return NRNERF_ERR_INVALID;
        t.dirs = a->dirs; t.hv = a->hv; t.hv_mask = (unsigned short*)a->hv_mask; t.d_pre_v = a->d_pre_v; t.d_dirs = a->d_dirs;
    }
    return NRNERF_OK;
}
}  // namespace

int nrnerf_trunk_forward(const nrnerf_model* m, const nrnerf_trunk_args* a, void* hip_stream) try {
    TrunkArgs t;
    const int rc = trunk_common(m, a, false, t);
    if (rc != NRNERF_OK) return rc;
    if (a->n_rays == 0) return NRNERF_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    const bool f32 = m->precision == NRNERF_PREC_F32;
    const hipStream_t s = (hipStream_t)hip_stream;
    const hipError_t e = (m->arch_id == 5) ? (f32 ? launch_trunk_fwd_train_f32_a5(t, m->num_cus, s) : launch_trunk_fwd_train_bf16_a5(t, m->num_cus, s))
                       : m->views ? (f32 ? launch_trunk_fwd_train_f32_views(t, m->num_cus, s) : launch_trunk_fwd_train_bf16_views(t, m->num_cus, s))
                                  : (f32 ? launch_trunk_fwd_train_f32(t, m->num_cus, s) : launch_trunk_fwd_train_bf16(t, m->num_cus, s));
    return e == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_trunk_backward(const nrnerf_model* m, const nrnerf_trunk_args* a, void* hip_stream) try {
    TrunkArgs t;
    const int rc = trunk_common(m, a, true, t);
    if (rc != NRNERF_OK) return rc;
    if (a->n_rays == 0) return NRNERF_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    const bool f32 = m->precision == NRNERF_PREC_F32;
    const hipStream_t s = (hipStream_t)hip_stream;
    const hipError_t e = (m->arch_id == 5) ? (f32 ? launch_trunk_bwd_f32_a5(t, m->num_cus, s) : launch_trunk_bwd_bf16_a5(t, m->num_cus, s))
                       : m->views ? (f32 ? launch_trunk_bwd_f32_views(t, m->num_cus, s) : launch_trunk_bwd_bf16_views(t, m->num_cus, s))
                                  : (f32 ? launch_trunk_bwd_f32(t, m->num_cus, s) : launch_trunk_bwd_bf16(t, m->num_cus, s));
    return e == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_trunk_wgrad(const nrnerf_model* m, const nrnerf_wgrad_args* a, void* hip_stream) try {
    if (!m || !a || a->struct_size != sizeof(nrnerf_wgrad_args)) return NRNERF_ERR_INVALID;
    if (!m->train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->n_partials < 1 || a->n_partials > 4096) return NRNERF_ERR_INVALID;
    if (!a->acts || !a->d_pre || !a->pts4 || !a->d_raw4 || !a->enc || !a->g_head || !a->partials) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    const bool f32 = m->precision == NRNERF_PREC_F32;
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
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    const hipStream_t s = (hipStream_t)hip_stream;
    const WgradOperandArgs ops{a->pts4, a->d_raw4, a->n_rays, a->n_samples, ArchDefault::L, a->enc, a->g_head, f32 ? nullptr : a->head_sums,
                               views ? a->dirs : nullptr, ArchDefault::LV, views ? a->encv : nullptr};
    if ((f32 ? launch_wgrad_operands_f32(ops, s) : launch_wgrad_operands(ops, s)) != hipSuccess) return NRNERF_ERR_HIP;
    const hipError_t e = (m->arch_id == 5) ? (f32 ? launch_trunk_wgrad_f32_a5(w, s) : launch_trunk_wgrad_bf16_a5(w, s))
                            : views ? (f32 ? launch_trunk_wgrad_f32_views(w, s) : launch_trunk_wgrad_bf16_views(w, s))
                                    : (f32 ? launch_trunk_wgrad_f32(w, s) : launch_trunk_wgrad_bf16(w, s));
    return e == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

namespace {
int bender_common(const nrnerf_model* m, const nrnerf_bender_args* a, bool bwd, BendTrainArgs& t) {
    if (!m || !a || a->struct_size != sizeof(nrnerf_bender_args)) return NRNERF_ERR_INVALID;
    if (!m->bend_train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES) return NRNERF_ERR_INVALID;
    if (!a->rays || a->ray_stride < 6 || !a->latents || a->latent_stride < m->latent_size || !a->z) return NRNERF_ERR_INVALID;
    if (!a->bent4 || !a->off4 || !a->acts_offsets || !a->acts_rigidity) return NRNERF_ERR_INVALID;
    if (bwd && (!a->g_bent4 || !a->dz_offsets || !a->dz_rigidity || !a->dz_out4 || !a->d_latents)) return NRNERF_ERR_INVALID;
    t = BendTrainArgs{};
    t.rays = a->rays; t.ray_stride = a->ray_stride; t.latents = a->latents; t.lat_stride = a->latent_stride; t.z = a->z;
    t.n_rays = a->n_rays; t.S = a->n_samples;
    const PassDev& p = bwd ? m->bend_train_bwd : m->bend_train_fwd;
    t.wstream = p.stream; t.bias = p.bias;
    t.knobs.has_cutoff = a->has_rigidity_cutoff; t.knobs.cutoff = a->rigidity_cutoff;
    t.knobs.has_scaling = a->has_test_time_scaling; t.knobs.scaling = a->test_time_scaling;
    t.bent4 = a->bent4; t.off4 = a->off4; t.acts_b = a->acts_offsets; t.acts_r = a->acts_rigidity;
    t.g_bent4 = a->g_bent4; t.g_bent4_b = a->g_bent4_b; t.g_unmasked = a->g_unmasked_offsets; t.g_mask = a->g_rigidity_mask;
    t.dz_b = a->dz_offsets; t.dz_r = a->dz_rigidity; t.dz_out4 = a->dz_out4; t.d_lat = a->d_latents;
    return NRNERF_OK;
}
}  // namespace

int nrnerf_bender_forward(const nrnerf_model* m, const nrnerf_bender_args* a, void* hip_stream) try {
    BendTrainArgs t;
    const int rc = bender_common(m, a, false, t);
    if (rc != NRNERF_OK) return rc;
    if (a->n_rays == 0) return NRNERF_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    const bool b16 = m->precision != NRNERF_PREC_F32;        // element type of the saved arrays (nrnerf_bender_args)
    const hipError_t e = (bender_arch_of(m) == 0) ? launch_bend_fwd_train_a0(t, m->num_cus, (hipStream_t)hip_stream, b16)
                                           : launch_bend_fwd_train_a1(t, m->num_cus, (hipStream_t)hip_stream, b16);
    return e == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_bender_backward(const nrnerf_model* m, const nrnerf_bender_args* a, void* hip_stream) try {
    BendTrainArgs t;
    const int rc = bender_common(m, a, true, t);
    if (rc != NRNERF_OK) return rc;
    if (a->n_rays == 0) return NRNERF_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    const bool b16 = m->precision != NRNERF_PREC_F32;
    const hipError_t e = (bender_arch_of(m) == 0) ? launch_bend_bwd_a0(t, m->num_cus, (hipStream_t)hip_stream, b16)
                                           : launch_bend_bwd_a1(t, m->num_cus, (hipStream_t)hip_stream, b16);
    return e == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_bender_wgrad(const nrnerf_model* m, const nrnerf_bender_wgrad_args* a, void* hip_stream) try {
    if (!m || !a || a->struct_size != sizeof(nrnerf_bender_wgrad_args)) return NRNERF_ERR_INVALID;
    if (!m->bend_train_ok) return NRNERF_ERR_UNSUPPORTED;
    if (a->n_rays < 0 || a->n_samples < 1 || a->n_samples > NRNERF_MAX_SAMPLES || a->n_partials < 4 || a->n_partials > 4096 || a->n_partials % 4) return NRNERF_ERR_INVALID;
    if (!a->rays || a->ray_stride < 6 || !a->latents || a->latent_stride < m->latent_size || !a->z) return NRNERF_ERR_INVALID;
    if (!a->acts_offsets || !a->acts_rigidity || !a->dz_offsets || !a->dz_rigidity || !a->dz_out4 || !a->partials) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    const int BD = (bender_arch_of(m) == 0) ? ArchDefault::BD : ArchDeepBend::BD;
    const int BW = ArchDefault::BW, RD = ArchDefault::RD, RW = ArchDefault::RW, X0 = 3 + ArchDefault::LAT;
    const size_t M = (size_t)a->n_rays * a->n_samples;
    if (m->precision != NRNERF_PREC_F32 && M * 64 * 4 >= 0xffffff00ull) return NRNERF_ERR_INVALID;      // 32-bit offsets in bend_wgrad16
    BendWgradArgs w{};
    int n = 0;
    const int b16 = m->precision != NRNERF_PREC_F32;        // the saved arrays' element type; dz_out4 is fp32 in every mode
    const size_t esz = b16 ? 2 : 4;
    auto at = [&](const void* base, size_t elems) { return (const void*)((const char*)base + elems * esz); };
    w.job[n++] = BendWgradJob{a->dz_offsets, BW, BW, nullptr, X0, X0, nullptr, nullptr, b16, 0};            // network[0]: input = [point, latent]
    for (int i = 1; i <= BD - 2; ++i)
        w.job[n++] = BendWgradJob{at(a->dz_offsets, (size_t)i * M * BW), BW, BW, at(a->acts_offsets, (size_t)(i - 1) * M * BW), BW, BW, nullptr, nullptr, b16, b16};
    w.job[n++] = BendWgradJob{a->dz_out4, 4, 3, at(a->acts_offsets, (size_t)(BD - 2) * M * BW), BW, BW, nullptr, nullptr, 0, b16};   // network[BD-1]: 3 x BW
    w.job[n++] = BendWgradJob{a->dz_rigidity, RW, RW, nullptr, X0, 3, nullptr, nullptr, b16, 0};             // rigidity_network[0]: input = the point
    for (int i = 1; i <= RD - 2; ++i)
        w.job[n++] = BendWgradJob{at(a->dz_rigidity, (size_t)i * M * RW), RW, RW, at(a->acts_rigidity, (size_t)(i - 1) * M * RW), RW, RW, nullptr, nullptr, b16, b16};
    w.job[n++] = BendWgradJob{a->dz_out4 + 3, 4, 1, at(a->acts_rigidity, (size_t)(RD - 2) * M * RW), RW, RW, nullptr, nullptr, 0, b16};   // the logit's layer: 1 x RW
    w.njobs = n; w.nparts = a->n_partials; w.m = (long long)M; w.out = a->partials;
    w.rays = a->rays; w.ray_stride = a->ray_stride; w.latents = a->latents; w.lat_stride = a->latent_stride; w.lat = m->latent_size;
    w.z = a->z; w.S = a->n_samples;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    return launch_bend_wgrad(w, (hipStream_t)hip_stream, m->precision != NRNERF_PREC_F32) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

namespace {
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
    t.knobs.has_cutoff = a->has_rigidity_cutoff; t.knobs.cutoff = a->rigidity_cutoff;
    t.knobs.has_scaling = a->has_test_time_scaling; t.knobs.scaling = a->test_time_scaling;
    t.div = a->divergence; t.off4 = a->off4; t.toff4 = a->toff4; t.tvec = a->tangent; t.g_tvec = a->g_tangent;
    t.r_g_bent4 = a->render_g_bent4; t.r_g_bent4_b = a->render_g_bent4_b; t.r_g_unmasked = a->render_g_unmasked_offsets; t.r_g_mask = a->render_g_rigidity_mask;
    t.bent4 = bwd ? nullptr : a->bent4;
    t.acts_b = a->acts_offsets; t.tacts_b = a->tacts_offsets; t.acts_r = a->acts_rigidity; t.tacts_r = a->tacts_rigidity;
    t.g_div = a->g_divergence; t.dz_b = a->dz_offsets; t.dtz_b = a->dtz_offsets; t.dz_r = a->dz_rigidity; t.dtz_r = a->dtz_rigidity;
    t.dz_out4 = a->dz_out4; t.dtz_out4 = a->dtz_out4; t.d_lat = a->d_latents;
    return NRNERF_OK;
}
}  // namespace

int nrnerf_bender_divergence_forward(const nrnerf_model* m, const nrnerf_divergence_args* a, void* hip_stream) try {
    BendDivArgs t;
    const int rc = divergence_common(m, a, false, t);
    if (rc != NRNERF_OK) return rc;
    if (a->n_points == 0) return NRNERF_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    const bool b16 = m->precision != NRNERF_PREC_F32;
    const hipError_t e = (bender_arch_of(m) == 0) ? launch_bend_div_fwd_a0(t, m->num_cus, (hipStream_t)hip_stream, b16)
                                                        : launch_bend_div_fwd_a1(t, m->num_cus, (hipStream_t)hip_stream, b16);
    return e == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_bender_divergence_backward(const nrnerf_model* m, const nrnerf_divergence_args* a, void* hip_stream) try {
    BendDivArgs t;
    const int rc = divergence_common(m, a, true, t);
    if (rc != NRNERF_OK) return rc;
    if (a->n_points == 0) return NRNERF_OK;
    const bool b16 = m->precision != NRNERF_PREC_F32;
    if (b16 && (size_t)a->n_points * 64 * 4 >= 0xffffff00ull) return NRNERF_ERR_INVALID;      // 32-bit offsets in bend_wgrad16: nothing is launched
    DeviceGuard guard(m->device);
    if (!guard.ok) return NRNERF_ERR_HIP;
    hipError_t e = (bender_arch_of(m) == 0) ? launch_bend_div_bwd_a0(t, m->num_cus, (hipStream_t)hip_stream, b16)
                                                  : launch_bend_div_bwd_a1(t, m->num_cus, (hipStream_t)hip_stream, b16);
    if (e != hipSuccess) return NRNERF_ERR_HIP;
    // weight / bias gradients: dW_i = dz_i^T h_{i-1} + dtz_i^T th_{i-1} (two products per job), db_i = column sums of dz_i
    const int BD = (bender_arch_of(m) == 0) ? ArchDefault::BD : ArchDeepBend::BD;
    const int BW = ArchDefault::BW, RD = ArchDefault::RD, RW = ArchDefault::RW, LAT = m->latent_size;
    const size_t M = (size_t)a->n_points;
    BendWgradArgs w{};
    int n = 0;
    const int s16 = b16 ? 1 : 0;                             // the saved arrays' element type; points / probes / latents / dz_out4: fp32
    const size_t esz = b16 ? 2 : 4;
    auto at = [&](const void* base, size_t elems) { return (const void*)((const char*)base + elems * esz); };
    w.job[n++] = BendWgradJob{a->dz_offsets, BW, BW, a->points, 3, 3, a->dtz_offsets, a->probe, s16, 0};                 // network[0][:, 0:3]: th_0 = e
    w.job[n++] = BendWgradJob{a->dz_offsets, BW, BW, a->latents, a->latent_stride, LAT, nullptr, nullptr, s16, 0};        // network[0][:, 3:]
    for (int i = 1; i <= BD - 2; ++i)
        w.job[n++] = BendWgradJob{at(a->dz_offsets, (size_t)i * M * BW), BW, BW, at(a->acts_offsets, (size_t)(i - 1) * M * BW), BW, BW,
                                  at(a->dtz_offsets, (size_t)i * M * BW), at(a->tacts_offsets, (size_t)(i - 1) * M * BW), s16, s16};
    w.job[n++] = BendWgradJob{a->dz_out4, 4, 3, at(a->acts_offsets, (size_t)(BD - 2) * M * BW), BW, BW,
                              a->dtz_out4, at(a->tacts_offsets, (size_t)(BD - 2) * M * BW), 0, s16};
    w.job[n++] = BendWgradJob{a->dz_rigidity, RW, RW, a->points, 3, 3, a->dtz_rigidity, a->probe, s16, 0};               // rigidity_network[0]
    for (int i = 1; i <= RD - 2; ++i)
        w.job[n++] = BendWgradJob{at(a->dz_rigidity, (size_t)i * M * RW), RW, RW, at(a->acts_rigidity, (size_t)(i - 1) * M * RW), RW, RW,
                                  at(a->dtz_rigidity, (size_t)i * M * RW), at(a->tacts_rigidity, (size_t)(i - 1) * M * RW), s16, s16};
    w.job[n++] = BendWgradJob{a->dz_out4 + 3, 4, 1, at(a->acts_rigidity, (size_t)(RD - 2) * M * RW), RW, RW,
                              a->dtz_out4 + 3, at(a->tacts_rigidity, (size_t)(RD - 2) * M * RW), 0, s16};
    w.njobs = n; w.nparts = a->n_partials; w.m = (long long)M; w.out = a->partials;
    w.S = 1;
    e = launch_bend_wgrad(w, (hipStream_t)hip_stream, m->precision != NRNERF_PREC_F32);
    return e == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

namespace {
int composite_device(const nrnerf_composite_args* a, int* dev) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, a->raw4) != hipSuccess) { (void)hipGetLastError(); return NRNERF_ERR_INVALID; }
    if (attr.type != hipMemoryTypeDevice) return NRNERF_ERR_INVALID;
    *dev = attr.device;
    return NRNERF_OK;
}
}  // namespace

int nrnerf_composite_forward(const nrnerf_composite_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_composite_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 2 || a->n_importance < 0) return NRNERF_ERR_INVALID;
    if (a->n_samples > NRNERF_MAX_SAMPLES || a->n_samples + a->n_importance > NRNERF_MAX_SAMPLES) return NRNERF_ERR_UNSUPPORTED;
    if (a->rank_new && a->n_samples + a->n_importance > 256) return NRNERF_ERR_UNSUPPORTED;       // 8-bit ranks (the split fine bender)
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || a->ray_stride < 8 || !a->raw4 || !a->rgb || !a->disp || !a->acc) return NRNERF_ERR_INVALID;
    if (a->n_importance > 0 && !a->z_merged) return NRNERF_ERR_INVALID;
    if ((a->z_new != nullptr) != (a->rank_new != nullptr)) return NRNERF_ERR_INVALID;
    int dev = 0;
    int rc = composite_device(a, &dev);
    if (rc != NRNERF_OK) return rc;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    CompositeArgs c{};
    c.rays = a->rays; c.ray_stride = a->ray_stride; c.raw4 = a->raw4; c.z = a->z; c.lindisp = a->lindisp;
    c.white_bkgd = a->white_bkgd; c.noise = a->noise; c.u = a->u; c.n_rays = a->n_rays; c.S = a->n_samples;
    c.n_importance = a->n_importance; c.rgb = a->rgb; c.disp = a->disp; c.acc = a->acc; c.z_std = a->z_std;
    c.z_out = a->z_merged; c.vis = a->weights; c.alpha = a->alpha;
    if (a->n_importance > 0) { c.z_new = a->z_new; c.rank_new = a->rank_new; }
    return launch_composite(c, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_composite_backward(const nrnerf_composite_args* a, void* hip_stream) try {
    if (!a || a->struct_size != sizeof(nrnerf_composite_args)) return NRNERF_ERR_INVALID;
    if (a->n_rays < 0 || a->n_samples < 2 || a->n_samples > NRNERF_MAX_SAMPLES) return NRNERF_ERR_INVALID;
    if (a->n_rays == 0) return NRNERF_OK;
    if (!a->rays || a->ray_stride < 8 || !a->raw4 || !a->g_rgb || !a->d_raw4) return NRNERF_ERR_INVALID;
    int dev = 0;
    int rc = composite_device(a, &dev);
    if (rc != NRNERF_OK) return rc;
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    CompositeBwdArgs c{};
    c.rays = a->rays; c.ray_stride = a->ray_stride; c.raw4 = a->raw4; c.z = a->z; c.lindisp = a->lindisp;
    c.white_bkgd = a->white_bkgd; c.noise = a->noise; c.n_rays = a->n_rays; c.S = a->n_samples;
    c.g_rgb = a->g_rgb; c.g_disp = a->g_disp; c.g_acc = a->g_acc; c.g_w = a->g_weights; c.d_raw4 = a->d_raw4;
    return launch_composite_bwd(c, (hipStream_t)hip_stream) == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP;
} NRN_CATCH

int nrnerf_profile_begin(nrnerf_model* m) try {
    if (!m) return NRNERF_ERR_INVALID;
    std::lock_guard<std::mutex> g(m->prof_mu);
    for (auto& e : m->prof_events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    m->prof_events.clear();
    m->prof_on = true;
    return NRNERF_OK;
} NRN_CATCH

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
