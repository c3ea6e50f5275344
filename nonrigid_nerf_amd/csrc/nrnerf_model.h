// nrnerf_model.h -- what the two units of the C ABI share (nrnerf_api.cpp: model lifetime and rendering; nrnerf_train_api.cpp: the training
// entry points): the handle, and how an entry point reaches a device.  Host only, no kernel body.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <vector>

#include "nrnerf_pack.h"

// Nothing throws across the C ABI (include/nrnerf.h): every extern "C" body is a function-try-block that turns
// std::bad_alloc (the packer's std::vector growth) into NRNERF_ERR_NOMEM and anything else -- the packer's
// plan-consistency checks throw std::logic_error -- into NRNERF_ERR_INTERNAL.
#define NRN_CATCH catch (const std::bad_alloc&) { return NRNERF_ERR_NOMEM; } catch (...) { return NRNERF_ERR_INTERNAL; }

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
struct ImageDev : PassDev { nrn::GenArgs prog{}; nrn::GxMeta gx{}; };

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

struct nrnerf_model : nrn::ModelTraits {
    // `fine` / `gen_fine` resolve to the coarse network's image when the model has no fine network (one network for both passes)
    explicit nrnerf_model(const nrn::ModelTraits& t)
        : nrn::ModelTraits(t), fine(img[t.fine_is_coarse ? nrn::IMG_COARSE : nrn::IMG_FINE]), gen_fine(img[t.fine_is_coarse ? nrn::IMG_GEN_COARSE : nrn::IMG_GEN_FINE]) {}
    int device = 0, num_cus = 0;
    ImageDev img[nrn::IMG_COUNT];      // every packed weight image, by slot (pack_images says which exist); the names below are what the launch code uses
    ImageDev &coarse = img[nrn::IMG_COARSE], &fine;
    // split-bender path (bender; finite-difference view directions if any): the fine network WITHOUT the bender layers (its input points
    // come from the stand-alone bender kernel) and the bender + rigidity layers alone
    ImageDev &fine_trunk = img[nrn::IMG_FINE_TRUNK], &coarse_trunk = img[nrn::IMG_COARSE_TRUNK], &bend_only = img[nrn::IMG_BEND_ONLY];
    // the fine network's trunk once more, packed for the 16x16x32 kernel (nrnerf_net_x16.h): what the split-bender path's fine pass
    // runs when the call asks for no detail outputs
    ImageDev &fine_trunk_x16 = img[nrn::IMG_FINE_TRUNK_X16], &coarse_trunk_x16 = img[nrn::IMG_COARSE_TRUNK_X16];
    ImageDev &bend_x16 = img[nrn::IMG_BEND_X16];             // the bender + rigidity MLPs packed for the 16x16x32 stand-alone bender ("bf16" mode)
    // training (nrnerf_train.h): transposed trunk weights of both networks; train_ok: see training_eligible, fp32 or bf16
    ImageDev &coarse_bwd = img[nrn::IMG_COARSE_BWD], &fine_bwd = img[nrn::IMG_FINE_BWD];
    // view-dependent head / time-conditioned baseline: bender-less forward images for trunk_fwd_train (with both branches of the head /
    // without the latent columns)
    ImageDev &coarse_train = img[nrn::IMG_COARSE_TRAIN], &fine_train = img[nrn::IMG_FINE_TRAIN];
    // training of the ray bender (nrnerf_train_bend.h): its layers alone in fp32 (whatever the model's precision) and
    // their transposes; bend_train_ok: train_ok and a bender
    ImageDev &bend_train_fwd = img[nrn::IMG_BEND_TRAIN_FWD], &bend_train_bwd = img[nrn::IMG_BEND_TRAIN_BWD];
    // generic architecture (nrnerf_generic.h): layer programs (ImageDev::prog) instead of compiled plans
    ImageDev &gen_bend = img[nrn::IMG_GEN_BEND], &gen_coarse = img[nrn::IMG_GEN_COARSE], &gen_fine;
    // the trunks of a generic model packed for the width-class 16x16x32 kernel (nrnerf_gx16.h; ImageDev::gx): 16-bit modes
    ImageDev &gx_coarse = img[nrn::IMG_GX_COARSE], &gx_fine = img[nrn::IMG_GX_FINE];
    // training of a generic model with a plain head (fp32 / bf16): the backward-data programs (transposed weights); the forward is
    // gen_coarse / gen_fine run with GenArgs::save set
    ImageDev &gen_coarse_bwd = img[nrn::IMG_GEN_COARSE_BWD], &gen_fine_bwd = img[nrn::IMG_GEN_FINE_BWD];
    ImageDev &gx_coarse_bwd = img[nrn::IMG_GX_COARSE_BWD], &gx_fine_bwd = img[nrn::IMG_GX_FINE_BWD];          // backward-data programs of the width-class trunks (nrnerf_gx16_bwd.h), when gx16_trainable
    int64_t flat_floats = 0;      // length of the flat parameter vector nrnerf_model_update_device expects
    unsigned* adam_barrier = nullptr;   // two words of device memory: the grid barrier of nrnerf_adam_step (nrnerf_optim.hip)
    // profiling (guarded; the render path itself is otherwise read-only on the handle)
    mutable std::mutex prof_mu;
    mutable bool prof_on = false;
    mutable int resident_launches[NRNERF_NUM_KERNELS] = {};      // net_kernel_x16's resident-slice variant, per profile slot, since profile_begin (prof_mu)
    struct Ev { int kernel; hipEvent_t a, b; double flops, mfma; const char* name; };
    mutable std::vector<Ev> prof_events;
};

// the run-time-parameterised kernel's TRAINING instantiations (nrnerf_generic.hip; the rendering ones: launch_generic, nrnerf_kernels.h): the
// training entry points' kernel, and the render path's on exact Jacobian view directions
namespace nrn { hipError_t launch_generic_train(int precision, const GenArgs& a, int num_cus, hipStream_t stream); }

// which compiled bender shape (0: 5 x 64, 1: 7 x 64) the bender's training kernels run: the handle's architecture, or -- a generic handle --
// the compiled shape its bender happens to have (the reference's hard-coded one next to an odd trunk, rnh:406-407)
inline int bender_arch_of(const nrnerf_model* m) { return m->generic ? m->gen_compiled_bender : nrn::bender_arch(m->arch_id); }

// the device that owns `ptr` (device memory): NRNERF_OK and `dev`, or NRNERF_ERR_INVALID
inline int device_of(const void* ptr, int& dev) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) { (void)hipGetLastError(); return NRNERF_ERR_INVALID; }
    if (attr.type != hipMemoryTypeDevice) return NRNERF_ERR_INVALID;
    dev = attr.device;
    return NRNERF_OK;
}

inline int status_of(hipError_t e) { return e == hipSuccess ? NRNERF_OK : NRNERF_ERR_HIP; }
// THE EXCEPTION (nrnerf_encoding_*, nrnerf_tn_products): their launchers answer hipErrorInvalidValue for an operand they cannot take (alignment,
// row stride) without launching anything, and the caller hears NRNERF_ERR_INVALID rather than NRNERF_ERR_HIP
inline int status_of_checked_launch(hipError_t e) { return e == hipErrorInvalidValue ? NRNERF_ERR_INVALID : status_of(e); }

// How an entry point launches: `run` -- the launches, answering a status -- with the right device current, whatever the calling thread's is.
// On a device index, on the device that owns `ptr` (the model-less entry points), on the model's device.
template <class RUN> int on_device(int dev, RUN&& run) {
    DeviceGuard guard(dev);
    if (!guard.ok) return NRNERF_ERR_HIP;
    return run();
}
template <class RUN> int on_owner_of(const void* ptr, RUN&& run) {
    int dev = 0;
    if (device_of(ptr, dev) != NRNERF_OK) return NRNERF_ERR_INVALID;
    return on_device(dev, run);
}
template <class RUN> int on_model_device(const nrnerf_model* m, RUN&& run) { return on_device(m->device, run); }

// every packed image of the handle (weight stream + bias table) from `flat_params`: segments of repack launches, REPACK_MAX_SEGMENTS per launch
inline int repack_batches(const nrnerf_model* m, const float* flat_params, hipStream_t stream) {
    for (const ImageDev& p : m->img)
        if (p.stream && !p.src) return NRNERF_ERR_UNSUPPORTED;          // (before anything is launched)
    nrn::RepackBatchArgs b{};
    b.flat = flat_params;
    auto add = [&](const int32_t* src, const uint8_t* fmt, void* dst, long long n) -> bool {
        if (n <= 0) return true;
        if (b.n_segments == nrn::REPACK_MAX_SEGMENTS) {
            if (nrn::launch_repack_batch(b, stream) != hipSuccess) return false;
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
    return status_of(nrn::launch_repack_batch(b, stream));
}
