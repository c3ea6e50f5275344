// nrnerf_pack.h -- the host-side weight packer's interface (nrnerf_pack.cpp): what the rest of the library (nrnerf_api.cpp: upload /
// refresh / free, render plan, training entry points) sees of it.  No HIP call on either side of this header.
#pragma once
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "nrnerf.h"
#include "nrnerf_kernels.h"
#include "nrnerf_gx16_plan.h"

namespace nrn {

struct PackedPass {
    std::vector<uint8_t> stream;
    std::vector<uint32_t> unit_off;   // nunits + 1, in 16-byte words
    std::vector<float> bias;          // ntiles * 32
    int ntiles = 0, nunits = 0, frag_bytes = 0, slot_bytes = 0, mfma_per_block = 0;
    // where every stream element / bias entry comes from in the flat parameter vector (nrnerf_model_update_device):
    // index (-1 = constant zero) and target format (RepackFmt); filled when a FlatLayout is given to the packer
    std::vector<int32_t> src, bias_src;
    std::vector<uint8_t> fmt;
};

// Flat parameter vector of a model (documented in nrnerf.h at nrnerf_model_update_device): every nn.Linear as weight
// [out, in] row-major then bias [out] (if it has one), in the order bender.network[0..], bender.rigidity_network[0..],
// coarse (pts_linears[0..], then output_linear | alpha, feature, views, rgb), fine likewise.
struct FlatLayout {
    std::vector<std::pair<const float*, int64_t>> base;      // host weight / bias pointer of the description -> offset
    int64_t total = 0;
    void add(const nrnerf_linear& l) {
        if (!l.weight) return;
        base.push_back({l.weight, total}); total += (int64_t)l.out_features * l.in_features;
        if (l.bias) { base.push_back({l.bias, total}); total += l.out_features; }
    }
    int64_t of(const float* p) const {
        for (auto& b : base) if (b.first == p) return b.second;
        return -1;
    }
    // DERIVED entries, after every real parameter: per network with the view-dependent head (coarse, then fine) the views
    // layer with feature_linear folded in -- weight [W/2][W + direction encoding] = [W_v[:, :W] W_f | W_v[:, W:]], then bias
    // [W/2] = W_v[:, :W] b_f + b_v -- keyed by the views weight pointer of the description
    std::vector<std::pair<const float*, int64_t>> folded;
    void add_folded(const nrnerf_mlp_desc& m) {
        if (!m.use_viewdirs || !m.views_linear.weight) return;
        folded.push_back({m.views_linear.weight, total});
        total += (int64_t)m.views_linear.out_features * m.views_linear.in_features + m.views_linear.out_features;
    }
    int64_t folded_of(const float* views_weight) const {
        for (auto& b : folded) if (b.first == views_weight) return b.second;
        return -1;
    }
};
FlatLayout flat_layout(const nrnerf_model_desc& d);

// ---- the packed weight images of a model handle: pack_images() is the one place that says which exist, how each is packed and what
// metadata goes with it; create / update / destroy and the device-side re-pack iterate the slots
enum ImageSlot : int {
    IMG_COARSE, IMG_FINE, IMG_FINE_TRUNK, IMG_COARSE_TRUNK, IMG_BEND_ONLY, IMG_FINE_TRUNK_X16, IMG_COARSE_TRUNK_X16, IMG_BEND_X16,
    IMG_COARSE_BWD, IMG_FINE_BWD, IMG_COARSE_TRAIN, IMG_FINE_TRAIN, IMG_BEND_TRAIN_FWD, IMG_BEND_TRAIN_BWD,
    IMG_GEN_BEND, IMG_GEN_COARSE, IMG_GEN_FINE, IMG_GX_COARSE, IMG_GX_FINE, IMG_GEN_COARSE_BWD, IMG_GEN_FINE_BWD, IMG_GX_COARSE_BWD, IMG_GX_FINE_BWD,
    IMG_COUNT
};
// an image as the host packs it
struct Image {
    ImageSlot slot;
    PackedPass pk;
    double algo_flops = 0, mfma_flops = 0;      // per sample, as PassDev
    int output_ch = 4;
    GenArgs proto{};                             // layer programs: the program
    GxMeta gx{};                                 // width-class trunks: the kernel's run-time parameters
    explicit Image(ImageSlot s) : slot(s) {}
};
// what the training entry points of a generic handle know about a trunk
struct GenTrainNet { int W = 0, D = 0, dv = 0, draw_col = 0, in_w = 0, lat = 0, skip = 0, views = 0; };
// what a model description makes of a handle besides its images (pack_images); a refresh needs a description with the same traits
// (ints throughout, flags included: no padding, so two records are the same model exactly when their bytes are equal -- same_traits)
struct ModelTraits {
    int precision = 0, has_bend = 0, views = 0, arch_id = 0, needs_latents = 0, latent_size = 0, exact = 0;
    int fine_is_coarse = 0;       // no fine network: the coarse network's images serve both passes
    int split_ok = 0;             // split-bender images (fine_trunk, coarse_trunk, bend_only)
    int train_ok = 0;             // see training_eligible
    int bend_train_ok = 0;        // the bender's training images
    int generic = 0;              // architecture outside the compiled set: layer programs
    int gen_compiled_bender = -1; // generic, >= 0: the bender has one of the compiled shapes (0: 5 x 64, 1: 7 x 64; latent 32, rigidity 3 x 32) and the
                                  // stand-alone bender kernel (nrnerf_bend.h, image `bend_only`) takes the passes without detail outputs
    int gen_train_ok = 0;
    GenTrainNet gen_tn[2];        // [coarse, fine]
};
static_assert(std::has_unique_object_representations_v<ModelTraits>, "ModelTraits is compared as bytes: no padding, no floating point");
inline bool same_traits(const ModelTraits& a, const ModelTraits& b) { return std::memcmp(&a, &b, sizeof(ModelTraits)) == 0; }

// the trunk-only / bender-only kernels of the split-bender path: the trunk is the architecture's without bender (the 5- and
// the 7-layer bender share architecture 0's), the bender kernel is compiled per bender shape (narrow trunk: the 5-layer one)
int trunk_arch(int arch_id);
int bender_arch(int arch_id);

// The images of a model description, and what else the description makes of a handle (`t`).  Every eligibility decision and every
// metadata formula of a handle lives here; no HIP call.  `lay` (create): the packers record where every element comes from in the flat
// parameter vector (nrnerf_model_update_device); null for a refresh.  "No fine network" yields no IMG_FINE / IMG_GEN_FINE (the handle
// resolves them to the coarse images).
int pack_images(const nrnerf_model_desc& d, const FlatLayout* lay, ModelTraits& t, std::vector<Image>& out);
// the image nrnerf_pack_host (include/nrnerf.h) hands out for `which`; a program's "unit table" is its layer list
int pack_host_image(const nrnerf_model_desc* desc, int which, PackedPass& pk);

}  // namespace nrn
