// nrnerf_pack.cpp -- weight packing into the MFMA fragment streams described by nrnerf_plan.h (and nrnerf_gx16_plan.h,
// nrnerf_bend_x16_plan.h): every packer, eligibility predicate and layer-program builder, and pack_images(), which says which images a
// model description has.  Host code only: no HIP call.
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include <vector>

#include "nrnerf_pack.h"
#include "nrnerf_x16_api.h"
#include "nrnerf_bend_x16_plan.h"
#include "nrnerf_plan.h"

namespace nrn {
namespace {

// ------------------------------------------------------------------------------------------
// host-side element conversion
// ------------------------------------------------------------------------------------------
inline uint16_t f32_to_bf16(float f) {       // round to nearest even, NaN preserved
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline uint16_t f32_to_f16(float f) {
    _Float16 h = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}

// views_linears[0] o feature_linear as one layer (see LK_VIEWS in nrnerf_plan.h): fp64 products rounded to fp32 once
struct FoldedViews {
    std::vector<float> w, b;
    nrnerf_linear lin{};
    explicit FoldedViews(const nrnerf_mlp_desc& m) {
        const nrnerf_linear& v = m.views_linear;
        const nrnerf_linear& f = m.feature_linear;
        const int O = v.out_features, K = v.in_features, W = f.out_features, Wi = f.in_features;
        if (!v.weight || !f.weight || K < W) throw std::logic_error("view-dependent head: views layer narrower than the feature vector");
        w.assign((size_t)O * (size_t)(K - W + Wi), 0.0f);
        b.assign((size_t)O, 0.0f);
        const int Kf = K - W + Wi;                 // (Wi == W for the reference's head: same row length as the views layer)
        for (int r = 0; r < O; ++r) {
            for (int c = 0; c < Wi; ++c) {
                double acc = 0.0;
                for (int k = 0; k < W; ++k) acc += (double)v.weight[(size_t)r * K + k] * (double)f.weight[(size_t)k * Wi + c];
                w[(size_t)r * Kf + c] = (float)acc;
            }
            for (int c = W; c < K; ++c) w[(size_t)r * Kf + Wi + (c - W)] = v.weight[(size_t)r * K + c];
            double acc = v.bias ? (double)v.bias[r] : 0.0;
            if (f.bias) for (int k = 0; k < W; ++k) acc += (double)v.weight[(size_t)r * K + k] * (double)f.bias[k];
            b[r] = (float)acc;
        }
        lin.weight = w.data(); lin.bias = b.data(); lin.out_features = O; lin.in_features = Kf;
    }
};
void add_mlp(FlatLayout& f, const nrnerf_mlp_desc& m) {
    for (int i = 0; i < m.depth; ++i) f.add(m.pts_linears[i]);
    if (m.use_viewdirs) { f.add(m.alpha_linear); f.add(m.feature_linear); f.add(m.views_linear); f.add(m.rgb_linear); }
    else f.add(m.output_linear);
}

const nrnerf_linear* layer_source(const nrnerf_model_desc& d, const nrnerf_mlp_desc& mlp, const LayerSpec& sp) {
    switch (sp.kind) {
        case LK_BEND_IN: case LK_BEND_HID: case LK_BEND_OUT: return &d.bender->network[sp.index];
        case LK_RIG_IN: case LK_RIG_HID: case LK_RIG_OUT: return &d.bender->rigidity_network[sp.index];
        case LK_TR_IN: case LK_TR_HID: case LK_TR_SKIP: return &mlp.pts_linears[sp.index];
        case LK_HEAD: return &mlp.output_linear;
        case LK_ALPHA: return &mlp.alpha_linear;
        case LK_FEAT: return &mlp.feature_linear;
        case LK_VIEWS: return &mlp.views_linear;
        case LK_RGB: return &mlp.rgb_linear;
    }
    return nullptr;
}

// ------------------------------------------------------------------------------------------
// The fragment writer: what every packer below shares.  A packer is its layer list plus two rules -- which W[row][col] a fragment slot
// holds (and in which format), and which bias row a table entry holds; these are what must match the index functions of the plan
// headers the kernels read with.  The writer owns the rest: the PackedPass preamble, the zero-if-negative read, the conversion, the
// record of where every element comes from in the flat parameter vector (when a FlatLayout is given) and the plan / packer drift checks.
// ------------------------------------------------------------------------------------------
// PackedPass::fmt.  FMT_LO: the lo fragment of a split layer, f16((w - f16(w)) * LO_SCALE)
enum Fmt : uint8_t { FMT_F32 = 0, FMT_BF16 = 1, FMT_F16 = 2, FMT_LO = 3 };
// (one scale for every shape: the writer converts without knowing the packer's shape)
constexpr float LO_SCALE = Shape16::LO_SCALE;
static_assert(ShapeF32::LO_SCALE == LO_SCALE && Shape16Fast::LO_SCALE == LO_SCALE, "FMT_LO: the shapes' lo-part scales differ");

// a layer's parameters: on the host, and in the flat parameter vector (-1: not recorded)
struct Source { const nrnerf_linear* lin; int64_t wbase, bbase; };
Source source_of(const FlatLayout* lay, const nrnerf_linear* lin) {
    return {lin, lay ? lay->of(lin->weight) : -1, (lay && lin->bias) ? lay->of(lin->bias) : -1};
}
// the views layer with feature_linear folded in: the derived entries of the flat vector (FlatLayout::add_folded), weight then bias
Source folded_source(const FlatLayout* lay, const nrnerf_mlp_desc& mlp, const FoldedViews& folded) {
    const int64_t fb = lay ? lay->folded_of(mlp.views_linear.weight) : -1;
    return {&folded.lin, fb, fb < 0 ? -1 : fb + (int64_t)folded.lin.out_features * folded.lin.in_features};
}

struct FragWriter {
    PackedPass& out;
    const FlatLayout* lay;
    const int frag_bytes, elem_bytes, bias_rows;      // bias_rows: table entries per tile (32, or 16 in the 16x16x32 images)
    size_t nfrags = 0, written = 0;                   // fragments there is room for / filled so far
    FragWriter(PackedPass& o, const FlatLayout* l, int fb, int eb, int rows) : out(o), lay(l), frag_bytes(fb), elem_bytes(eb), bias_rows(rows) {}

    // the preamble: a zeroed stream of `units` slots, the unit table (ramp: every slot's offset in 16-byte words; else a single 0), a
    // zeroed bias table of `tiles` tiles; `fmt`: what the device-side refresh writes where no packer rule does (padding)
    void begin(int units, int slot_bytes, size_t stream_bytes, int tiles, Fmt fmt, bool ramp) {
        out.ntiles = tiles; out.nunits = units; out.frag_bytes = frag_bytes; out.slot_bytes = slot_bytes;
        out.stream.clear(); out.bias.clear(); out.src.clear(); out.fmt.clear(); out.bias_src.clear();
        grow(stream_bytes, tiles, fmt);
        out.unit_off.assign(ramp ? units + 1 : 1, 0);
        for (int u = 0; ramp && u <= units; ++u) out.unit_off[u] = (uint32_t)((size_t)u * slot_bytes / 16);
        written = 0;
    }
    // ... of a compiled plan: its padded units, its fragment count as the drift bound
    template <class SH> void begin_plan(const Tables& T, Fmt fmt) {
        begin(T.nunits_padded, SH::UNIT_BYTES, (size_t)T.nunits_padded * SH::UNIT_BYTES, T.ntiles, fmt, true);
        out.mfma_per_block = T.mfma_per_block;
        nfrags = (size_t)T.nfrags;
    }
    // room for more fragments and bias tiles behind what is there (a layer program grows layer by layer)
    void grow(size_t stream_bytes, int tiles, Fmt fmt) {
        out.stream.resize(out.stream.size() + stream_bytes, 0);
        out.bias.resize(out.bias.size() + (size_t)tiles * bias_rows, 0.0f);
        if (lay) {
            out.src.resize(out.stream.size() / elem_bytes, -1);
            out.fmt.resize(out.stream.size() / elem_bytes, fmt);
            out.bias_src.resize(out.bias.size(), -1);
        }
        nfrags = out.stream.size() / frag_bytes;
    }
    // One fragment being filled.  (A value the packer's loops keep in registers: the stores into the stream are byte stores, after which
    // anything reached through the writer would have to be read again.)
    struct Frag {
        uint8_t* data; int32_t* src; uint8_t* fmt;       // the fragment's first element in PackedPass::stream / src / fmt (the maps: null when not recorded)
        // slot `slot` = W[row][col] of the layer as `f`; a negative row or column: a constant zero
        void put(int slot, const Source& s, int row, int col, Fmt f) const {
            if (row < 0 || col < 0) return put(slot, 0.0f, -1, f);
            const int64_t at = (int64_t)row * s.lin->in_features + col;
            put(slot, s.lin->weight[at], s.wbase < 0 ? -1 : s.wbase + at, f);
        }
        // ... = w, which sits at `from` in the flat parameter vector (-1: nowhere)
        void put(int slot, float w, int64_t from, Fmt f) const {
            if (src) { src[slot] = (int32_t)from; fmt[slot] = f; }
            if (f == FMT_F32) { std::memcpy(data + slot * 4, &w, 4); return; }
            if (f == FMT_LO) w = (w - (float)(_Float16)w) * LO_SCALE;
            const uint16_t q = f == FMT_BF16 ? f32_to_bf16(w) : f32_to_f16(w);
            std::memcpy(data + slot * 2, &q, 2);
        }
    };
    // ... with the drift checks: every fragment a packer fills lies in the plan, and it fills as many as the plan has
    Frag frag(size_t fi) {
        if (fi >= nfrags) throw std::logic_error("plan / packer drift");
        ++written;
        const size_t el = fi * (size_t)(frag_bytes / elem_bytes);
        return {out.stream.data() + fi * frag_bytes, lay ? out.src.data() + el : nullptr, lay ? out.fmt.data() + el : nullptr};
    }
    void done(size_t expected) const { if (written != expected) throw std::logic_error("plan / packer drift"); }

    // the bias rows of a tile: table entry j = bias[row_of(j)] of the layer (a negative row, or a layer without bias: zero)
    template <class RowOf> void bias(size_t tile, const Source& s, RowOf row_of) {
        for (int j = 0; j < bias_rows; ++j) {
            const int row = row_of(j);
            if (row < 0 || !s.lin->bias) continue;
            out.bias[tile * bias_rows + j] = s.lin->bias[row];
            if (lay && s.bbase >= 0) out.bias_src[tile * bias_rows + j] = (int32_t)(s.bbase + row);
        }
    }
    // width-class streams: a copy of the first `tail` units behind unit `units` (the ring runs on into the next iteration's first units)
    void append_ring_tail(int units, int tail) {
        const size_t n = (size_t)tail * out.slot_bytes, o = (size_t)units * out.slot_bytes;
        std::memcpy(out.stream.data() + o, out.stream.data(), n);
        if (lay) {
            std::copy(out.src.begin(), out.src.begin() + n / elem_bytes, out.src.begin() + o / elem_bytes);
            std::copy(out.fmt.begin(), out.fmt.begin() + n / elem_bytes, out.fmt.begin() + o / elem_bytes);
        }
    }
};
// table entry j of a 32-row tile holds output row tile_row(j & 15, j >> 4) of the tile (the accumulator registers of lane half j >> 4)
inline int bias_row32(int j) { return tile_row(j & 15, j >> 4); }
// the views layer's last tile in the 16x16x32 images holds alpha_linear: its row 0, over the hidden k-steps only
inline int alpha_tile_row(int r) { return r == 0 ? 0 : -1; }

// tcb_shift (training of the time-conditioned baseline with architecture A = the plain trunk): the module's first layer
// reads [encoding, latent] and its skip layer [encoding, latent, h] (rnh:207-209, 273-282); the latent columns act as a
// per-ray bias (the latent is constant along a ray) that the caller supplies (nrnerf_trunk_args.ray_bias), so the images
// hold the encoding and the hidden columns only: hidden column c of the skip layer sits tcb_shift columns further right.
template <class SH, class A, bool HAS_BEND, bool VIEWS, bool TRUNK = true>
void pack_pass(const nrnerf_model_desc& d, const nrnerf_mlp_desc& mlp, int precision, PackedPass& out, const FlatLayout* lay = nullptr,
               int tcb_shift = 0) {
    constexpr int KH = SH::KH;
    const Tables& T = Plan<SH, A, HAS_BEND, VIEWS, TRUNK>::TB;
    FragWriter wr(out, lay, SH::FRAG_BYTES, SH::ELEM_BYTES, 32);
    wr.begin_plan<SH>(T, KH == 1 ? FMT_F32 : FMT_BF16);
    std::unique_ptr<FoldedViews> folded;           // the views layer's weights with feature_linear folded in (VIEWS plans)
    for (int l = 0; l < T.nlayers; ++l) {
        const LayerSpec& sp = T.layers[l];
        Source src = source_of(lay, layer_source(d, mlp, sp));
        if (sp.kind == LK_VIEWS) {
            folded.reset(new FoldedViews(mlp));
            src = folded_source(lay, mlp, *folded);
        }
        const int out_f = src.lin->out_features;
        const int in_f = src.lin->in_features - ((sp.kind == LK_TR_IN || sp.kind == LK_TR_SKIP) ? tcb_shift : 0);
        for (int t = 0; t < sp.nt; ++t) {
            const TileInfo& ti = T.tiles[sp.tile0 + t];
            for (int s = 0; s < sp.ns; ++s) {
                // split layers: fragment pair (hi, lo) with lo = f16((w - f16(w)) * 2^11); others: one fragment
                for (int part = 0; part <= sp.split; ++part) {
                    const FragWriter::Frag fr = wr.frag((size_t)ti.gbase + (size_t)s * ti.gstride + part);
                    const bool as_f16 = (precision == NRNERF_PREC_F16) || frag_is_f16<SH, A>(sp.kind, s);
                    const Fmt fmt = (KH == 1) ? FMT_F32 : (part == 1 ? FMT_LO : (as_f16 ? FMT_F16 : FMT_BF16));
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i = lane & 31, h = lane >> 5;
                        const int row = out_row<A>(sp.kind, t, i, out_f);
                        for (int e = 0; e < KH; ++e) {
                            int col = in_col<SH, A>(sp.kind, s, h, e, in_f);
                            if (tcb_shift && sp.kind == LK_TR_SKIP && col >= 3 + 6 * A::L) col += tcb_shift;
                            fr.put(lane * KH + e, src, row, col, fmt);
                        }
                    }
                }
            }
            wr.bias(sp.tile0 + t, src, [&](int j) { return out_row<A>(sp.kind, t, bias_row32(j), out_f); });
        }
    }
    wr.done(T.nfrags);
}

// The trunk-only image of the 16x16x32 kernel (nrnerf_net_x16.h, PlanX16): fragment (tile t, k-step s) holds, for lane (r = lane & 15,
// g = lane >> 4) and element e < 8,  W[x16_out_row(t, r)][x16_in_col(s, g, e)]; encoding k-steps f16, hidden ones the model's type;
// bias table [tile][16 rows].
// VIEWS: the view-dependent head as PlanX16 lays it out -- [views_linears[0] o feature_linear (FoldedViews) | alpha_linear in the last tile],
// then rgb_linear.
template <class SH, class A, bool VIEWS = false>
void pack_pass_x16(const nrnerf_mlp_desc& mlp, int precision, PackedPass& out, const FlatLayout* lay = nullptr) {
    using PL = PlanX16<SH, A, VIEWS>;
    const Tables& T = PL::TB;
    FragWriter wr(out, lay, SH::FRAG_BYTES, 2, 16);
    wr.begin_plan<SH>(T, FMT_BF16);
    std::unique_ptr<FoldedViews> folded;
    for (int l = 0; l < T.nlayers; ++l) {
        const LayerSpec& sp = T.layers[l];
        Source src0 = source_of(lay, (sp.kind == LK_HEAD) ? &mlp.output_linear : (sp.kind == LK_RGB ? &mlp.rgb_linear : &mlp.pts_linears[sp.index]));
        if (sp.kind == LK_VIEWS) {
            folded.reset(new FoldedViews(mlp));
            src0 = folded_source(lay, mlp, *folded);
        }
        for (int t = 0; t < sp.nt; ++t) {
            const bool alpha_tile = sp.kind == LK_VIEWS && t == sp.nt - 1;
            const Source src = alpha_tile ? source_of(lay, &mlp.alpha_linear) : src0;
            const int out_f = src.lin->out_features, in_f = src.lin->in_features;
            auto row_of = [&](int r) { return alpha_tile ? alpha_tile_row(r) : x16_out_row<A>(sp.kind, t, r, out_f); };
            const TileInfo& ti = T.tiles[sp.tile0 + t];
            for (int s = 0; s < sp.ns; ++s) {
                const FragWriter::Frag fr = wr.frag((size_t)ti.gbase + (size_t)s * ti.gstride);
                const bool enc_step = ((sp.kind == LK_TR_IN || sp.kind == LK_TR_SKIP) && s < PL::NS_E) || (sp.kind == LK_VIEWS && s == 0);
                const Fmt fmt = (precision == NRNERF_PREC_F16 || enc_step) ? FMT_F16 : FMT_BF16;
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = lane & 15, g = lane >> 4;
                    const int row = row_of(r);
                    for (int e = 0; e < 8; ++e) {
                        int col;
                        if (alpha_tile) { col = (s == 0) ? -1 : x16_hidden_feature(s - 1, g, e); if (col >= in_f) col = -1; }
                        else col = x16_in_col<A>(sp.kind, s, g, e, in_f);
                        fr.put(lane * 8 + e, src, row, col, fmt);
                    }
                }
            }
            wr.bias(sp.tile0 + t, src, row_of);
        }
    }
    wr.done(T.nfrags);
}
// does the 16x16x32 trunk kernel have this network?  (compiled architecture 0's trunk, output_linear head, 16-bit precision)
bool x16_eligible(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m, bool any_16bit = false) {
    using A = ArchDefault;
    const bool width_ok = m.width == ArchDefault::W || m.width == ArchNarrow::W;        // the two compiled trunk widths
    // (both 16-bit modes; nrnerf_model_desc::flags & NRNERF_MODEL_NO_X16_F16 keeps "f16" mode on the 32x32x16 kernels only.  At render
    //  time NRNERF_RENDER_NO_X16 selects the 32x32x16 trunk-only kernel per call: the split path is then bit-identical to the
    //  fused-bender fine pass in "f16" mode, which tests/test_gpu_parity.py asserts)
    const bool f16_too = !(d.flags & NRNERF_MODEL_NO_X16_F16);
    if (d.precision != NRNERF_PREC_BF16 && !(d.precision == NRNERF_PREC_F16 && (f16_too || any_16bit))) return false;
    if (m.time_conditioned || d.multires != A::L || m.depth != A::D || !width_ok || m.skip != A::SKIP) return false;
    if (m.use_viewdirs) {            // view-dependent head: width 256, 4 direction frequencies, finite-difference (not exact Jacobian) directions
        if (m.width != A::W || d.multires_views != A::LV || (d.exact_viewdirs && d.bender)) return false;
        if (m.views_linear.out_features != A::W / 2 || m.feature_linear.out_features != A::W) return false;
        return true;
    }
    if (m.output_ch != 4 && m.output_ch != 5) return false;
    return true;
}
void pack_x16(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m, PackedPass& out, const FlatLayout* lay = nullptr) {
    if (m.use_viewdirs) {
        if (d.precision == NRNERF_PREC_F16) pack_pass_x16<Shape16, ArchDefault, true>(m, d.precision, out, lay);
        else pack_pass_x16<Shape16Fast, ArchDefault, true>(m, d.precision, out, lay);
        return;
    }
    if (m.width == ArchNarrow::W) {
        if (d.precision == NRNERF_PREC_F16) pack_pass_x16<Shape16, ArchNarrow>(m, d.precision, out, lay);
        else pack_pass_x16<Shape16Fast, ArchNarrow>(m, d.precision, out, lay);
        return;
    }
    if (d.precision == NRNERF_PREC_F16) pack_pass_x16<Shape16, ArchDefault>(m, d.precision, out, lay);
    else pack_pass_x16<Shape16Fast, ArchDefault>(m, d.precision, out, lay);
}

// The bender + rigidity MLPs for the 16x16x32 stand-alone bender (nrnerf_bend_x16.h, PlanX16Bend): f16 fragments of 16 rows x 32 k,
// element (lane (r, g), e) = W[x16b_out_row(t, r)][x16b_in_col(s, g, e)]; bias table [tile][16 rows].
template <class A>
void pack_pass_x16_bend(const nrnerf_bender_desc& bd, PackedPass& out, const FlatLayout* lay = nullptr) {
    using SH = Shape16Fast;
    const Tables& T = PlanX16Bend<A>::TB;
    FragWriter wr(out, lay, SH::FRAG_BYTES, 2, 16);
    // (the kernel reads the fragments in place: no padding to whole units, no unit ramp)
    wr.begin(cdiv(T.nfrags, SH::UNIT_FRAGS), SH::UNIT_BYTES, (size_t)T.nfrags * SH::FRAG_BYTES, T.ntiles, FMT_F16, false);
    out.mfma_per_block = T.mfma_per_block;
    for (int l = 0; l < T.nlayers; ++l) {
        const LayerSpec& sp = T.layers[l];
        const Source src = source_of(lay, (sp.kind <= LK_BEND_OUT) ? &bd.network[sp.index] : &bd.rigidity_network[sp.index]);
        const int out_f = src.lin->out_features, in_f = src.lin->in_features;
        for (int t = 0; t < sp.nt; ++t) {
            const TileInfo& ti = T.tiles[sp.tile0 + t];
            for (int s = 0; s < sp.ns; ++s) {
                const FragWriter::Frag fr = wr.frag((size_t)ti.gbase + (size_t)s * ti.gstride);
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = lane & 15, g = lane >> 4;
                    const int row = x16b_out_row(sp.kind, t, r, out_f);
                    for (int e = 0; e < 8; ++e) fr.put(lane * 8 + e, src, row, x16b_in_col(sp.kind, s, g, e, in_f), FMT_F16);
                }
            }
            wr.bias(sp.tile0 + t, src, [&](int r) { return x16b_out_row(sp.kind, t, r, out_f); });
        }
    }
    wr.done(T.nfrags);
}
// does the 16x16x32 bender kernel have this bender?  (one of the two compiled shapes; both 16-bit modes: the single-product f16 bender.
// "f16" mode's fp32-equivalent three-product bender -- 3 x the MFMAs, 11.7 % of a 1080p frame in round 5 -- stays what the FUSED-bender kernels
// and the 32x32x16 stand-alone bender compute; NRNERF_MODEL_NO_X16_F16 keeps an "f16" handle on those alone.  That the single-product bender
// meets "f16" mode's stated bar (>= 40 dB vs the fp32 oracle, <= 0.1 dB vs ground truth) on all four fitted checkpoints:
// tests/test_fitted_checkpoint.py, profiles/r06_fitted_accuracy.txt.)
bool bend_x16_eligible(const nrnerf_model_desc& d) {
    if (!d.bender) return false;
    if (d.precision != NRNERF_PREC_BF16 && !(d.precision == NRNERF_PREC_F16 && !(d.flags & NRNERF_MODEL_NO_X16_F16))) return false;
    const nrnerf_bender_desc& b = *d.bender;
    using A = ArchDefault;
    return b.latent_size == A::LAT && b.hidden == A::BW && (b.depth == ArchDefault::BD || b.depth == ArchDeepBend::BD) &&
           b.rigidity_hidden == A::RW && b.rigidity_depth == A::RD;
}
void pack_bend_x16(const nrnerf_model_desc& d, PackedPass& out, const FlatLayout* lay = nullptr) {
    if (d.bender->depth == ArchDeepBend::BD) pack_pass_x16_bend<ArchDeepBend>(*d.bender, out, lay);
    else pack_pass_x16_bend<ArchDefault>(*d.bender, out, lay);
}

// Transposed weights for the backward-data kernel (nrnerf_train.h): PlanB's layer list, fragment element
// (tile t, row i, slab s, half h, element e) = W[y][x] with (y, x) from bwd_y / bwd_x.  No biases.
// VIEWS (view-dependent head, rnh:284-304): rgb_linear^T, then the layer that joins both branches of the head -- its k index
// runs over [d raw (only channel 3, sigma, is used: alpha_linear), d z_v (W/2)], its rows over [direction-encoding slots (one
// tile, enc_col order), h_{D-1} (W)]; the weights of the d z_v part are the FOLDED views layer's (FoldedViews: hidden columns
// first, then the direction encoding's), transposed.
template <class SH, class A, bool VIEWS = false>
void pack_pass_bwd(const nrnerf_mlp_desc& mlp, int precision, PackedPass& out, const FlatLayout* lay = nullptr, int tcb_shift = 0) {
    using PL = PlanB<SH, A, VIEWS>;
    constexpr int KH = SH::KH, SP = SH::SP;
    const Tables& T = PL::TB;
    const Fmt fmt = (KH == 1) ? FMT_F32 : (precision == NRNERF_PREC_F16 ? FMT_F16 : FMT_BF16);
    FragWriter wr(out, lay, SH::FRAG_BYTES, SH::ELEM_BYTES, 32);
    wr.begin_plan<SH>(T, fmt);
    std::unique_ptr<FoldedViews> folded;
    if (VIEWS) folded.reset(new FoldedViews(mlp));
    const int64_t fbase = VIEWS ? folded_source(lay, mlp, *folded).wbase : -1;
    const int64_t abase = VIEWS ? source_of(lay, &mlp.alpha_linear).wbase : -1;
    // LK_B_VHEAD: value and flat-vector position of element (tile t, row i, slab s, half h, element e)
    auto vhead = [&](int t, int i, int s, int h, int e, int64_t* src) -> float {
        constexpr int NT_EV = PL::NT_EV, NS_DR = PL::NS_DR;
        const int Kf = folded->lin.in_features, Wi = mlp.feature_linear.in_features;
        *src = -1;
        int col;                                    // column of the folded layer = output row of its transpose
        if (t < NT_EV) {
            const int hh = (i >> 2) & 1, r = (i & 3) + 4 * (i >> 3), q = t * 16 + r;      // inverse of tile_row
            const int c = q < enc_slots(A::LV) ? enc_col(A::LV, hh, q) : -1;
            if (c < 0) return 0.0f;
            col = Wi + c;
        } else {
            col = 32 * (t - NT_EV) + i;
            if (col >= Wi) return 0.0f;
        }
        if (s < NS_DR) {                            // d raw: only sigma (channel 3) enters here, through alpha_linear
            const int ch = (2 * s + h) * KH + e;
            if (ch != 3 || t < NT_EV) return 0.0f;
            if (abase >= 0) *src = abase + col;
            return mlp.alpha_linear.weight[col];
        }
        const int s2 = s - NS_DR, tp = s2 / SP, u = s2 % SP, r = u * KH + e;
        const int y = 32 * tp + tile_row(r, h);
        if (y >= folded->lin.out_features) return 0.0f;
        if (fbase >= 0) *src = fbase + (int64_t)y * Kf + col;
        return folded->w[(size_t)y * Kf + col];
    };
    for (int l = 0; l < T.nlayers; ++l) {
        const LayerSpec& sp = T.layers[l];
        const Source src = source_of(lay, (sp.kind == LK_B_HEAD) ? &mlp.output_linear
                                        : (sp.kind == LK_B_RGB) ? &mlp.rgb_linear : (sp.kind == LK_B_VHEAD) ? &mlp.alpha_linear : &mlp.pts_linears[sp.index]);
        const int out_f = src.lin->out_features;
        const int in_f = src.lin->in_features - ((sp.kind == LK_B_IN || sp.kind == LK_B_SKIP) ? tcb_shift : 0);
        for (int t = 0; t < sp.nt; ++t) {
            const TileInfo& ti = T.tiles[sp.tile0 + t];
            for (int s = 0; s < sp.ns; ++s) {
                const FragWriter::Frag fr = wr.frag((size_t)ti.gbase + (size_t)s * ti.gstride);
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = lane & 31, h = lane >> 5;
                    int x = bwd_x<SH, A>(sp.kind, t, i, in_f);
                    if (tcb_shift && sp.kind == LK_B_SKIP && x >= 3 + 6 * A::L) x += tcb_shift;      // see pack_pass
                    for (int e = 0; e < KH; ++e) {
                        if (sp.kind == LK_B_VHEAD) {
                            int64_t at;
                            const float w = vhead(t, i, s, h, e, &at);
                            fr.put(lane * KH + e, w, at, fmt);
                        } else {
                            fr.put(lane * KH + e, src, bwd_y<SH, A>(sp.kind, s, h, e, out_f), x, fmt);      // W[y][x]: the transpose
                        }
                    }
                }
            }
        }
    }
    wr.done(T.nfrags);
}

// Transposed weights of the bender / rigidity MLPs for their backward-data kernel (nrnerf_train_bend.h): PlanBB's layer
// list, always fp32.  Same element rule as pack_pass_bwd.
template <class A>
void pack_pass_bwd_bender(const nrnerf_bender_desc& b, PackedPass& out, const FlatLayout* lay = nullptr) {
    using SH = ShapeF32;
    const Tables& T = PlanBB<SH, A>::TB;
    FragWriter wr(out, lay, SH::FRAG_BYTES, SH::ELEM_BYTES, 32);
    wr.begin_plan<SH>(T, FMT_F32);
    for (int l = 0; l < T.nlayers; ++l) {
        const LayerSpec& sp = T.layers[l];
        const bool rig = sp.kind == LK_BR_OUT || sp.kind == LK_BR_HID;
        const Source src = source_of(lay, rig ? &b.rigidity_network[sp.index] : &b.network[sp.index]);
        for (int t = 0; t < sp.nt; ++t) {
            const TileInfo& ti = T.tiles[sp.tile0 + t];
            for (int s = 0; s < sp.ns; ++s) {
                const FragWriter::Frag fr = wr.frag((size_t)ti.gbase + (size_t)s * ti.gstride);
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = lane & 31, h = lane >> 5;
                    fr.put(lane, src, bwd_y<SH, A>(sp.kind, s, h, 0, src.lin->out_features), bwd_x<SH, A>(sp.kind, t, i, src.lin->in_features), FMT_F32);
                }
            }
        }
    }
    wr.done(T.nfrags);
}

bool linear_is(const nrnerf_linear& l, int out_f, int in_f, bool need_bias) {
    return l.weight && l.out_features == out_f && l.in_features == in_f && (!need_bias || l.bias);
}

// does the bender have compiled architecture A's bender shape?
template <class A>
bool bender_matches(const nrnerf_bender_desc& b) {
    if (b.latent_size != A::LAT || b.depth != A::BD || b.hidden != A::BW || b.rigidity_depth != A::RD || b.rigidity_hidden != A::RW) return false;
    if (!b.network || !b.rigidity_network) return false;
    for (int i = 0; i < A::BD; ++i)
        if (!linear_is(b.network[i], (i == A::BD - 1) ? 3 : A::BW, (i == 0) ? 3 + A::LAT : A::BW, i != A::BD - 1)) return false;
    for (int i = 0; i < A::RD; ++i)
        if (!linear_is(b.rigidity_network[i], (i == A::RD - 1) ? 1 : A::RW, (i == 0) ? 3 : A::RW, true)) return false;
    return true;
}

// Does (desc, mlp) match compiled architecture A?  (ArchDefault: 8x256 trunk with skip after layer 4, L = 10, bender
// 5x64, rigidity 3x32, latent 32, optional view-dependent head with L = 4; ArchDeepBend: the same with a 7-layer bender.)
template <class A>
int check_arch_t(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m) {
    if (d.precision < 0 || d.precision > 2) return NRNERF_ERR_INVALID;
    if (d.multires != A::L) return NRNERF_ERR_UNSUPPORTED;
    if ((m.time_conditioned != 0) != (A::TCB != 0)) return NRNERF_ERR_UNSUPPORTED;
    if (A::TCB && d.bender) return NRNERF_ERR_UNSUPPORTED;      // the reference forbids the combination (train.py:574-576)
    if (m.use_viewdirs && d.multires_views != A::LV) return NRNERF_ERR_UNSUPPORTED;
    if (m.depth != A::D || m.width != A::W || m.skip != A::SKIP) return NRNERF_ERR_UNSUPPORTED;
    if (m.output_ch != 4 && m.output_ch != 5) return NRNERF_ERR_UNSUPPORTED;
    if (!m.pts_linears) return NRNERF_ERR_INVALID;
    const int enc = 3 + 6 * A::L + (A::TCB ? A::LAT : 0);
    if (A::TCB && m.pts_linears[0].in_features != enc) return NRNERF_ERR_UNSUPPORTED;     // other latent size
    for (int i = 0; i < A::D; ++i) {
        const int in_f = (i == 0) ? enc : ((i - 1 == A::SKIP) ? A::W + enc : A::W);
        if (!linear_is(m.pts_linears[i], A::W, in_f, true)) return NRNERF_ERR_INVALID;
    }
    if (m.use_viewdirs) {
        if (m.output_ch != 4) return NRNERF_ERR_INVALID;
        if (!linear_is(m.alpha_linear, 1, A::W, true) || !linear_is(m.feature_linear, A::W, A::W, true) ||
            !linear_is(m.views_linear, A::W / 2, A::W + 3 + 6 * A::LV, true) || !linear_is(m.rgb_linear, 3, A::W / 2, true))
            return NRNERF_ERR_INVALID;
    } else if (!linear_is(m.output_linear, m.output_ch, A::W, true)) {
        return NRNERF_ERR_INVALID;
    }
    if (d.bender) {
        const nrnerf_bender_desc& b = *d.bender;
        if (b.latent_size != A::LAT || b.depth != A::BD || b.hidden != A::BW || b.rigidity_depth != A::RD ||
            b.rigidity_hidden != A::RW)
            return NRNERF_ERR_UNSUPPORTED;
        if (!bender_matches<A>(b)) return NRNERF_ERR_INVALID;      // (the shape is A's: a missing or mis-sized layer)
    }
    return NRNERF_OK;
}

template <class A>
void pack_arch(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m, PackedPass& out, bool bender_only = false,
               const FlatLayout* lay = nullptr) {
    const bool bend = d.bender != nullptr, views = m.use_viewdirs != 0;
    auto go = [&](auto sh) {
        using SH = decltype(sh);
        if (bender_only) pack_pass<SH, A, true, false, false>(d, m, d.precision, out, lay);       // nrnerf_bend.h
        else if (bend && views) pack_pass<SH, A, true, true>(d, m, d.precision, out, lay);
        else if (bend) pack_pass<SH, A, true, false>(d, m, d.precision, out, lay);
        else if (views) pack_pass<SH, A, false, true>(d, m, d.precision, out, lay);
        else pack_pass<SH, A, false, false>(d, m, d.precision, out, lay);
    };
    if (d.precision == NRNERF_PREC_F32) go(ShapeF32{});
    else if (d.precision == NRNERF_PREC_BF16) go(Shape16Fast{});      // single-product bender (nrnerf_plan.h Shape::SPLIT)
    else go(Shape16{});
}

// picks the compiled architecture (nrnerf_plan.h ArchById) the description matches; *arch_id receives its id
int pack_dispatch(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m, PackedPass& out, int* arch_id = nullptr,
                  bool bender_only = false, const FlatLayout* lay = nullptr) {
    int rc = check_arch_t<ArchDefault>(d, m);
    if (rc == NRNERF_OK) {
        pack_arch<ArchDefault>(d, m, out, bender_only, lay);
        if (arch_id) *arch_id = 0;
        return NRNERF_OK;
    }
    if (rc == NRNERF_ERR_UNSUPPORTED && !d.bender && m.time_conditioned) {
        const int rc2 = check_arch_t<ArchTimeCond>(d, m);
        if (rc2 == NRNERF_OK) {
            pack_arch<ArchTimeCond>(d, m, out, false, lay);
            if (arch_id) *arch_id = 2;
            return NRNERF_OK;
        }
        return rc2;
    }
    if (rc == NRNERF_ERR_UNSUPPORTED && d.bender) {     // arch 1 is a bender variant: only compiled with a bender
        const int rc1 = check_arch_t<ArchDeepBend>(d, m);
        if (rc1 == NRNERF_OK) {
            pack_arch<ArchDeepBend>(d, m, out, bender_only, lay);
            if (arch_id) *arch_id = 1;
            return NRNERF_OK;
        }
        if (rc1 != NRNERF_ERR_UNSUPPORTED) return rc1;
    }
    if (rc == NRNERF_ERR_UNSUPPORTED && !m.time_conditioned && !m.use_viewdirs) {      // arch 5: netwidth 128, no view-dependent head
        const int rc5 = check_arch_t<ArchNarrow>(d, m);
        if (rc5 == NRNERF_OK) {
            pack_arch<ArchNarrow>(d, m, out, bender_only, lay);
            if (arch_id) *arch_id = 5;
            return NRNERF_OK;
        }
        if (rc5 != NRNERF_ERR_UNSUPPORTED) return rc5;
    }
    return rc;
}
// ------------------------------------------------------------------------------------------
// Any other architecture: the run-time-parameterised kernel of nrnerf_generic.h.  The reference builds NeRF(D, W) for any
// --netdepth / --netwidth (and _fine), any --multires / --multires_views, a bender for any --ray_bending_latent_size
// (train.py:1004-1010, 1060, 1133-1139, 564-630); what is not one of the compiled shapes gets a layer PROGRAM here: per layer
// the fragment offset of its weights, its sources among the LDS buffers E (network input) / H (hidden) / V (second input) and
// its destination.  Columns keep the reference's order, so a fragment element is W[32 t + i][first column of the source + k].
// ------------------------------------------------------------------------------------------
struct GenProgram {
    GenArgs proto{};          // mode, L, LV, lat, layers, ke / kv / kh filled in; pointers are per launch
    PackedPass pk;
};
int pad16(int v) { return (v + 15) / 16 * 16; }
struct GenSource { int buf, col0, n; };

// one layer into the program and the packed images.  16-bit precisions: fragments read against E / V are f16, against H the
// model's type (nrnerf_generic.h).
// (t_wbase >= 0: `lin` is a TRANSPOSED copy of rows [t_row0, t_row0 + lin.in_features ... ) -- element (row r, column k) of `lin` is the
//  original layer's W[k][t_col0 + r], whose flat-vector position is t_wbase + k * t_orig_in + t_col0 + r: the device-side refresh
//  (nrnerf_model_update_device) then fills the backward-data images of a non-compiled architecture like every other image)
// (a transposed layer's place in the flat parameter buffer: element (output row r, source column k) of the layer is element
//  (k - kshift, col0 + r) of the ORIGINAL matrix at wbase, whose rows have orig_in elements; columns k < kshift are constant zeros)
struct GenTSrc { int64_t wbase = -1; int orig_in = 0, col0 = 0, kshift = 0; };
void gen_add_layer(GenProgram& g, int precision, const nrnerf_linear& lin, GenSource a, GenSource b, int dst, int relu, int o_col, const FlatLayout* lay,
                   const GenTSrc* ta = nullptr, const GenTSrc* tb = nullptr) {
    if (g.proto.n_layers >= GEN_MAX_LAYERS) throw std::logic_error("generic program too long");
    const bool f32 = precision == NRNERF_PREC_F32;
    // a fragment = 64 lanes x 16 bytes in every precision: 8 16-bit k per lane (one MFMA), or 4 fp32 k per lane (four 32x32x2 MFMAs:
    // lane half h holds k = 8 s + 4 h + e), see nrnerf_generic.h::GenTypes
    const int KH = f32 ? 4 : 8, KS = 2 * KH, FB = 1024;
    GenLayer& ly = g.proto.layer[g.proto.n_layers++];
    ly.w_frag = (int)(g.pk.stream.size() / FB);
    ly.bias_tile = (int)(g.pk.bias.size() / 32);
    ly.nt = (lin.out_features + 31) / 32;
    ly.src0 = a.buf; ly.ns0 = (a.n + KS - 1) / KS;
    ly.src1 = b.buf; ly.ns1 = (b.n + KS - 1) / KS;
    ly.dst = dst; ly.relu = relu; ly.o_col = o_col; ly.o_rows = lin.out_features;
    ly.save_idx = -1; ly.mask_idx = -1; ly.boff0 = 0; ly.boff1 = 0;
    if (ly.nt > GEN_WAVES * GEN_MAXT || a.col0 + a.n > lin.in_features || b.col0 + b.n > lin.in_features) throw std::logic_error("generic layer out of range");
    const int ns = ly.ns0 + ly.ns1;
    const bool transposed = ta != nullptr;
    const Source src = transposed ? Source{&lin, -1, -1} : source_of(lay, &lin);
    FragWriter wr(g.pk, lay, FB, f32 ? 4 : 2, 32);
    wr.grow((size_t)ly.nt * ns * FB, ly.nt, FMT_F32);
    for (int t = 0; t < ly.nt; ++t) {
        for (int sl = 0; sl < ns; ++sl) {
            const bool first = sl < ly.ns0;
            const GenSource& from = first ? a : b;
            const GenTSrc* ts = first ? ta : tb;
            const int s = first ? sl : sl - ly.ns0;
            const Fmt fmt = f32 ? FMT_F32 : ((precision == NRNERF_PREC_F16 || from.buf != GB_H) ? FMT_F16 : FMT_BF16);
            const FragWriter::Frag fr = wr.frag((size_t)ly.w_frag + (size_t)t * ns + sl);
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 31, h = lane >> 5, row = 32 * t + i;
                for (int e = 0; e < KH; ++e) {
                    const int k = s * KS + h * KH + e;
                    const bool live = row < lin.out_features && k < from.n;
                    if (!transposed || !live) { fr.put(lane * KH + e, src, live ? row : -1, from.col0 + k, fmt); continue; }
                    const int64_t at = (ts && ts->wbase >= 0 && k >= ts->kshift) ? ts->wbase + (int64_t)(k - ts->kshift) * ts->orig_in + ts->col0 + row : -1;
                    fr.put(lane * KH + e, lin.weight[(size_t)row * lin.in_features + from.col0 + k], at, fmt);
                }
            }
        }
        wr.bias(ly.bias_tile + t, src, [&](int j) { const int row = 32 * t + bias_row32(j); return row < lin.out_features ? row : -1; });
    }
}
void gen_finish(GenProgram& g) {
    const int FB = 1024;
    g.pk.frag_bytes = FB; g.pk.slot_bytes = FB;
    g.pk.ntiles = (int)(g.pk.bias.size() / 32);
    g.proto.n_bias_tiles = g.pk.ntiles;
    g.pk.nunits = (int)(g.pk.stream.size() / FB);
    g.pk.unit_off.assign(1, 0);
}

int gen_skip(const nrnerf_mlp_desc& m) { return (m.skip >= 0 && m.skip <= m.depth - 2) ? m.skip : -1; }
// what the generic kernel takes (everything else: NRNERF_ERR_UNSUPPORTED, i.e. the reference's own function)
int gen_check_mlp(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m) {
    if (d.precision < 0 || d.precision > 2) return NRNERF_ERR_INVALID;
    if (!m.pts_linears || m.depth < 1 || m.width < 1) return NRNERF_ERR_INVALID;
    if (d.multires < 0 || d.multires > 16 || m.width > GEN_MAX_W || m.depth > 16) return NRNERF_ERR_UNSUPPORTED;
    if (m.time_conditioned && d.bender) return NRNERF_ERR_UNSUPPORTED;                       // train.py:574-576
    const int enc = 3 + 6 * d.multires;
    const int lat = m.time_conditioned ? m.pts_linears[0].in_features - enc : 0;
    if (lat < 0 || lat > 64 || pad16(enc + lat) > GEN_MAX_E) return NRNERF_ERR_UNSUPPORTED;
    // NeRF.forward concatenates [input, h] after layer `skip` whatever follows (rnh:277-282): after the LAST layer the
    // reference's own head fails on the wider vector; a skip index beyond the depth never triggers
    if (m.skip == m.depth - 1) return NRNERF_ERR_UNSUPPORTED;
    const int skip = gen_skip(m);
    for (int i = 0; i < m.depth; ++i) {
        const int in_f = (i == 0) ? enc + lat : ((skip >= 0 && i - 1 == skip) ? m.width + enc + lat : m.width);
        if (!linear_is(m.pts_linears[i], m.width, in_f, true)) return NRNERF_ERR_INVALID;
    }
    if (m.use_viewdirs) {
        if (d.multires_views < 0 || d.multires_views > 10 || m.output_ch != 4) return NRNERF_ERR_UNSUPPORTED;
        const int half = m.views_linear.out_features;
        if (!linear_is(m.alpha_linear, 1, m.width, true) || !linear_is(m.feature_linear, m.width, m.width, true) || half < 1 || half > GEN_MAX_W ||
            !linear_is(m.views_linear, half, m.width + 3 + 6 * d.multires_views, true) || !linear_is(m.rgb_linear, 3, half, true))
            return NRNERF_ERR_INVALID;
    } else {
        if (m.output_ch < 4 || m.output_ch > 5) return NRNERF_ERR_UNSUPPORTED;
        if (!linear_is(m.output_linear, m.output_ch, m.width, true)) return NRNERF_ERR_INVALID;
    }
    return NRNERF_OK;
}
int gen_check_bender(const nrnerf_bender_desc& b) {
    if (!b.network || !b.rigidity_network || b.depth < 2 || b.rigidity_depth < 2) return NRNERF_ERR_INVALID;
    if (b.latent_size < 0 || b.latent_size > 64 || b.hidden < 1 || b.hidden > GEN_MAX_W || b.rigidity_hidden < 1 || b.rigidity_hidden > GEN_MAX_W ||
        b.depth + b.rigidity_depth > GEN_MAX_LAYERS)
        return NRNERF_ERR_UNSUPPORTED;
    for (int i = 0; i < b.depth; ++i) {
        const int in_f = (i == 0) ? 3 + b.latent_size : b.hidden, out_f = (i == b.depth - 1) ? 3 : b.hidden;
        if (!linear_is(b.network[i], out_f, in_f, i != b.depth - 1)) return NRNERF_ERR_INVALID;
    }
    for (int i = 0; i < b.rigidity_depth; ++i) {
        const int in_f = (i == 0) ? 3 : b.rigidity_hidden, out_f = (i == b.rigidity_depth - 1) ? 1 : b.rigidity_hidden;
        if (!linear_is(b.rigidity_network[i], out_f, in_f, true)) return NRNERF_ERR_INVALID;
    }
    return NRNERF_OK;
}
// NeRF.forward (rnh:240-314) as a layer program
void gen_pack_mlp(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m, GenProgram& g, const FlatLayout* lay) {
    const int enc = 3 + 6 * d.multires, lat = m.time_conditioned ? m.pts_linears[0].in_features - enc : 0, in_w = enc + lat, W = m.width;
    g.proto.mode = 1; g.proto.L = d.multires; g.proto.LV = m.use_viewdirs ? d.multires_views : -1; g.proto.lat = lat;
    g.proto.ke = pad16(in_w);
    g.proto.kv = m.use_viewdirs ? pad16(3 + 6 * d.multires_views) : 16;
    int widest = W;
    const int skip = gen_skip(m);
    const GenSource none{GB_H, 0, 0};
    for (int i = 0; i < m.depth; ++i) {
        if (i == 0) gen_add_layer(g, d.precision, m.pts_linears[0], GenSource{GB_E, 0, in_w}, none, GB_H, 1, 0, lay);
        else if (skip >= 0 && i - 1 == skip)            // h = cat([input_pts, h]) (rnh:280-282): columns [input | hidden]
            gen_add_layer(g, d.precision, m.pts_linears[i], GenSource{GB_E, 0, in_w}, GenSource{GB_H, in_w, W}, GB_H, 1, 0, lay);
        else gen_add_layer(g, d.precision, m.pts_linears[i], GenSource{GB_H, 0, W}, none, GB_H, 1, 0, lay);
    }
    if (m.use_viewdirs) {                              // rnh:284-304
        const int half = m.views_linear.out_features, dv = 3 + 6 * d.multires_views;
        widest = imax(widest, half);
        gen_add_layer(g, d.precision, m.alpha_linear, GenSource{GB_H, 0, W}, none, GB_O, 0, 3, lay);
        gen_add_layer(g, d.precision, m.feature_linear, GenSource{GB_H, 0, W}, none, GB_H, 0, 0, lay);
        gen_add_layer(g, d.precision, m.views_linear, GenSource{GB_H, 0, W}, GenSource{GB_V, W, dv}, GB_H, 1, 0, lay);   // cat([feature, input_views])
        gen_add_layer(g, d.precision, m.rgb_linear, GenSource{GB_H, 0, half}, none, GB_O, 0, 0, lay);
    } else {
        gen_add_layer(g, d.precision, m.output_linear, GenSource{GB_H, 0, W}, none, GB_O, 0, 0, lay);
    }
    g.proto.kh = (widest + 31) / 32 * 32;
    for (int i = 0; i < m.depth; ++i) g.proto.layer[i].save_idx = i;        // (training: layer i's activations, only with GenArgs::save set)
    if (m.use_viewdirs) {                                                   // + feature_linear's outputs (slot D) and the colour branch's activations (slot D + 1)
        g.proto.layer[m.depth + 1].save_idx = m.depth;
        g.proto.layer[m.depth + 2].save_idx = m.depth + 1;
    }
    gen_finish(g);
}
// Backward-data of a plain-headed NeRF (training of a non-compiled architecture): the forward's layers in reverse order with TRANSPOSED
// weights, no biases, run by the same kernel (GenArgs::mode 2).  H starts as the rows of d raw; output_linear^T gives d h_{D-1}, masked
// by the forward activation of layer D - 1 = d pre_{D-1} (saved as index D - 1); pts_linears[i]^T takes d pre_i to d pre_{i-1} (mask:
// activation i - 1); the layer behind the skip connection has [input | hidden] columns: its input part goes straight to memory
// (GB_OUT1: the encoding's gradient), its hidden part goes on; pts_linears[0]^T ends in the encoding's gradient (GB_OUT0).
bool gen_trainable(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m) {
    if (d.precision == NRNERF_PREC_F16 || m.width % 4 != 0 || m.depth < 1) return false;
    if (m.time_conditioned && (d.bender || m.pts_linears[0].in_features > 512)) return false;
    if (m.use_viewdirs) return m.feature_linear.out_features == m.width && m.views_linear.in_features == m.width + 3 + 6 * d.multires_views &&
                               m.views_linear.out_features <= m.width && m.depth + 5 <= GEN_MAX_LAYERS && (m.width + 31) / 32 * 32 + 32 <= GEN_MAX_W;
    return m.output_ch >= 4 && m.output_ch <= 5 && m.depth + 2 <= GEN_MAX_LAYERS;          // (layers of the backward-data program)
}
// column of H where mode 2 parks the rows of d raw (plain head: 0 -- they are the first layer's only input; view-dependent head: behind the
// activations, because d sigma is needed again when the colour branch's gradient has come down to h_{D-1})
int gen_draw_col(const nrnerf_mlp_desc& m) { return m.use_viewdirs ? (m.width + 31) / 32 * 32 : 0; }
void gen_pack_mlp_bwd(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m, GenProgram& g, const FlatLayout* lay) {
    // (time-conditioned baseline, rnh:207-209, 273-282: the latent code's columns follow the encoding's in both layers that read the input,
    //  and so do their gradients in the two outputs)
    const int enc = m.time_conditioned ? m.pts_linears[0].in_features : 3 + 6 * d.multires, W = m.width, D = m.depth, skip = gen_skip(m);
    g.proto.mode = 2; g.proto.L = d.multires; g.proto.LV = -1; g.proto.lat = 0;
    g.proto.ke = 16; g.proto.kv = 16;
    const GenSource none{GB_H, 0, 0};
    std::vector<std::vector<float>> keep;           // transposed copies (alive until the fragments are written: gen_add_layer copies)
    auto transposed = [&](const nrnerf_linear& lin, int col0, int ncols) {       // rows = the layer's input columns [col0, col0 + ncols), columns = its outputs
        keep.emplace_back((size_t)ncols * lin.out_features);
        std::vector<float>& t = keep.back();
        for (int r = 0; r < ncols; ++r)
            for (int k = 0; k < lin.out_features; ++k) t[(size_t)r * lin.out_features + k] = lin.weight[(size_t)k * lin.in_features + col0 + r];
        nrnerf_linear lt{};
        lt.weight = t.data(); lt.bias = nullptr; lt.out_features = ncols; lt.in_features = lin.out_features;
        return lt;
    };
    auto add = [&](const nrnerf_linear& lin, int col0, int ncols, int k_in, int dst, int mask_idx, int save_idx, int boff = 0) {
        const nrnerf_linear lt = transposed(lin, col0, ncols);
        const GenTSrc ts{lay ? lay->of(lin.weight) : -1, lin.in_features, col0, 0};
        gen_add_layer(g, d.precision, lt, GenSource{GB_H, 0, k_in}, none, dst, 0, 0, lay, &ts, nullptr);
        GenLayer& ly = g.proto.layer[g.proto.n_layers - 1];
        ly.mask_idx = mask_idx; ly.save_idx = save_idx; ly.boff0 = boff;
    };
    if (m.use_viewdirs) {
        // rgb = rgb_linear(hv), hv = relu(views_linear([feature, enc(dir)])), feature = feature_linear(h), sigma = alpha_linear(h)  (rnh:284-304)
        const int half = m.views_linear.out_features, dv = 3 + 6 * d.multires_views, dc = gen_draw_col(m);
        add(m.rgb_linear, 0, half, 3, GB_H, D + 1, D + 1, dc);                        // d rgb (columns dc .. dc + 2) -> d pre of the colour branch (slot D + 1)
        add(m.views_linear, W, dv, half, GB_OUT2, -1, -1);                            // its direction columns: the direction encoding's gradient, to memory
        add(m.views_linear, 0, W, half, GB_H, -1, D);                                 // its feature columns: d feature (slot D; feature_linear has no relu)
        // d h_{D-1} = feature_linear^T d feature + alpha_linear^T d sigma: ONE layer, columns [d feature | the d raw block, only its column 3 live]
        keep.emplace_back((size_t)W * (W + 4), 0.0f);
        std::vector<float>& t = keep.back();
        for (int r = 0; r < W; ++r) {
            for (int k = 0; k < W; ++k) t[(size_t)r * (W + 4) + k] = m.feature_linear.weight[(size_t)k * W + r];
            t[(size_t)r * (W + 4) + W + 3] = m.alpha_linear.weight[r];
        }
        nrnerf_linear lt{};
        lt.weight = t.data(); lt.bias = nullptr; lt.out_features = W; lt.in_features = W + 4;
        const GenTSrc tf{lay ? lay->of(m.feature_linear.weight) : -1, W, 0, 0}, tal{lay ? lay->of(m.alpha_linear.weight) : -1, W, 0, 3};
        gen_add_layer(g, d.precision, lt, GenSource{GB_H, 0, W}, GenSource{GB_H, W, 4}, GB_H, 0, 0, lay, &tf, &tal);
        GenLayer& ly = g.proto.layer[g.proto.n_layers - 1];
        ly.mask_idx = D - 1; ly.save_idx = D - 1; ly.boff1 = dc;
    } else {
        add(m.output_linear, 0, W, 4, GB_H, D - 1, D - 1);                             // d raw (rgb, sigma; a 5th channel never reaches a loss) -> d pre_{D-1}
    }
    for (int i = D - 1; i >= 1; --i) {
        if (skip >= 0 && i - 1 == skip) {
            add(m.pts_linears[i], 0, enc, W, GB_OUT1, -1, -1);                         // input part: gradient of the encoding, to memory
            add(m.pts_linears[i], enc, W, W, GB_H, i - 1, i - 1);                      // hidden part: d pre_{i-1}
        } else {
            add(m.pts_linears[i], 0, W, W, GB_H, i - 1, i - 1);
        }
    }
    add(m.pts_linears[0], 0, enc, W, GB_OUT0, -1, -1);
    g.proto.kh = m.use_viewdirs ? gen_draw_col(m) + 32 : (imax(W, 16) + 31) / 32 * 32;
    gen_finish(g);
}
// ray_bending.forward (rnh:507-577): always packed (and run) in fp32
void gen_pack_bender(const nrnerf_bender_desc& b, GenProgram& g, const FlatLayout* lay) {
    g.proto.mode = 0; g.proto.L = 0; g.proto.LV = -1; g.proto.lat = b.latent_size;
    g.proto.ke = pad16(3 + b.latent_size); g.proto.kv = 16;
    const GenSource none{GB_H, 0, 0};
    for (int i = 0; i < b.depth; ++i) {
        const bool last = i == b.depth - 1;
        gen_add_layer(g, NRNERF_PREC_F32, b.network[i], i == 0 ? GenSource{GB_E, 0, 3 + b.latent_size} : GenSource{GB_H, 0, b.hidden}, none,
                      last ? GB_O : GB_H, last ? 0 : 1, 0, lay);
    }
    for (int i = 0; i < b.rigidity_depth; ++i) {
        const bool last = i == b.rigidity_depth - 1;
        gen_add_layer(g, NRNERF_PREC_F32, b.rigidity_network[i], i == 0 ? GenSource{GB_V, 0, 3} : GenSource{GB_H, 0, b.rigidity_hidden}, none,
                      last ? GB_O : GB_H, last ? 0 : 1, 3, lay);
    }
    g.proto.kh = (imax(b.hidden, b.rigidity_hidden) + 31) / 32 * 32;
    gen_finish(g);
}

// algorithmic MACs per sample, unpadded
double algo_macs(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m) {
    double macs = 0;
    for (int i = 0; i < m.depth; ++i) macs += (double)m.pts_linears[i].in_features * m.pts_linears[i].out_features;
    if (m.use_viewdirs) {
        for (const nrnerf_linear* l : {&m.alpha_linear, &m.feature_linear, &m.views_linear, &m.rgb_linear})
            macs += (double)l->in_features * l->out_features;
    } else {
        macs += (double)m.output_linear.in_features * m.output_linear.out_features;
    }
    if (d.bender) {
        for (int i = 0; i < d.bender->depth; ++i) macs += (double)d.bender->network[i].in_features * d.bender->network[i].out_features;
        for (int i = 0; i < d.bender->rigidity_depth; ++i)
            macs += (double)d.bender->rigidity_network[i].in_features * d.bender->rigidity_network[i].out_features;
    }
    return macs;
}

constexpr int NRN_RING_LAG_HOST = 2;      // NRN_RING_LAG of nrnerf_net_impl.h (device header): units of DMA lead behind the ring's read position

// The two extra weight images of the split-bender path: the fine network without its bender layers (same trunk for the
// 5- and the 7-layer bender: compiled architecture 0 without bender) and the bender + rigidity layers alone.
int pack_split(const nrnerf_model_desc& d, PackedPass& trunk, PackedPass& bend, PackedPass* coarse_trunk = nullptr,
               const FlatLayout* lay = nullptr) {
    const nrnerf_mlp_desc& fm = d.fine ? *d.fine : *d.coarse;
    nrnerf_model_desc d2 = d;
    d2.bender = nullptr;
    int rc = pack_dispatch(d2, fm, trunk, nullptr, false, lay);
    if (rc != NRNERF_OK) return rc;
    if (coarse_trunk) {
        rc = pack_dispatch(d2, *d.coarse, *coarse_trunk, nullptr, false, lay);
        if (rc != NRNERF_OK) return rc;
    }
    return pack_dispatch(d, fm, bend, nullptr, /*bender_only=*/true, lay);
}

// transposed trunk weights for the backward-data kernel; eligible models only (see nrnerf_model::train_ok)
bool training_eligible(const nrnerf_model_desc& d, int arch_id) {
    // (with the view-dependent head: the directions are an input of the trunk's training kernels -- finite differences, the rays' own, or
    //  the exact Jacobian directions, whose tangent and its gradient come from nrnerf_bender_divergence_* (tangent / g_tangent))
    // (time-conditioned baseline, architecture 2: trained through the plain trunk's kernels, the latent columns of its two
    //  input layers as per-ray biases -- pack_pass, tcb_shift)
    return (arch_id <= 2 || arch_id == 5) && d.precision != NRNERF_PREC_F16;
}
int tcb_shift_of(const nrnerf_mlp_desc& mlp) {      // latent columns of a time-conditioned trunk (0: plain trunk)
    return mlp.time_conditioned ? mlp.pts_linears[0].in_features - (3 + 6 * ArchDefault::L) : 0;
}
void pack_bwd(const nrnerf_model_desc& d, const nrnerf_mlp_desc& mlp, PackedPass& out, const FlatLayout* lay = nullptr) {
    const bool narrow = mlp.width == ArchNarrow::W, views = mlp.use_viewdirs != 0;      // (no view-dependent head at width 128)
    const int ts = tcb_shift_of(mlp);
    if (d.precision == NRNERF_PREC_F32) {
        if (narrow) pack_pass_bwd<ShapeF32, ArchNarrow>(mlp, d.precision, out, lay, ts);
        else if (views) pack_pass_bwd<ShapeF32, ArchDefault, true>(mlp, d.precision, out, lay, ts);
        else pack_pass_bwd<ShapeF32, ArchDefault>(mlp, d.precision, out, lay, ts);
    } else {
        if (narrow) pack_pass_bwd<Shape16, ArchNarrow>(mlp, d.precision, out, lay, ts);
        else if (views) pack_pass_bwd<Shape16, ArchDefault, true>(mlp, d.precision, out, lay, ts);
        else pack_pass_bwd<Shape16, ArchDefault>(mlp, d.precision, out, lay, ts);
    }
}
// ---- the width-class trunk kernel for architectures outside the compiled set (nrnerf_gx16.h, nrnerf_gx16_plan.h)
// does it take this network?  16-bit modes, no view-dependent head, no time conditioning, <= 10 encoding frequencies, 4 / 5 output channels
bool gx16_eligible(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m) {
    if (d.precision != NRNERF_PREC_BF16 && d.precision != NRNERF_PREC_F16) return false;
    if (m.time_conditioned || d.multires < 0 || d.multires > GX_MAX_L) return false;
    if (m.width < 1 || m.width > 512 || m.depth < 1 || m.depth > 16) return false;
    if (m.use_viewdirs) {            // view-dependent head: <= 4 direction frequencies, finite-difference directions, views layer <= half the class
        if (d.multires_views < 0 || d.multires_views > GX_MAX_LV || (d.exact_viewdirs && d.bender)) return false;
        if (m.views_linear.out_features > gx_width_class(m.width) / 2 || m.feature_linear.out_features != m.width) return false;
        return true;
    }
    if (m.output_ch != 4 && m.output_ch != 5) return false;
    return true;
}
// The stream walk of both width-class images: the layers' (`kinds`) fragment blocks back to back, each padded to gx_layer_units()
// units, + a copy of the stream's first RING - LAG units behind the last (the ring runs on into the next iteration's first units).
// `layer(wr, li, T, frag0, tile0)` fills layer li (single-layer tables T) from fragment frag0 / bias tile tile0 on.
template <class Layer>
void pack_gx16_stream(const nrnerf_model_desc& d, const nrnerf_mlp_desc& mlp, const std::vector<int>& kinds, PackedPass& out, GxMeta& meta,
                      const FlatLayout* lay, Layer layer) {
    using SH = Shape16Fast;
    constexpr int TAIL = RING - NRN_RING_LAG_HOST;
    const int wc = gx_width_class(mlp.width);
    int units = 0, tiles = 0, mfma = 0;
    for (int k : kinds) { units += gx_layer_units(wc, k); tiles += gx_layer_tiles(wc, k); }
    FragWriter wr(out, lay, SH::FRAG_BYTES, 2, 16);
    wr.begin(units + TAIL, SH::UNIT_BYTES, (size_t)(units + TAIL) * SH::UNIT_BYTES, tiles, FMT_BF16, true);
    size_t unit0 = 0, tile0 = 0;
    for (size_t li = 0; li < kinds.size(); ++li) {
        const Tables T = build_tables_gx(wc, kinds[li]);
        layer(wr, li, T, unit0 * SH::UNIT_FRAGS, tile0);
        mfma += T.layers[0].ns * T.layers[0].nt;
        unit0 += gx_layer_units(wc, kinds[li]);
        tile0 += T.layers[0].nt;
    }
    wr.done(mfma);
    wr.append_ring_tail(units, TAIL);
    out.mfma_per_block = mfma;
    meta.wc = wc; meta.depth = mlp.depth; meta.skip = gen_skip(mlp); meta.L = d.multires; meta.n_bias_tiles = tiles; meta.views = 0; meta.LV = 0;
}
// The forward image, layers in evaluation order: IN, then HID / SKIP per pts_linears[i], then HEAD (view-dependent head: VIEWS = [the folded
// views layer | alpha_linear in the last tile], then RGB).  Fragment element (lane (r, g), e) of (tile t, k-step s): W[row][col] with the
// maps of nrnerf_gx16_plan.h; encoding k-steps f16, hidden ones the model's type; bias table [tile][16 rows].
void pack_gx16(const nrnerf_model_desc& d, const nrnerf_mlp_desc& mlp, PackedPass& out, GxMeta& meta, const FlatLayout* lay = nullptr) {
    const int D = mlp.depth, skip = gen_skip(mlp), L = d.multires, enc = 3 + 6 * L, W = mlp.width;
    const bool views = mlp.use_viewdirs != 0;
    std::vector<int> kinds;
    kinds.push_back(GX_IN);
    for (int i = 1; i < D; ++i) kinds.push_back((i - 1 == skip) ? GX_SKIP : GX_HID);
    if (views) { kinds.push_back(GX_VIEWS); kinds.push_back(GX_RGB); }
    else kinds.push_back(GX_HEAD);
    std::unique_ptr<FoldedViews> folded;
    if (views) folded.reset(new FoldedViews(mlp));
    const int EV = 3 + 6 * d.multires_views;
    pack_gx16_stream(d, mlp, kinds, out, meta, lay, [&](FragWriter& wr, size_t li, const Tables& T, size_t frag0, size_t tile0) {
        const int kind = kinds[li];
        const LayerSpec& sp = T.layers[0];
        const Source src0 = kind == GX_VIEWS ? folded_source(lay, mlp, *folded)
                                             : source_of(lay, kind == GX_HEAD ? &mlp.output_linear : (kind == GX_RGB ? &mlp.rgb_linear : &mlp.pts_linears[li]));
        for (int t = 0; t < sp.nt; ++t) {
            const bool alpha_tile = kind == GX_VIEWS && t == sp.nt - 1;
            const Source src = alpha_tile ? source_of(lay, &mlp.alpha_linear) : src0;
            const int out_f = src.lin->out_features, in_f = src.lin->in_features;
            auto row_of = [&](int r) {
                if (alpha_tile) return alpha_tile_row(r);
                if (kind == GX_HEAD) return r < out_f ? r : -1;
                if (kind == GX_RGB) return r < 3 ? r : -1;
                return (16 * t + r < out_f) ? 16 * t + r : -1;
            };
            for (int s = 0; s < sp.ns; ++s) {
                const FragWriter::Frag fr = wr.frag(frag0 + (size_t)T.tiles[t].gbase + (size_t)s * T.tiles[t].gstride);
                const bool enc_step = ((kind == GX_IN || kind == GX_SKIP) && s < GX_NS_E) || (kind == GX_VIEWS && s == 0);
                const Fmt fmt = (d.precision == NRNERF_PREC_F16 || enc_step) ? FMT_F16 : FMT_BF16;
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = lane & 15, g = lane >> 4;
                    const int row = row_of(r);
                    for (int e = 0; e < 8; ++e) {
                        int col;
                        if (kind == GX_VIEWS) {            // folded columns: hidden (W) first, then the direction encoding's (EV); alpha: hidden only
                            if (s == 0) { const int c = gx_enc_col(d.multires_views, 0, g, e); col = (c < 0 || alpha_tile) ? -1 : (in_f - EV) + c; }
                            else { const int c = x16_hidden_feature(s - 1, g, e); col = c < W ? c : -1; }
                        } else if (kind == GX_RGB) {
                            col = x16_hidden_feature(s, g, e);
                        } else if (enc_step) col = gx_enc_col(L, s, g, e);
                        else {
                            const int c = x16_hidden_feature(kind == GX_SKIP ? s - GX_NS_E : s, g, e);
                            col = c < W ? (kind == GX_SKIP ? enc + c : c) : -1;
                        }
                        fr.put(lane * 8 + e, src, row, col < in_f ? col : -1, fmt);
                    }
                }
            }
            wr.bias(tile0 + t, src, row_of);
        }
    });
    meta.views = views ? 1 : 0; meta.LV = d.multires_views;
}

// The backward-data program of the same trunk (nrnerf_gx16_bwd.h; plain head, bf16): output_linear^T, pts_linears[D-1 .. 1]^T, pts_linears[0]^T,
// every fragment element (tile t, row r, k-slot (s, g, e)) = W[k feature][column of output row] -- the k feature of a hidden k-step is
// x16_hidden_feature(s, g, e) (the operand order d z is handed on in), of the d raw k-step the channel 8 g + e < 4; an output row is a hidden
// feature 16 t + r, or -- the four tiles in front of them in the two layers that read the encoding -- the encoding's slot position.
// No biases (the table is zeros).
void pack_gx16_bwd(const nrnerf_model_desc& d, const nrnerf_mlp_desc& mlp, PackedPass& out, GxMeta& meta, const FlatLayout* lay = nullptr) {
    const int D = mlp.depth, skip = gen_skip(mlp), L = d.multires, enc = 3 + 6 * L, W = mlp.width;
    std::vector<int> kinds, layer_of;
    kinds.push_back(GX_BHEAD); layer_of.push_back(-1);
    for (int i = D - 1; i >= 1; --i) { kinds.push_back((i - 1 == skip) ? GX_BSKIP : GX_BHID); layer_of.push_back(i); }
    kinds.push_back(GX_BIN); layer_of.push_back(0);
    pack_gx16_stream(d, mlp, kinds, out, meta, lay, [&](FragWriter& wr, size_t li, const Tables& T, size_t frag0, size_t) {
        const int kind = kinds[li];
        const LayerSpec& sp = T.layers[0];
        const Source src = source_of(lay, kind == GX_BHEAD ? &mlp.output_linear : &mlp.pts_linears[layer_of[li]]);
        const int out_f = src.lin->out_features, in_f = src.lin->in_features;
        const int enc_tiles = (kind == GX_BSKIP || kind == GX_BIN) ? 4 : 0;
        for (int t = 0; t < sp.nt; ++t) {
            // the column of the layer's weight this output row is the gradient of (-1: none)
            auto col_of = [&](int r) {
                if (t < enc_tiles) return gx_enc_col_of_pos(L, 16 * t + r);
                const int f = 16 * (t - enc_tiles) + r;
                if (f >= W || kind == GX_BIN) return -1;
                return kind == GX_BSKIP ? enc + f : f;
            };
            for (int s = 0; s < sp.ns; ++s) {
                const FragWriter::Frag fr = wr.frag(frag0 + (size_t)T.tiles[t].gbase + (size_t)s * T.tiles[t].gstride);
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = lane & 15, g = lane >> 4;
                    const int col = col_of(r);
                    for (int e = 0; e < 8; ++e) {
                        int row;                     // the weight's ROW = the k feature
                        if (kind == GX_BHEAD) row = (g == 0 && e < 4) ? e : -1;
                        else { const int c = x16_hidden_feature(s, g, e); row = c < W ? c : -1; }
                        fr.put(lane * 8 + e, src, row < out_f ? row : -1, col < in_f ? col : -1, FMT_BF16);
                    }
                }
            }
        }
    });
}
// which trunks the x16 training kernels take (forward with saves: gx16_kernel<.., SAVE>; backward-data: gx16_bwd_kernel): bf16, plain head, no
// latent input columns, width % 4 == 0 (rows of whole 8-byte pieces)
bool gx16_trainable(const nrnerf_model_desc& d, const nrnerf_mlp_desc& m) {
    return d.precision == NRNERF_PREC_BF16 && gx16_eligible(d, m) && !m.use_viewdirs && !m.time_conditioned && m.width % 4 == 0;
}

// ---- models of an architecture outside the compiled set (nrnerf_generic.h)
int gen_pack_all(const nrnerf_model_desc& d, const FlatLayout* lay, GenProgram& gb, GenProgram& gc, GenProgram& gf) {
    // exact Jacobian view directions (rnh:358-385) off the compiled set: the tangent J d comes from the bender's compiled divergence kernel
    // (ray mode of bend_div_fwd), so the BENDER must have one of the two compiled shapes, and the handle its training images (not "f16")
    if (d.exact_viewdirs && d.bender && d.coarse->use_viewdirs &&
        (d.precision == NRNERF_PREC_F16 || !(bender_matches<ArchDefault>(*d.bender) || bender_matches<ArchDeepBend>(*d.bender))))
        return NRNERF_ERR_UNSUPPORTED;
    int rc = gen_check_mlp(d, *d.coarse);
    if (rc == NRNERF_OK && d.fine) rc = gen_check_mlp(d, *d.fine);
    if (rc == NRNERF_OK && d.fine && (d.fine->time_conditioned != 0) != (d.coarse->time_conditioned != 0)) rc = NRNERF_ERR_INVALID;
    if (rc == NRNERF_OK && d.bender) rc = gen_check_bender(*d.bender);
    if (rc != NRNERF_OK) return rc;
    if (d.bender) gen_pack_bender(*d.bender, gb, lay);
    gen_pack_mlp(d, *d.coarse, gc, lay);
    if (d.fine) gen_pack_mlp(d, *d.fine, gf, lay);
    return NRNERF_OK;
}
// issued MFMA flops per sample of a layer program (padding included): every (tile, k-slab) is one 32 x 32 x KS MFMA per 32 samples
double gen_mfma_flops_per_sample(const GenArgs& g, bool f32) {
    double f = 0;
    for (int l = 0; l < g.n_layers; ++l) f += (double)g.layer[l].nt * (g.layer[l].ns0 + g.layer[l].ns1) * 2.0 * 32 * (f32 ? 8 : 16);
    return f;
}
// the training images of a bender of compiled shape cb, compiled or generic handle (the fp32 forward plan and the backward plan, whatever the model's precision)
void gen_pack_bender_train(const nrnerf_model_desc& d, int cb, PackedPass& bfw, PackedPass& bbw, const FlatLayout* lay) {
    nrnerf_model_desc d32 = d;
    d32.precision = NRNERF_PREC_F32;
    if (cb == 0) {
        pack_pass<ShapeF32, ArchDefault, true, false, false>(d32, *d.coarse, NRNERF_PREC_F32, bfw, lay);
        pack_pass_bwd_bender<ArchDefault>(*d.bender, bbw, lay);
    } else {
        pack_pass<ShapeF32, ArchDeepBend, true, false, false>(d32, *d.coarse, NRNERF_PREC_F32, bfw, lay);
        pack_pass_bwd_bender<ArchDeepBend>(*d.bender, bbw, lay);
    }
}
// issued MFMA flops per sample of a packed image (padding included): a compiled plan issues mfma_per_block 32 x 32 x (2 | 16) MFMAs per block of 32
// samples, the 16x16x32 kernels mfma_per_block 16 x 16 x 32 MFMAs per block of 16
double mfma32_flops_per_sample(const PackedPass& pk, int precision) {
    const double mfma_flop = 2.0 * 32 * 32 * (precision == NRNERF_PREC_F32 ? 2 : 16);
    return pk.mfma_per_block * mfma_flop / 32.0;
}
double mfma16_flops_per_sample(const PackedPass& pk) { return pk.mfma_per_block * (2.0 * 16 * 16 * 32) / 16.0; }
// The "unit table" nrnerf_pack_host hands out for a layer program: n_layers, per layer the first `per_layer` integers of GenLayer -- 11: what
// the forward programs use; 15: + save / mask slot and source offsets (backward-data programs) -- then the program's scalars `tail`.
void program_unit_table(PackedPass& pk, const GenArgs& p, int per_layer, std::initializer_list<int> tail) {
    pk.unit_off.assign(1, (uint32_t)p.n_layers);
    for (int l = 0; l < p.n_layers; ++l) {
        const GenLayer& y = p.layer[l];
        const int v[15] = {y.w_frag, y.bias_tile, y.nt, y.src0, y.ns0, y.src1, y.ns1, y.dst, y.relu, y.o_col, y.o_rows, y.save_idx, y.mask_idx, y.boff0, y.boff1};
        for (int i = 0; i < per_layer; ++i) pk.unit_off.push_back((uint32_t)v[i]);
    }
    for (int v : tail) pk.unit_off.push_back((uint32_t)v);
    pk.nunits = (int)pk.unit_off.size() - 1;
}

}  // namespace

FlatLayout flat_layout(const nrnerf_model_desc& d) {
    FlatLayout f;
    if (d.bender) {
        for (int i = 0; i < d.bender->depth; ++i) f.add(d.bender->network[i]);
        for (int i = 0; i < d.bender->rigidity_depth; ++i) f.add(d.bender->rigidity_network[i]);
    }
    add_mlp(f, *d.coarse);
    if (d.fine) add_mlp(f, *d.fine);
    f.add_folded(*d.coarse);
    if (d.fine) f.add_folded(*d.fine);
    return f;
}

// the trunk-only / bender-only kernels of the split-bender path: the trunk is the architecture's without bender (the 5- and
// the 7-layer bender share architecture 0's), the bender kernel is compiled per bender shape (narrow trunk: the 5-layer one)
int trunk_arch(int arch_id) { return arch_id == 5 ? 5 : 0; }
int bender_arch(int arch_id) { return arch_id == 5 ? 0 : arch_id; }

// The images of a model description, and what else the description makes of a handle (`t`).  Every eligibility decision and every
// metadata formula of a handle lives here; no HIP call.  `lay` (create): the packers record where every element comes from in the flat
// parameter vector (nrnerf_model_update_device); null for a refresh.  "No fine network" yields no IMG_FINE / IMG_GEN_FINE (the handle
// resolves them to the coarse images).
int pack_images(const nrnerf_model_desc& d, const FlatLayout* lay, ModelTraits& t, std::vector<Image>& out) {
    t = ModelTraits{};
    out.clear();
    out.reserve(IMG_COUNT);            // (references to entries stay valid)
    auto add = [&](ImageSlot s) -> Image& { out.emplace_back(s); return out.back(); };
    if (d.fine && (d.fine->use_viewdirs != 0) != (d.coarse->use_viewdirs != 0)) return NRNERF_ERR_INVALID;
    t.precision = d.precision;
    t.has_bend = d.bender != nullptr;
    t.views = d.coarse->use_viewdirs != 0;
    t.exact = d.exact_viewdirs != 0 && t.has_bend && t.views;      // only meaningful with bender + view-dependent head
    t.needs_latents = t.has_bend || d.coarse->time_conditioned;
    t.fine_is_coarse = !d.fine;
    const nrnerf_mlp_desc& fm = d.fine ? *d.fine : *d.coarse;       // the network of the fine pass
    nrnerf_model_desc d2 = d;                                       // the model without its bender
    d2.bender = nullptr;
    const bool f32 = d.precision == NRNERF_PREC_F32;

    int arch_f = 0;
    int rc = pack_dispatch(d, *d.coarse, add(IMG_COARSE).pk, &t.arch_id, false, lay);
    if (rc == NRNERF_OK && d.fine) {
        rc = pack_dispatch(d, *d.fine, add(IMG_FINE).pk, &arch_f, false, lay);
        if (rc == NRNERF_OK && arch_f != t.arch_id) rc = NRNERF_ERR_UNSUPPORTED;      // e.g. --netwidth_fine != --netwidth: generic below
    }
    // NRNERF_MODEL_FORCE_GENERIC: the generic kernel also for the compiled shapes (tests: the two routes against each other)
    const bool force_generic = (d.flags & NRNERF_MODEL_FORCE_GENERIC) != 0;
    if (rc == NRNERF_OK && force_generic && !(d.exact_viewdirs && d.bender && d.coarse->use_viewdirs)) rc = NRNERF_ERR_UNSUPPORTED;
    if (rc != NRNERF_OK && rc != NRNERF_ERR_UNSUPPORTED) return rc;
    t.generic = rc == NRNERF_ERR_UNSUPPORTED;

    int cb = -1;                      // compiled shape of the bender (0: 5 x 64, 1: 7 x 64) when a stand-alone bender image exists
    double bend_algo = 0;             // algorithmic flops per sample of the bender alone
    if (!t.generic) {
        // ---- compiled architecture: the fused passes ...
        if (t.exact && t.arch_id > 1) return NRNERF_ERR_UNSUPPORTED;
        t.latent_size = d.bender ? d.bender->latent_size : 0;
        for (Image& im : out) {
            const nrnerf_mlp_desc& mlp = im.slot == IMG_COARSE ? *d.coarse : *d.fine;
            im.algo_flops = 2.0 * algo_macs(d, mlp);
            im.mfma_flops = mfma32_flops_per_sample(im.pk, d.precision);
            im.output_ch = mlp.output_ch;
        }
        // ... the split-bender path's (exact view directions need the bender's Jacobian: fused only; an architecture without a trunk-only
        // plan simply has no split path) ...
        Image ft(IMG_FINE_TRUNK), bo(IMG_BEND_ONLY), ct(IMG_COARSE_TRUNK);
        if (t.has_bend && !t.exact && pack_split(d, ft.pk, bo.pk, &ct.pk, lay) == NRNERF_OK) {
            t.split_ok = true;
            cb = bender_arch(t.arch_id);
            ft.algo_flops = 2.0 * algo_macs(d2, fm);
            ft.output_ch = fm.output_ch;
            ct.algo_flops = 2.0 * algo_macs(d2, *d.coarse);
            ct.output_ch = d.coarse->output_ch;
            bend_algo = bo.algo_flops = 2.0 * algo_macs(d, fm) - ft.algo_flops;
            for (Image* im : {&ft, &bo, &ct}) im->mfma_flops = mfma32_flops_per_sample(im->pk, d.precision);
            // ... with the trunks once more for the 16x16x32 kernel (the coarse network's: the coarse pass of the split path on it too)
            for (const nrnerf_mlp_desc* mlp : {&fm, d.fine ? d.coarse : nullptr}) {
                if (!mlp || !x16_eligible(d, *mlp)) continue;
                Image& x = add(mlp == &fm ? IMG_FINE_TRUNK_X16 : IMG_COARSE_TRUNK_X16);
                pack_x16(d, *mlp, x.pk, lay);
                x.algo_flops = 2.0 * algo_macs(d2, *mlp);
                x.mfma_flops = mfma16_flops_per_sample(x.pk);
                x.output_ch = mlp->output_ch;
            }
            out.push_back(std::move(ft)); out.push_back(std::move(bo)); out.push_back(std::move(ct));
        }
        // ... and the training kernels' (nrnerf_train.h): transposed trunk weights, and -- view-dependent head / time-conditioned baseline --
        // bender-less forward images with both branches of the head / without the latent columns
        if (training_eligible(d, t.arch_id)) {
            t.train_ok = true;
            t.bend_train_ok = t.has_bend;
            if (t.has_bend) cb = bender_arch(t.arch_id);
            auto pack_train = [&](const nrnerf_mlp_desc& mlp, PackedPass& pk) {
                const int ts = tcb_shift_of(mlp);
                if (mlp.use_viewdirs) {             // trunk + both branches of the view-dependent head (trunk_fwd_train<.., VIEWS>)
                    if (f32) pack_pass<ShapeF32, ArchDefault, false, true>(d2, mlp, d.precision, pk, lay, ts);
                    else pack_pass<Shape16Fast, ArchDefault, false, true>(d2, mlp, d.precision, pk, lay, ts);
                } else if (f32) pack_pass<ShapeF32, ArchDefault, false, false>(d2, mlp, d.precision, pk, lay, ts);
                else pack_pass<Shape16Fast, ArchDefault, false, false>(d2, mlp, d.precision, pk, lay, ts);
            };
            for (const nrnerf_mlp_desc* mlp : {d.coarse, d.fine}) {
                if (!mlp) continue;
                Image& bw = add(mlp == d.coarse ? IMG_COARSE_BWD : IMG_FINE_BWD);
                pack_bwd(d, *mlp, bw.pk, lay);
                bw.mfma_flops = mfma32_flops_per_sample(bw.pk, d.precision);
                if (t.views || d.coarse->time_conditioned) pack_train(*mlp, add(mlp == d.coarse ? IMG_COARSE_TRAIN : IMG_FINE_TRAIN).pk);
            }
        }
    } else {
        // ---- architecture outside the compiled set (nrnerf_generic.h): layer programs ...
        out.clear();
        t.arch_id = -1;
        GenProgram gb, gc, gf;
        rc = gen_pack_all(d, lay, gb, gc, gf);
        if (rc != NRNERF_OK) return rc;
        t.latent_size = d.bender ? d.bender->latent_size : gc.proto.lat;
        auto program = [&](ImageSlot s, GenProgram& g, const nrnerf_mlp_desc* mlp) -> Image& {
            Image& im = add(s);
            im.pk = std::move(g.pk);
            im.proto = g.proto;
            if (mlp) {
                im.algo_flops = 2.0 * algo_macs(d2, *mlp);
                im.mfma_flops = gen_mfma_flops_per_sample(g.proto, f32);
                im.output_ch = mlp->output_ch;
            }
            return im;
        };
        if (d.bender) {
            bend_algo = program(IMG_GEN_BEND, gb, nullptr).algo_flops = 2.0 * (algo_macs(d, *d.coarse) - algo_macs(d2, *d.coarse));
            // the usual case -- an odd TRUNK with the reference's hard-coded bender (rnh:406-407): its compiled stand-alone kernel ...
            cb = t.gen_compiled_bender = bender_matches<ArchDefault>(*d.bender) ? 0 : (bender_matches<ArchDeepBend>(*d.bender) ? 1 : -1);
            if (cb >= 0) {
                Image& bo = add(IMG_BEND_ONLY);            // (mfma_flops stay 0: the profile records of a generic handle)
                auto go = [&](auto sh) {
                    using SH = decltype(sh);
                    if (cb == 0) pack_pass<SH, ArchDefault, true, false, false>(d, *d.coarse, d.precision, bo.pk, lay);
                    else pack_pass<SH, ArchDeepBend, true, false, false>(d, *d.coarse, d.precision, bo.pk, lay);
                };
                if (f32) go(ShapeF32{});
                else if (d.precision == NRNERF_PREC_BF16) go(Shape16Fast{});
                else go(Shape16{});
                bo.algo_flops = bend_algo;
                // ... and its training kernels (forward with saved activations, backward, divergence chains)
                t.bend_train_ok = d.precision != NRNERF_PREC_F16;
            }
        }
        program(IMG_GEN_COARSE, gc, d.coarse);
        if (d.fine) program(IMG_GEN_FINE, gf, d.fine);
        // ... their backward-data programs (training) ...
        if (gen_trainable(d, *d.coarse) && (!d.fine || gen_trainable(d, *d.fine))) {
            t.gen_train_ok = true;
            for (const nrnerf_mlp_desc* mlp : {d.coarse, d.fine}) {
                GenTrainNet& tn = t.gen_tn[mlp == d.coarse ? 0 : 1];
                if (!mlp) { tn = t.gen_tn[0]; continue; }
                GenProgram bw;
                gen_pack_mlp_bwd(d, *mlp, bw, lay);
                program(mlp == d.coarse ? IMG_GEN_COARSE_BWD : IMG_GEN_FINE_BWD, bw, nullptr);
                tn.W = mlp->width; tn.D = mlp->depth; tn.skip = gen_skip(*mlp) >= 0; tn.views = mlp->use_viewdirs != 0;
                tn.dv = tn.views ? 3 + 6 * d.multires_views : 0; tn.draw_col = gen_draw_col(*mlp);
                tn.in_w = mlp->time_conditioned ? mlp->pts_linears[0].in_features : 3 + 6 * d.multires; tn.lat = tn.in_w - (3 + 6 * d.multires);
            }
        }
        if (t.exact && !(t.bend_train_ok && t.gen_train_ok)) return NRNERF_ERR_UNSUPPORTED;      // (needs bend_div_fwd and the per-sample-direction instantiation)
        // ... and the trunks also for the width-class x16 kernel: rendering passes that run on ready-made points (a bender in front), and the
        // training forward of any such trunk (its points are always handed in); with their backward-data programs
        // (training: nrnerf_generic_trunk_backward on gx16_bwd_kernel)
        if (gx16_eligible(d, *d.coarse) && (!d.fine || gx16_eligible(d, *d.fine))) {
            const bool trainable = t.gen_train_ok && gx16_trainable(d, *d.coarse) && (!d.fine || gx16_trainable(d, *d.fine));
            for (const nrnerf_mlp_desc* mlp : {d.coarse, d.fine}) {
                if (!mlp) continue;
                Image& gx = add(mlp == d.coarse ? IMG_GX_COARSE : IMG_GX_FINE);
                pack_gx16(d, *mlp, gx.pk, gx.gx, lay);
                gx.algo_flops = 2.0 * algo_macs(d2, *mlp);
                gx.mfma_flops = mfma16_flops_per_sample(gx.pk);
                gx.output_ch = mlp->output_ch;
                if (!trainable) continue;
                Image& gxb = add(mlp == d.coarse ? IMG_GX_COARSE_BWD : IMG_GX_FINE_BWD);
                pack_gx16_bwd(d, *mlp, gxb.pk, gxb.gx, lay);
            }
        }
    }
    // ---- either way, around a bender of a compiled shape: its training images (fp32 whatever the model's precision) and -- where the
    //      stand-alone bender runs ("bf16" mode) -- its 16x16x32 image
    if (t.bend_train_ok) {
        Image& fwd = add(IMG_BEND_TRAIN_FWD);
        Image& bwd = add(IMG_BEND_TRAIN_BWD);
        gen_pack_bender_train(d, cb, fwd.pk, bwd.pk, lay);
    }
    if ((t.split_ok || t.gen_compiled_bender >= 0) && bend_x16_eligible(d)) {
        Image& bx = add(IMG_BEND_X16);
        pack_bend_x16(d, bx.pk, lay);
        bx.algo_flops = bend_algo;
        bx.mfma_flops = mfma16_flops_per_sample(bx.pk);
    }
    return NRNERF_OK;
}

int pack_host_image(const nrnerf_model_desc* desc, int which, PackedPass& pk) {
    const nrnerf_mlp_desc* m = (which == 1 && desc->fine) ? desc->fine : desc->coarse;
    int rc;
    if (which == 2 || which == 3) {
        if (!desc->bender || (desc->coarse->use_viewdirs && desc->exact_viewdirs)) return NRNERF_ERR_UNSUPPORTED;
        PackedPass other;
        rc = (which == 2) ? pack_split(*desc, pk, other) : pack_split(*desc, other, pk);
    } else if (which == 4 || which == 5) {       // transposed trunk weights of the backward-data kernel (training)
        if (desc->coarse->time_conditioned || desc->precision == NRNERF_PREC_F16) return NRNERF_ERR_UNSUPPORTED;
        PackedPass fwd;
        nrnerf_model_desc d2 = *desc;
        d2.bender = nullptr;
        const nrnerf_mlp_desc* mm = (which == 5 && desc->fine) ? desc->fine : desc->coarse;
        int arch_id = 0;
        rc = pack_dispatch(d2, *mm, fwd, &arch_id);   // validates the architecture
        if (rc == NRNERF_OK && arch_id != 0 && arch_id != 5) rc = NRNERF_ERR_UNSUPPORTED;      // training kernels: trunks of width 256 / 128
        if (rc == NRNERF_OK) pack_bwd(*desc, *mm, pk);
    } else if (which == 6) {                     // transposed bender / rigidity weights of its backward-data kernel (fp32)
        if (!desc->bender) return NRNERF_ERR_UNSUPPORTED;
        PackedPass fwd;
        int arch_id = 0;
        rc = pack_dispatch(*desc, *desc->coarse, fwd, &arch_id);
        if (rc == NRNERF_OK && arch_id > 1 && arch_id != 5) rc = NRNERF_ERR_UNSUPPORTED;
        if (rc == NRNERF_OK) {
            if (bender_arch(arch_id) == 0) pack_pass_bwd_bender<ArchDefault>(*desc->bender, pk);
            else pack_pass_bwd_bender<ArchDeepBend>(*desc->bender, pk);
        }
    } else if (which == 11 || which == 12) {     // the coarse / fine trunk packed for the width-class kernel (nrnerf_gx16.h)
        const nrnerf_mlp_desc* mm = (which == 12 && desc->fine) ? desc->fine : desc->coarse;
        if (!gx16_eligible(*desc, *mm)) return NRNERF_ERR_UNSUPPORTED;
        GxMeta gm;
        rc = NRNERF_OK;
        pack_gx16(*desc, *mm, pk, gm);
    } else if (which == 10) {                    // the fine network's trunk packed for the 16x16x32 kernel (nrnerf_net_x16.h)
        const nrnerf_mlp_desc* mm = desc->fine ? desc->fine : desc->coarse;
        if (!x16_eligible(*desc, *mm, /*any_16bit=*/true)) return NRNERF_ERR_UNSUPPORTED;
        rc = NRNERF_OK;
        pack_x16(*desc, *mm, pk);
    } else if (which == 15) {                    // the resident-slice table of image 10 (ResX16, nrnerf_plan.h): no image, the table as the unit table
        const nrnerf_mlp_desc* mm = desc->fine ? desc->fine : desc->coarse;
        if (!x16_eligible(*desc, *mm, /*any_16bit=*/true) || mm->use_viewdirs || mm->width != 256) return NRNERF_ERR_UNSUPPORTED;
        rc = NRNERF_OK;
        auto table = [&](auto rs) {
            using RS = decltype(rs);
            pk = PackedPass{};
            pk.frag_bytes = Shape16::FRAG_BYTES; pk.slot_bytes = Shape16::UNIT_BYTES;
            pk.unit_off.assign(1, (uint32_t)RS::NRES);
            for (int r = 0; r < RS::NRES; ++r) pk.unit_off.push_back((uint32_t)RS::T.res_src[r]);
            pk.unit_off.push_back((uint32_t)RS::NUNITS);
            pk.unit_off.push_back((uint32_t)Shape16::UNIT_FRAGS);
            for (int u = 0; u < RS::NUNITS; ++u) pk.unit_off.push_back((uint32_t)(RS::unit_src_bytes(u) / 16));
            pk.nunits = (int)pk.unit_off.size() - 1;
        };
        if (desc->precision == NRNERF_PREC_F16) table(ResX16<Shape16, ArchDefault>{});      // (the two 16-bit modes share the plan: one table)
        else table(ResX16<Shape16Fast, ArchDefault>{});
    } else if (which == 13 || which == 14) {    // backward-data programs of the run-time-parameterised kernel (training): 13 = coarse, 14 = fine
        GenProgram gb, gc, gf;
        rc = gen_pack_all(*desc, nullptr, gb, gc, gf);
        const nrnerf_mlp_desc* mm = (which == 14) ? desc->fine : desc->coarse;
        if (rc == NRNERF_OK && !mm) rc = NRNERF_ERR_INVALID;
        if (rc == NRNERF_OK && !gen_trainable(*desc, *mm)) rc = NRNERF_ERR_UNSUPPORTED;
        if (rc == NRNERF_OK) {
            GenProgram g;
            gen_pack_mlp_bwd(*desc, *mm, g, nullptr);
            pk = g.pk;
            program_unit_table(pk, g.proto, 15, {g.proto.ke, g.proto.kv, g.proto.kh, g.proto.lat, gen_draw_col(*mm)});
        }
    } else if (which >= 7 && which <= 9) {      // layer programs of the run-time-parameterised kernel: 7 = coarse, 8 = fine, 9 = ray bender
        GenProgram gb, gc, gf;
        rc = gen_pack_all(*desc, nullptr, gb, gc, gf);
        if (rc == NRNERF_OK && ((which == 8 && !desc->fine) || (which == 9 && !desc->bender))) rc = NRNERF_ERR_INVALID;
        if (rc == NRNERF_OK) {
            GenProgram& g = which == 7 ? gc : (which == 8 ? gf : gb);
            pk = g.pk;
            program_unit_table(pk, g.proto, 11, {g.proto.ke, g.proto.kv, g.proto.kh, g.proto.lat});
        }
    } else {
        rc = pack_dispatch(*desc, *m, pk);
    }
    return rc;
}

}  // namespace nrn
