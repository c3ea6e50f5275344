"""Status codes of the training and auxiliary entry points of the C ABI (include/nrnerf.h): a literal table of
(entry point, case) -> status.  It pins the order of the argument checks, which of two failing checks wins, and whether a zero-size call
answers before or after the pointer checks -- what nothing else in the suite looks at.

CPU part: cases the library decides before its first HIP call (the owner lookup of a pointer included), so the answer is the same on a box
without a GPU; non-null pointers are addresses of a small host buffer, a non-null model is such an address too (never dereferenced: the
struct_size check sits in front).  GPU part: four small handles, 3 rays, 5 + 3 samples; every case is a rejection or a zero-size OK, and
every non-null device pointer is a real allocation large enough for the shape the call states.

Not in the table, checked by reading: the 32-bit-offset rejections of nrnerf_bender_wgrad / nrnerf_bender_divergence_backward (bf16,
16.7 M samples and up) -- the arrays of that shape are not something a test allocates."""
import ctypes as C

import pytest
import torch

from nonrigid_nerf_amd import _lib

OK, INVALID, UNSUPPORTED, WORKSPACE = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
N, S, I = 3, 5, 3                 # ragged against the 16- and 32-sample blocks
STREAM = C.c_void_p(0)

_HOST = (C.c_char * 4096)()       # what a non-null pointer of a CPU case points at (64-byte aligned below)
H = (C.addressof(_HOST) + 63) & ~63


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)
    return obj


def _make(cls, p, **kw):
    """An argument record whose every pointer field is ``p(name)`` and whose struct_size is right, then ``kw`` on top."""
    a = cls()
    for name, typ in cls._fields_:
        if typ is C.c_void_p:
            setattr(a, name, p(name))
    if hasattr(a, "struct_size"):
        a.struct_size = C.sizeof(cls)
    return _set(a, **kw)


def _host(_name):
    return H


# ---- valid-looking records (host pointers): each CPU case changes one or two fields --------------------------------------------------
def trunk_args(p=_host, **kw):
    return _make(_lib.TrunkArgs, p, **{**dict(which=0, n_rays=N, n_samples=S, raw_ch=4), **kw})


def generic_args(p=_host, **kw):
    return _make(_lib.GenericTrunkArgs, p, **{**dict(which=0, n_rays=N, n_samples=S, raw_ch=4), **kw})


def wgrad_args(p=_host, **kw):
    return _make(_lib.WgradArgs, p, **{**dict(n_rays=N, n_samples=S, n_partials=1), **kw})


def bender_args(p=_host, **kw):
    return _make(_lib.BenderArgs, p, **{**dict(n_rays=N, n_samples=S, ray_stride=11, latent_stride=32), **kw})


def bender_wgrad_args(p=_host, **kw):
    return _make(_lib.BenderWgradArgs, p, **{**dict(n_rays=N, n_samples=S, ray_stride=11, latent_stride=32, n_partials=4), **kw})


def divergence_args(p=_host, **kw):
    return _make(_lib.DivergenceArgs, p, **{**dict(n_points=N * S, latent_stride=32, n_partials=4), **kw})


def loss_args(p=_host, **kw):
    return _make(_lib.LossArgs, p, **{**dict(n_rays=N, n_samples=S), **kw})


def encoding_args(p=_host, **kw):
    return _make(_lib.EncodingArgs, p, **{**dict(n_rows=N * S, n_freqs=4, src_stride=4, enc_cols=27), **kw})


def composite_args(p=_host, **kw):
    return _make(_lib.CompositeArgs, p, **{**dict(n_rays=N, n_samples=S, n_importance=I, ray_stride=8), **kw})


def adam_args(p=_host, **kw):
    a = _make(_lib.AdamArgs, p, **{**dict(n_segments=0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8), **kw})
    return a


def adam_with_segment(**seg):
    a = adam_args(n_segments=1)
    _set(a.segments[0], **{**dict(param=H, grad=H, exp_avg=H, exp_avg_sq=H, n=4), **seg})
    return a


def tn_args(p=_host, **kw):
    return _make(_lib.TnArgs, p, **{**dict(n_jobs=1, n_rows=8, out_floats=16, workspace_bytes=64), **kw})


def camera(**kw):
    return _set(_lib.Camera(), **{**dict(focal_x=50.0, focal_y=50.0, center_x=2.0, center_y=2.0, height=4, width=4), **kw})


def call(lib, name, *args):
    return getattr(lib, name)(*[C.byref(a) if isinstance(a, C.Structure) else a for a in args])


MODEL = H          # a non-null model of a CPU case: only ever compared with NULL

# entry point -> how to build (args with the record built by `make(**kw)`)
MODEL_CALLS = {
    "nrnerf_generic_trunk_forward": generic_args, "nrnerf_generic_trunk_backward": generic_args,
    "nrnerf_trunk_forward": trunk_args, "nrnerf_trunk_backward": trunk_args, "nrnerf_trunk_wgrad": wgrad_args,
    "nrnerf_bender_forward": bender_args, "nrnerf_bender_backward": bender_args, "nrnerf_bender_wgrad": bender_wgrad_args,
    "nrnerf_bender_divergence_forward": divergence_args, "nrnerf_bender_divergence_backward": divergence_args,
}


def _cpu_cases():
    """(id, thunk(lib) -> status, expected)"""
    cases = []

    def add(name, case, expected, fn):
        cases.append((f"{name}:{case}", fn, expected))

    # ---- every model-taking entry point: a NULL model, NULL arguments, a wrong struct_size
    for name, make in MODEL_CALLS.items():
        add(name, "null_model", INVALID, lambda lib, name=name, make=make: call(lib, name, None, make(), STREAM))
        add(name, "null_args", INVALID, lambda lib, name=name: getattr(lib, name)(MODEL, None, STREAM))
        add(name, "struct_size", INVALID, lambda lib, name=name, make=make: call(lib, name, MODEL, make(struct_size=4), STREAM))
    add("nrnerf_model_trains_generic", "null_model", INVALID, lambda lib: lib.nrnerf_model_trains_generic(None))
    add("nrnerf_model_trains_bender", "null_model", INVALID, lambda lib: lib.nrnerf_model_trains_bender(None))
    add("nrnerf_generic_trunk_bits_bytes", "null_model", 0, lambda lib: lib.nrnerf_generic_trunk_bits_bytes(None, 0, N, S))

    # ---- nrnerf_adam_step (works without a model: then the caller brings the barrier words)
    def adam(case, expected, a):
        add("nrnerf_adam_step", case, expected, lambda lib, a=a: getattr(lib, "nrnerf_adam_step")(None, C.byref(a) if a is not None else None, STREAM))
    adam("null_args", INVALID, None)
    adam("struct_size", INVALID, adam_args(struct_size=8))
    adam("n_segments_negative", INVALID, adam_args(n_segments=-1))
    adam("n_segments_41", INVALID, adam_args(n_segments=_lib.ADAM_MAX_SEGMENTS + 1))
    adam("null_step", INVALID, adam_args(step=None))
    adam("beta1_one", INVALID, adam_args(beta1=1.0))
    adam("beta1_negative", INVALID, adam_args(beta1=-0.1))
    adam("beta2_one", INVALID, adam_args(beta2=1.0))
    adam("beta2_nan", INVALID, adam_args(beta2=float("nan")))
    adam("eps_negative", INVALID, adam_args(eps=-1e-8))
    adam("no_model_no_barrier", INVALID, adam_args(barrier=None))
    adam("segment_null_param", INVALID, adam_with_segment(param=None))
    adam("segment_null_exp_avg_sq", INVALID, adam_with_segment(exp_avg_sq=None))

    # ---- nrnerf_tn_products
    def one(name, case, expected, a):
        add(name, case, expected, lambda lib, a=a: getattr(lib, name)(C.byref(a) if a is not None else None, STREAM))
    one("nrnerf_tn_products", "null_args", INVALID, None)
    one("nrnerf_tn_products", "struct_size", INVALID, tn_args(struct_size=8))
    one("nrnerf_tn_products", "null_out", INVALID, tn_args(out=None))
    one("nrnerf_tn_products", "null_workspace", INVALID, tn_args(workspace=None))

    # ---- nrnerf_encoding_forward / _backward
    for name in ("nrnerf_encoding_forward", "nrnerf_encoding_backward"):
        one(name, "null_args", INVALID, None)
        one(name, "struct_size", INVALID, encoding_args(struct_size=8))
        one(name, "n_rows_negative", INVALID, encoding_args(n_rows=-1))
        one(name, "null_src", INVALID, encoding_args(src=None))
        one(name, "n_rows_zero", OK, encoding_args(n_rows=0))
        one(name, "n_rows_zero_null_src", INVALID, encoding_args(n_rows=0, src=None))

    # ---- nrnerf_loss_forward / _backward: the pointer and stride rules of loss_call
    for name, bwd in (("nrnerf_loss_forward", False), ("nrnerf_loss_backward", True)):
        one(name, "null_args", INVALID, None)
        one(name, "struct_size", INVALID, loss_args(struct_size=8))
        one(name, "n_rays_negative", INVALID, loss_args(n_rays=-1))
        one(name, "n_samples_negative", INVALID, loss_args(n_samples=-1))
        one(name, "null_rgb_map", INVALID, loss_args(rgb_map=None))
        one(name, "null_target", INVALID, loss_args(target=None))
        one(name, "weights_without_offsets", INVALID, loss_args(offsets=None))
        one(name, "weights_without_rigidity", INVALID, loss_args(rigidity=None))
        one(name, "divergence_without_alpha", INVALID, loss_args(alpha=None))
        one(name, "regularisers_without_samples", INVALID, loss_args(n_samples=0))
        one(name, "offsets_stride_negative", INVALID, loss_args(offsets_stride=-1))
        one(name, "rigidity_stride_negative", INVALID, loss_args(rigidity_stride=-1))
        one(name, "offsets_stride_2", INVALID, loss_args(offsets_stride=2))
        one(name, "n_rays_zero", OK, loss_args(n_rays=0))
        one(name, "n_rays_zero_strides_3_1", OK, loss_args(n_rays=0, offsets_stride=3, rigidity_stride=1))
        one(name, "n_rays_zero_null_target", INVALID, loss_args(n_rays=0, target=None))
    one("nrnerf_loss_forward", "null_loss", INVALID, loss_args(loss=None))
    one("nrnerf_loss_backward", "null_loss_n_rays_zero", OK, loss_args(loss=None, n_rays=0))
    one("nrnerf_loss_backward", "no_g_loss_no_g_mean", INVALID, loss_args(g_loss=None, g_mean=None))
    one("nrnerf_loss_backward", "g_mean_alone_n_rays_zero", OK, loss_args(g_loss=None, n_rays=0))
    one("nrnerf_loss_backward", "null_g_rgb_map", INVALID, loss_args(g_rgb_map=None))
    one("nrnerf_loss_backward", "rgb0_without_g_rgb0", INVALID, loss_args(g_rgb0=None))
    one("nrnerf_loss_backward", "weights_without_g_offsets", INVALID, loss_args(g_offsets=None))
    one("nrnerf_loss_backward", "weights_without_g_rigidity", INVALID, loss_args(g_rigidity=None))
    one("nrnerf_loss_backward", "divergence_without_g_divergence", INVALID, loss_args(g_divergence=None))
    one("nrnerf_loss_forward", "backward_only_fields_missing_n_rays_zero", OK, loss_args(n_rays=0, g_loss=None, g_mean=None, g_rgb_map=None))

    # ---- the small kernels: positional arguments
    def pos(name, case, expected, *args):
        add(name, case, expected, lambda lib, args=args: getattr(lib, name)(*args, STREAM))
    cg = lambda **kw: tuple({**dict(index=H, g=H, n_rays=N, latent_size=32, n_codes=2, out=H), **kw}.values())
    pos("nrnerf_code_gradients", "null_index", INVALID, *cg(index=None))
    pos("nrnerf_code_gradients", "null_g", INVALID, *cg(g=None))
    pos("nrnerf_code_gradients", "null_out", INVALID, *cg(out=None))
    pos("nrnerf_code_gradients", "n_rays_negative", INVALID, *cg(n_rays=-1))
    pos("nrnerf_code_gradients", "latent_size_0", INVALID, *cg(latent_size=0))
    pos("nrnerf_code_gradients", "latent_size_257", INVALID, *cg(latent_size=257))
    pos("nrnerf_code_gradients", "n_codes_negative", INVALID, *cg(n_codes=-1))
    pos("nrnerf_code_gradients", "n_codes_zero", OK, *cg(n_codes=0))
    pos("nrnerf_code_gradients", "n_codes_zero_latent_size_257", INVALID, *cg(n_codes=0, latent_size=257))

    mr = lambda **kw: tuple({**dict(rank_new=H, n_rays=N, n_samples=S, n_importance=I, coarse_a=H, coarse_b=H, new_a=H, new_b=H, merged_a=H,
                                    merged_b=H, inverse=0), **kw}.values())
    pos("nrnerf_merge_rows", "null_rank_new", INVALID, *mr(rank_new=None))
    pos("nrnerf_merge_rows", "null_coarse_a", INVALID, *mr(coarse_a=None))
    pos("nrnerf_merge_rows", "null_new_a", INVALID, *mr(new_a=None))
    pos("nrnerf_merge_rows", "null_merged_a", INVALID, *mr(merged_a=None))
    pos("nrnerf_merge_rows", "n_rays_negative", INVALID, *mr(n_rays=-1))
    pos("nrnerf_merge_rows", "n_samples_0", INVALID, *mr(n_samples=0))
    pos("nrnerf_merge_rows", "n_importance_0", INVALID, *mr(n_importance=0))
    pos("nrnerf_merge_rows", "257_merged_samples", INVALID, *mr(n_samples=129, n_importance=128))
    pos("nrnerf_merge_rows", "coarse_b_without_merged_b", INVALID, *mr(new_b=None, merged_b=None))
    pos("nrnerf_merge_rows", "new_b_without_merged_b", INVALID, *mr(coarse_b=None, merged_b=None))
    pos("nrnerf_merge_rows", "merged_b_alone", INVALID, *mr(coarse_b=None, new_b=None))
    pos("nrnerf_merge_rows", "n_rays_zero", OK, *mr(n_rays=0))
    pos("nrnerf_merge_rows", "n_rays_zero_no_b_arrays", OK, *mr(n_rays=0, coarse_b=None, new_b=None, merged_b=None))
    pos("nrnerf_merge_rows", "n_rays_zero_merged_b_alone", INVALID, *mr(n_rays=0, coarse_b=None, new_b=None))

    rp = lambda **kw: tuple({**dict(partials=H, record_stride=64, n_partials=4, n_short=2, index=H, n_out=8, out=H), **kw}.values())
    for name, tail in (("nrnerf_reduce_partials", ()), ("nrnerf_reduce_partials_aux", (None, 0, None))):
        pos(name, "null_partials", INVALID, *rp(partials=None), *tail)
        pos(name, "null_index", INVALID, *rp(index=None), *tail)
        pos(name, "null_out", INVALID, *rp(out=None), *tail)
        pos(name, "n_out_negative", INVALID, *rp(n_out=-1), *tail)
        pos(name, "n_partials_0", INVALID, *rp(n_partials=0, n_short=0), *tail)
        pos(name, "n_short_negative", INVALID, *rp(n_short=-1), *tail)
        pos(name, "n_short_above_n_partials", INVALID, *rp(n_short=5), *tail)
        pos(name, "record_stride_0", INVALID, *rp(record_stride=0), *tail)
        pos(name, "record_stride_REDUCE_SHORT", INVALID, *rp(record_stride=_lib.REDUCE_SHORT), *tail)
        pos(name, "n_out_zero", OK, *rp(n_out=0), *tail)
        pos(name, "n_out_zero_record_stride_0", INVALID, *rp(n_out=0, record_stride=0), *tail)
    aux_pos = (C.c_int64 * 4)(0, 1, 2, 3)
    pos("nrnerf_reduce_partials_aux", "aux_n_aux_negative", INVALID, *rp(), H, -1, aux_pos)
    pos("nrnerf_reduce_partials_aux", "aux_without_aux_pos", INVALID, *rp(), H, 4, None)
    pos("nrnerf_reduce_partials_aux", "aux_n_out_zero", OK, *rp(n_out=0), H, 4, aux_pos)
    pos("nrnerf_reduce_partials_aux", "aux_without_aux_pos_n_out_zero", INVALID, *rp(n_out=0), H, 4, None)

    pos("nrnerf_tile_row_sums", "null_tiles", INVALID, None, 8, H)
    pos("nrnerf_tile_row_sums", "null_out", INVALID, H, 8, None)
    pos("nrnerf_tile_row_sums", "n_rows_negative", INVALID, H, -1, H)
    pos("nrnerf_tile_row_sums", "n_rows_zero", OK, H, 0, H)

    t2r = lambda **kw: tuple({**dict(tiles=H, n_rays=N, n_samples=S, width=256, rows=H), **kw}.values())
    pos("nrnerf_tiles_to_rows", "null_tiles", INVALID, *t2r(tiles=None))
    pos("nrnerf_tiles_to_rows", "null_rows", INVALID, *t2r(rows=None))
    pos("nrnerf_tiles_to_rows", "n_rays_negative", INVALID, *t2r(n_rays=-1))
    pos("nrnerf_tiles_to_rows", "n_samples_0", INVALID, *t2r(n_samples=0))
    pos("nrnerf_tiles_to_rows", "n_samples_257", INVALID, *t2r(n_samples=257))
    pos("nrnerf_tiles_to_rows", "width_64", INVALID, *t2r(width=64))
    pos("nrnerf_tiles_to_rows", "width_128_n_rays_zero", OK, *t2r(width=128, n_rays=0))
    pos("nrnerf_tiles_to_rows", "n_rays_zero", OK, *t2r(n_rays=0))
    pos("nrnerf_tiles_to_rows", "n_rays_zero_width_64", INVALID, *t2r(n_rays=0, width=64))

    de = lambda **kw: tuple({**dict(bent4=H, n_rays=N, n_samples=S, n_freqs=4, enc=H, enc_is_bf16=0, g_bent4=None), **kw}.values())
    pos("nrnerf_direction_encoding", "null_bent4", INVALID, *de(bent4=None))
    pos("nrnerf_direction_encoding", "null_enc", INVALID, *de(enc=None))
    pos("nrnerf_direction_encoding", "n_rays_negative", INVALID, *de(n_rays=-1))
    pos("nrnerf_direction_encoding", "n_samples_1", INVALID, *de(n_samples=1))
    pos("nrnerf_direction_encoding", "n_samples_1025", INVALID, *de(n_samples=_lib.MAX_SAMPLES + 1))
    pos("nrnerf_direction_encoding", "n_freqs_negative", INVALID, *de(n_freqs=-1))
    pos("nrnerf_direction_encoding", "n_freqs_11", INVALID, *de(n_freqs=11))
    pos("nrnerf_direction_encoding", "n_rays_zero_n_freqs_10", OK, *de(n_rays=0, n_freqs=10))
    pos("nrnerf_direction_encoding", "n_rays_zero_n_freqs_11", INVALID, *de(n_rays=0, n_freqs=11))

    # ---- nrnerf_generate_rays, nrnerf_sample_depths, nrnerf_sample_depths_points
    def rays(case, expected, cam, out, stride):
        add("nrnerf_generate_rays", case, expected,
            lambda lib, cam=cam: lib.nrnerf_generate_rays(C.byref(cam) if cam is not None else None, 2.0, 6.0, out, stride, STREAM))
    rays("null_camera", INVALID, None, H, 8)
    rays("null_rays_out", INVALID, camera(), None, 8)
    rays("ray_stride_9", INVALID, camera(), H, 9)
    rays("ray_stride_10", INVALID, camera(), H, 10)
    rays("height_0", INVALID, camera(height=0), H, 11)
    rays("width_0", INVALID, camera(width=0), H, 8)
    rays("focal_x_0", INVALID, camera(focal_x=0.0), H, 8)
    rays("focal_y_0", INVALID, camera(focal_y=0.0), H, 8)
    sd = lambda **kw: tuple({**dict(rays=H, ray_stride=8, uniforms=None, n_rays=N, n_samples=S, lindisp=0, z_out=H), **kw}.values())
    for name, tail in (("nrnerf_sample_depths", ()), ("nrnerf_sample_depths_points", (H,))):
        pos(name, "null_rays", INVALID, *sd(rays=None), *tail)
        pos(name, "null_z_out", INVALID, *sd(z_out=None), *tail)
        pos(name, "ray_stride_7", INVALID, *sd(ray_stride=7), *tail)
        pos(name, "n_rays_negative", INVALID, *sd(n_rays=-1), *tail)
        pos(name, "n_samples_1", INVALID, *sd(n_samples=1), *tail)
        pos(name, "n_samples_1025", INVALID, *sd(n_samples=_lib.MAX_SAMPLES + 1), *tail)
        pos(name, "n_rays_zero", OK, *sd(n_rays=0), *tail)
        pos(name, "n_rays_zero_n_samples_1", INVALID, *sd(n_rays=0, n_samples=1), *tail)
    pos("nrnerf_sample_depths_points", "null_points_out", INVALID, *sd(), None)
    pos("nrnerf_sample_depths_points", "null_points_out_n_rays_zero", INVALID, *sd(n_rays=0), None)

    # ---- the two composite calls: the same sample limit answers differently, and the zero-size OK comes before the pointer checks
    fwd, bwd = "nrnerf_composite_forward", "nrnerf_composite_backward"
    for name in (fwd, bwd):
        one(name, "null_args", INVALID, None)
        one(name, "struct_size", INVALID, composite_args(struct_size=8))
        one(name, "n_rays_negative", INVALID, composite_args(n_rays=-1))
        one(name, "n_samples_1", INVALID, composite_args(n_samples=1))
        one(name, "n_rays_zero", OK, composite_args(n_rays=0))
        one(name, "n_rays_zero_null_pointers", OK, _set(_make(_lib.CompositeArgs, lambda n: None), n_rays=0, n_samples=S))      # the order decides
        one(name, "null_rays", INVALID, composite_args(rays=None))
        one(name, "ray_stride_7", INVALID, composite_args(ray_stride=7))
        one(name, "null_raw4", INVALID, composite_args(raw4=None))
    one(fwd, "n_importance_negative", INVALID, composite_args(n_importance=-1))
    one(fwd, "n_samples_1025", UNSUPPORTED, composite_args(n_samples=_lib.MAX_SAMPLES + 1, n_importance=0))
    one(fwd, "1025_merged_samples", UNSUPPORTED, composite_args(n_samples=1000, n_importance=25))
    one(fwd, "rank_new_257_merged_samples", UNSUPPORTED, composite_args(n_samples=200, n_importance=57))
    one(fwd, "257_merged_samples_without_rank_new_n_rays_zero", OK, composite_args(n_samples=200, n_importance=57, z_new=None, rank_new=None, n_rays=0))
    one(fwd, "null_rgb", INVALID, composite_args(rgb=None))
    one(fwd, "null_disp", INVALID, composite_args(disp=None))
    one(fwd, "null_acc", INVALID, composite_args(acc=None))
    one(fwd, "importance_without_z_merged", INVALID, composite_args(z_merged=None))
    one(fwd, "z_new_without_rank_new", INVALID, composite_args(rank_new=None))
    one(fwd, "rank_new_without_z_new", INVALID, composite_args(z_new=None))
    # two checks fail at once
    one(fwd, "n_samples_1025_and_n_rays_negative", INVALID, composite_args(n_samples=_lib.MAX_SAMPLES + 1, n_rays=-1))
    one(fwd, "n_samples_1025_and_n_rays_zero", UNSUPPORTED, composite_args(n_samples=_lib.MAX_SAMPLES + 1, n_rays=0))
    one(fwd, "n_samples_1025_and_null_rays", UNSUPPORTED, composite_args(n_samples=_lib.MAX_SAMPLES + 1, rays=None))
    one(fwd, "rank_new_257_merged_samples_and_n_rays_zero", UNSUPPORTED, composite_args(n_samples=200, n_importance=57, n_rays=0))
    one(fwd, "rank_new_257_merged_samples_and_null_rgb", UNSUPPORTED, composite_args(n_samples=200, n_importance=57, rgb=None))
    one(fwd, "n_rays_zero_and_ray_stride_7", OK, composite_args(n_rays=0, ray_stride=7))
    one(fwd, "null_rays_and_rank_new_without_z_new", INVALID, composite_args(rays=None, z_new=None))
    one(bwd, "n_samples_1025", INVALID, composite_args(n_samples=_lib.MAX_SAMPLES + 1))
    one(bwd, "null_g_rgb", INVALID, composite_args(g_rgb=None))
    one(bwd, "null_d_raw4", INVALID, composite_args(d_raw4=None))
    one(bwd, "n_samples_1025_and_n_rays_zero", INVALID, composite_args(n_samples=_lib.MAX_SAMPLES + 1, n_rays=0))
    one(bwd, "n_rays_zero_and_null_g_rgb", OK, composite_args(n_rays=0, g_rgb=None))
    one(bwd, "n_importance_negative_is_not_looked_at_n_rays_zero", OK, composite_args(n_importance=-1, n_rays=0))
    return cases


CPU_CASES = _cpu_cases()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("thunk,expected", [pytest.param(fn, exp, id=cid) for cid, fn, exp in CPU_CASES])
def test_status_before_any_hip_call(lib, thunk, expected):
    assert thunk(lib) == expected


def test_cpu_table_is_complete():
    """every entry point this table is about has cases, and the ids are unique"""
    names = {cid.split(":")[0] for cid, _, _ in CPU_CASES}
    want = set(MODEL_CALLS) | {"nrnerf_adam_step", "nrnerf_tn_products", "nrnerf_encoding_forward", "nrnerf_encoding_backward", "nrnerf_loss_forward",
                               "nrnerf_loss_backward", "nrnerf_code_gradients", "nrnerf_merge_rows", "nrnerf_reduce_partials", "nrnerf_reduce_partials_aux",
                               "nrnerf_tile_row_sums", "nrnerf_tiles_to_rows", "nrnerf_direction_encoding", "nrnerf_generate_rays", "nrnerf_sample_depths",
                               "nrnerf_sample_depths_points", "nrnerf_composite_forward", "nrnerf_composite_backward", "nrnerf_model_trains_generic",
                               "nrnerf_generic_trunk_bits_bytes"}
    assert want <= names
    assert len({cid for cid, _, _ in CPU_CASES}) == len(CPU_CASES)


# ---- GPU part ---------------------------------------------------------------------------------------------------------------------------
MIB = 1 << 20


class Device:
    """Real device allocations for the pointer fields of a case; alive until the case has returned."""

    def __init__(self):
        self.keep, self.big = [], False

    def __call__(self, nbytes=MIB):
        t = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
        self.keep.append(t)
        return t.data_ptr()

    def scratch(self, nbytes):          # large and never read unless a check is lost: not cleared
        t = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
        self.keep.append(t)
        self.big = self.big or nbytes > (256 << 20)
        return t.data_ptr()

    def release(self):
        self.keep.clear()
        if self.big:                    # (the 4097-record arrays: back to the driver, not into the caching allocator's pool)
            torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def handles():
    from nonrigid_nerf_amd import render as R
    from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_scene
    dev = torch.device("cuda:0")
    out, keep = {}, []
    for key, cfg, prec in (("f32", SceneConfig(N_samples=S, N_importance=I), "f32"),
                           ("bf16", SceneConfig(N_samples=S, N_importance=I), "bf16"),
                           ("views", SceneConfig(N_samples=S, N_importance=I, use_viewdirs=True), "bf16"),
                           ("generic", SceneConfig(N_samples=S, N_importance=I, netdepth=6, netwidth=192), "f32")):
        _rb, coarse, fine = build_modules(make_scene(cfg, 0), device=dev)
        m = R.Model(coarse, fine, precision=prec, device=dev, flags=0)
        keep.append((coarse, fine, m))
        out[key] = m
    yield out
    for _c, _f, m in keep:
        m.close()


# the arrays of a call at 3 rays and at most 8 samples fit 1 MiB each (the largest: eight layers of bf16 tiles, 3 blocks x 256 x 32 x 2 bytes each);
# the partial sums are sized by the record count the case states
def wgrad_bytes(views, n_partials):
    stride = _lib.wgrad_stride_views(8, 256) if views else _lib.wgrad_stride(8, 256)
    return 4 * stride * max(n_partials, 1)


def bender_wgrad_bytes(n_partials, n_jobs=16):
    return 4 * _lib.BENDER_WGRAD_SLOT * n_jobs * max(n_partials, 1)


def _gpu_cases():
    """(id, handle key or None, thunk(lib, handle, d) -> status, expected); d: Device"""
    cases = []

    def add(cid, key, expected, fn):
        cases.append((cid, key, fn, expected))

    def model_call(name, make, cid, key, expected, partials=None, **kw):
        def fn(lib, h, d):
            a = make(lambda _n: d(), **{k: v for k, v in kw.items()})
            if partials is not None:
                a.partials = d.scratch(partials)
            return getattr(lib, name)(h, C.byref(a), STREAM)
        add(f"{name}:{key}:{cid}", key, expected, fn)

    T, G, W = "nrnerf_trunk_forward", "nrnerf_generic_trunk_forward", "nrnerf_trunk_wgrad"
    TB, GB = "nrnerf_trunk_backward", "nrnerf_generic_trunk_backward"
    # a missing relu mask: bf16 needs it, f32 does not (the f32 call is the zero-size one: it answers OK after the mask rule)
    for name in (T, TB):
        model_call(name, trunk_args, "no_relu_mask", "bf16", INVALID, relu_mask=None)
        model_call(name, trunk_args, "no_relu_mask_n_rays_zero", "bf16", INVALID, relu_mask=None, n_rays=0)
        model_call(name, trunk_args, "no_relu_mask_n_rays_zero", "f32", OK, relu_mask=None, n_rays=0)
        model_call(name, trunk_args, "no_view_arrays_n_rays_zero", "f32", OK, dirs=None, hv=None, hv_mask=None, d_pre_v=None, n_rays=0)
        model_call(name, trunk_args, "no_hv_mask", "views", INVALID, hv_mask=None)
        model_call(name, trunk_args, "no_dirs", "views", INVALID, dirs=None)
        model_call(name, trunk_args, "no_hv", "views", INVALID, hv=None)
        model_call(name, trunk_args, "no_hv_n_rays_zero", "views", INVALID, hv=None, n_rays=0)
        model_call(name, trunk_args, "n_rays_zero", "views", OK, n_rays=0)
        model_call(name, trunk_args, "generic_handle", "generic", UNSUPPORTED)
        model_call(name, trunk_args, "generic_handle_which_2", "generic", UNSUPPORTED, which=2)          # (the order decides)
        model_call(name, trunk_args, "which_2", "f32", INVALID, which=2)
        model_call(name, trunk_args, "which_negative", "bf16", INVALID, which=-1)
        model_call(name, trunk_args, "n_samples_0", "f32", INVALID, n_samples=0)
        model_call(name, trunk_args, "n_samples_1025", "f32", INVALID, n_samples=_lib.MAX_SAMPLES + 1, n_rays=0)
        model_call(name, trunk_args, "n_rays_zero", "f32", OK, n_rays=0)
        model_call(name, trunk_args, "n_rays_zero_fine", "bf16", OK, n_rays=0, which=1, n_samples=S + I)
    model_call(TB, trunk_args, "no_d_pre_v", "views", INVALID, d_pre_v=None)
    model_call(T, trunk_args, "no_d_pre_v_n_rays_zero", "views", OK, d_pre_v=None, n_rays=0)
    model_call(T, trunk_args, "raw_ch_3", "f32", INVALID, raw_ch=3)
    model_call(T, trunk_args, "raw_ch_6", "bf16", INVALID, raw_ch=6)
    model_call(T, trunk_args, "raw_ch_3_without_raw_n_rays_zero", "f32", OK, raw_ch=3, raw=None, n_rays=0)
    model_call(TB, trunk_args, "raw_ch_3_is_not_looked_at_n_rays_zero", "f32", OK, raw_ch=3, n_rays=0)
    model_call(TB, trunk_args, "no_d_pts4", "f32", INVALID, d_pts4=None)

    for name in (G, GB):
        model_call(name, generic_args, "compiled_handle", "f32", UNSUPPORTED)
        model_call(name, generic_args, "compiled_handle", "bf16", UNSUPPORTED)
        model_call(name, generic_args, "compiled_handle_which_2", "views", UNSUPPORTED, which=2)
        model_call(name, generic_args, "which_2", "generic", INVALID, which=2)
        model_call(name, generic_args, "no_acts", "generic", INVALID, acts=None)
        model_call(name, generic_args, "n_rays_zero", "generic", OK, n_rays=0)
        model_call(name, generic_args, "n_rays_zero_fine", "generic", OK, n_rays=0, which=1, n_samples=S + I)
    model_call(G, generic_args, "raw_ch_3", "generic", INVALID, raw_ch=3)
    model_call(G, generic_args, "raw_ch_above_output_ch", "generic", INVALID, raw_ch=9)
    model_call(G, generic_args, "raw_ch_3_without_raw_n_rays_zero", "generic", OK, raw_ch=3, raw=None, n_rays=0)
    model_call(GB, generic_args, "raw_ch_3_is_not_looked_at_n_rays_zero", "generic", OK, raw_ch=3, n_rays=0)
    model_call(G, generic_args, "no_raw4", "generic", INVALID, raw4=None)
    model_call(GB, generic_args, "no_d_enc0", "generic", INVALID, d_enc0=None)

    model_call(W, wgrad_args, "generic_handle", "generic", UNSUPPORTED, partials=wgrad_bytes(False, 1))
    model_call(W, wgrad_args, "n_partials_0", "f32", INVALID, partials=wgrad_bytes(False, 0), n_partials=0)
    model_call(W, wgrad_args, "n_partials_4097", "f32", INVALID, partials=wgrad_bytes(False, 4097), n_partials=4097)
    model_call(W, wgrad_args, "no_g_head", "bf16", INVALID, partials=wgrad_bytes(False, 1), g_head=None)
    model_call(W, wgrad_args, "n_rays_zero", "bf16", OK, partials=wgrad_bytes(False, 1), n_rays=0)
    # the views pointers are looked at only behind the zero-size return
    model_call(W, wgrad_args, "no_dirs", "views", INVALID, partials=wgrad_bytes(True, 1), dirs=None)
    model_call(W, wgrad_args, "no_encv", "views", INVALID, partials=wgrad_bytes(True, 1), encv=None)
    model_call(W, wgrad_args, "no_dirs_n_rays_zero", "views", OK, partials=wgrad_bytes(True, 1), dirs=None, n_rays=0)

    B, BB, BW = "nrnerf_bender_forward", "nrnerf_bender_backward", "nrnerf_bender_wgrad"
    for name in (B, BB):
        model_call(name, bender_args, "latent_stride_31", "f32", INVALID, latent_stride=31)
        model_call(name, bender_args, "latent_stride_31_n_rays_zero", "generic", INVALID, latent_stride=31, n_rays=0)
        model_call(name, bender_args, "ray_stride_5", "bf16", INVALID, ray_stride=5)
        model_call(name, bender_args, "no_off4", "views", INVALID, off4=None)
        model_call(name, bender_args, "n_rays_zero", "f32", OK, n_rays=0)
        model_call(name, bender_args, "n_rays_zero", "generic", OK, n_rays=0)
    model_call(BB, bender_args, "no_dz_out4", "f32", INVALID, dz_out4=None)
    model_call(B, bender_args, "no_dz_out4_n_rays_zero", "f32", OK, dz_out4=None, n_rays=0)
    model_call(BW, bender_wgrad_args, "n_partials_0", "f32", INVALID, partials=bender_wgrad_bytes(0), n_partials=0)
    model_call(BW, bender_wgrad_args, "n_partials_6", "f32", INVALID, partials=bender_wgrad_bytes(6), n_partials=6)
    model_call(BW, bender_wgrad_args, "n_partials_4097", "bf16", INVALID, partials=bender_wgrad_bytes(4097), n_partials=4097)
    model_call(BW, bender_wgrad_args, "latent_stride_31", "bf16", INVALID, partials=bender_wgrad_bytes(4), latent_stride=31)
    model_call(BW, bender_wgrad_args, "n_rays_zero", "generic", OK, partials=bender_wgrad_bytes(4), n_rays=0)
    model_call(BW, bender_wgrad_args, "n_partials_6_n_rays_zero", "f32", INVALID, partials=bender_wgrad_bytes(6), n_partials=6, n_rays=0)

    D, DB = "nrnerf_bender_divergence_forward", "nrnerf_bender_divergence_backward"
    for name in (D, DB):
        model_call(name, divergence_args, "latent_stride_16", "f32", INVALID, partials=bender_wgrad_bytes(4), latent_stride=16)
        model_call(name, divergence_args, "n_points_negative", "bf16", INVALID, partials=bender_wgrad_bytes(4), n_points=-1)
        model_call(name, divergence_args, "no_toff4", "generic", INVALID, partials=bender_wgrad_bytes(4), toff4=None)
        model_call(name, divergence_args, "n_points_zero", "f32", OK, partials=bender_wgrad_bytes(4), n_points=0)
        model_call(name, divergence_args, "n_points_zero_one_code_for_all", "bf16", OK, partials=bender_wgrad_bytes(4), n_points=0, latent_stride=0)
    # the record-count rules belong to the backward call alone
    for bad in (0, 6, 4097):
        model_call(DB, divergence_args, f"n_partials_{bad}", "f32", INVALID, partials=bender_wgrad_bytes(bad), n_partials=bad)
        model_call(D, divergence_args, f"n_partials_{bad}_n_points_zero", "f32", OK, partials=bender_wgrad_bytes(bad), n_partials=bad, n_points=0)
    model_call(DB, divergence_args, "n_partials_6_n_points_zero", "bf16", INVALID, partials=bender_wgrad_bytes(6), n_partials=6, n_points=0)
    model_call(DB, divergence_args, "no_g_divergence_no_g_tangent", "f32", INVALID, partials=bender_wgrad_bytes(4), g_divergence=None, g_tangent=None)
    model_call(DB, divergence_args, "g_tangent_alone_n_points_zero", "f32", OK, partials=bender_wgrad_bytes(4), g_divergence=None, n_points=0)

    # ---- model-less: aux positions, the workspace of nrnerf_tn_products, host pointers where the owner of device memory is looked up
    def aux(cid, positions, expected):
        def fn(lib, _h, d):
            return lib.nrnerf_reduce_partials_aux(d(), 64, 4, 2, d(), 8, d(), d(), 4, (C.c_int64 * 4)(*positions), STREAM)
        add(f"nrnerf_reduce_partials_aux:{cid}", None, expected, fn)
    aux("aux_pos_0_at_n_out", (8, 1, 2, 3), INVALID)
    aux("aux_pos_3_beyond_n_out", (0, 1, 2, 9), INVALID)

    def tn(cid, expected, offset=0, short=0, host_out=False):
        def fn(lib, _h, d):
            job = _lib.TnJob(a=d(), b=d(), lda=4, ldb=4, wo=4, wi=4, ldo=4, out_offset=0, bias_offset=-1)
            a = tn_args(lambda _n: d(), jobs=C.pointer(job), workspace_bytes=64 - short)      # one chunk of 16 floats
            a.workspace += offset
            if host_out:
                a.out = H
            return lib.nrnerf_tn_products(C.byref(a), STREAM)
        add(f"nrnerf_tn_products:{cid}", None, expected, fn)
    tn("workspace_misaligned", WORKSPACE, offset=4)
    tn("workspace_short", WORKSPACE, short=1)
    tn("workspace_short_and_misaligned", WORKSPACE, offset=8, short=60)
    tn("host_out", INVALID, host_out=True)
    tn("host_out_and_workspace_short", INVALID, host_out=True, short=1)          # (the owner lookup comes first)

    def host(name, fn):
        add(f"{name}:host_pointer", None, INVALID, fn)
    host("nrnerf_code_gradients", lambda lib, _h, d: lib.nrnerf_code_gradients(d(), d(), N, 32, 2, H, STREAM))
    host("nrnerf_merge_rows", lambda lib, _h, d: lib.nrnerf_merge_rows(d(), N, S, I, d(), None, d(), None, H, None, 0, STREAM))
    host("nrnerf_reduce_partials", lambda lib, _h, d: lib.nrnerf_reduce_partials(d(), 64, 4, 2, d(), 8, H, STREAM))
    host("nrnerf_tile_row_sums", lambda lib, _h, d: lib.nrnerf_tile_row_sums(d(), 8, H, STREAM))
    host("nrnerf_tiles_to_rows", lambda lib, _h, d: lib.nrnerf_tiles_to_rows(d(), N, S, 256, H, STREAM))
    host("nrnerf_direction_encoding", lambda lib, _h, d: lib.nrnerf_direction_encoding(d(), N, S, 4, H, 0, None, STREAM))
    host("nrnerf_generate_rays", lambda lib, _h, d: lib.nrnerf_generate_rays(C.byref(camera()), 2.0, 6.0, H, 8, STREAM))
    host("nrnerf_sample_depths", lambda lib, _h, d: lib.nrnerf_sample_depths(d(), 8, None, N, S, 0, H, STREAM))
    host("nrnerf_sample_depths_points", lambda lib, _h, d: lib.nrnerf_sample_depths_points(d(), 8, None, N, S, 0, H, d(), STREAM))
    host("nrnerf_encoding_forward", lambda lib, _h, d: lib.nrnerf_encoding_forward(C.byref(encoding_args(lambda _n: d(), src=H)), STREAM))
    host("nrnerf_loss_forward", lambda lib, _h, d: lib.nrnerf_loss_forward(C.byref(loss_args(lambda _n: d(), loss=H)), STREAM))
    # the backward call takes its device from g_rgb_map, the forward call from loss
    host("nrnerf_loss_backward", lambda lib, _h, d: lib.nrnerf_loss_backward(C.byref(loss_args(lambda _n: d(), g_rgb_map=H)), STREAM))
    host("nrnerf_composite_forward", lambda lib, _h, d: lib.nrnerf_composite_forward(C.byref(composite_args(lambda _n: d(), raw4=H)), STREAM))
    host("nrnerf_composite_backward", lambda lib, _h, d: lib.nrnerf_composite_backward(C.byref(composite_args(lambda _n: d(), raw4=H)), STREAM))
    host("nrnerf_adam_step", lambda lib, _h, d: lib.nrnerf_adam_step(None, C.byref(adam_args(lambda _n: d(), step=H)), STREAM))
    return cases


GPU_CASES = _gpu_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("key,thunk,expected", [pytest.param(key, fn, exp, id=cid) for cid, key, fn, exp in GPU_CASES])
def test_status_on_device(lib, handles, key, thunk, expected):
    d = Device()
    assert thunk(lib, handles[key].handle if key else None, d) == expected
    torch.cuda.synchronize()        # a case whose check were lost would have launched: let it finish before its arrays go
    d.release()


@pytest.mark.gpu
def test_handles_are_what_the_table_assumes(lib, handles):
    kinds = {k: (lib.nrnerf_model_is_generic(m.handle), lib.nrnerf_model_trains_generic(m.handle), lib.nrnerf_model_trains_bender(m.handle),
                 lib.nrnerf_model_precision(m.handle)) for k, m in handles.items()}
    assert kinds == {"f32": (0, 0, 1, 0), "bf16": (0, 0, 1, 1), "views": (0, 0, 1, 1), "generic": (1, 1, 1, 0)}
    gen = handles["generic"].handle
    assert lib.nrnerf_generic_trunk_bits_bytes(gen, 2, N, S) == 0 and lib.nrnerf_generic_trunk_bits_bytes(gen, 0, 0, S) == 0
    assert lib.nrnerf_generic_trunk_bits_bytes(handles["f32"].handle, 0, N, S) == 0
