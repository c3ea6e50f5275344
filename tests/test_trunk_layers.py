"""The trunk training kernels (nrnerf_trunk_forward / _backward, nrnerf_generic_trunk_forward / _backward), LAYER BY LAYER against
float64 (tests/trunk_reference.py): every layer from the kernel's own saved input to it, with an a-priori rounding bound -- no cosine,
no share of elements excused.  The one comparison that skips anything is relu bit == (pre64 > 0), on elements whose float64
pre-activation is within the bound of zero: at most 1e-3 of a layer (at least one element); bit == (stored > 0) holds on every element.

Every output buffer starts as NaN with a guard region behind it: every promised element is written, padded activation columns are
finite, padded gradient columns are exactly zero, the guards are untouched.  Each test prints the worst residual / bound per array.

Worst residual / bound seen on an MI355X over all cases below (a bf16 store alone reaches 1 at the bottom of a binade, where half an ulp
is the whole u16 |x| of the bound; the fp32 figures show how little of the accumulation bound is used):
  compiled, bf16: acts 0.988, hv 0.975, raw4 0.006, raw 0.004, d_pre 0.996, d_pre_v 0.980, d_pts4 0.157, d_dirs 0.002
  compiled, fp32: acts 0.039, hv 0.014, raw4 0.012, raw 0.005, d_pre 0.188, d_pre_v 0.216, d_pts4 0.002, d_dirs 0.006
  generic, bf16 (both backward routes alike): acts 0.982, raw4 0.009, raw 0.006, d_pre 0.995, d_enc0 0.015, d_enc1 0.008, d_encv 0.015
  generic, fp32: acts 0.046, raw4 0.020, raw 0.006, d_pre 0.345, d_enc0 0.021, d_enc1 0.031, d_encv 0.037
No relu bit was wrong.  Undecided shares: at most 5.1e-4 of any layer, the layers that read an encoding included; one element of the 768
of a three-sample layer (1.3e-3) in three of the four (1, 3) cases."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from nonrigid_nerf_amd import render as R
from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_scene
from tests import trunk_reference as T

DEV = "cuda:0"
GUARD = 4096                     # bytes behind every output buffer
GUARD_BYTE = 0xA5


class Out:
    """An output buffer: its bytes all ones (NaN in bf16 and fp32) and a guard region behind it."""

    def __init__(self, shape, dtype):
        self.n = int(torch.tensor(shape).prod()) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.raw[self.n:] = GUARD_BYTE
        self.t = self.raw[:self.n].view(dtype).view(*shape)
        self.ptr = self.t.data_ptr()

    def guard_ok(self):
        return bool((self.raw[self.n:] == GUARD_BYTE).all())


def _finish(rep, outs, written, label):
    for name, o in outs.items():
        rep.exact(name, o.guard_ok(), "the guard region behind the buffer was written")
    for name, t in written.items():
        rep.exact(name, bool(torch.isfinite(t.float()).all()), "an element the header promises was not written")
    print(f"\n[{label}] worst residual / bound: {rep.summary()}")
    assert not rep.failures, rep.failures


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    """the cached scenes, modules and handles live as long as this module's tests"""
    yield
    _compiled.cache_clear()
    _generic.cache_clear()
    torch.cuda.empty_cache()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _compiled(cfg_items, which, precision):
    """scene, device modules, handle and operand weights of one compiled configuration (shared by its cases; never modified)"""
    cfg = SceneConfig(N_importance=64, **dict(cfg_items))
    scene = make_scene(cfg, 1)
    rb, coarse, fine = build_modules(scene, device=DEV)
    for m in (rb, coarse, fine):
        if m is not None:
            m.requires_grad_(False)
    model = R.get_model(coarse, fine, precision=precision, device=torch.device(DEV))
    assert model.lib.nrnerf_model_trains_generic(model.handle) == 0 and model.lib.nrnerf_model_is_generic(model.handle) == 0
    return cfg, model, (rb, coarse, fine), T.compiled_operands(scene, which, precision)


def _inputs(n_rays, S, seed):
    gen = torch.Generator().manual_seed(seed)
    M = n_rays * S
    pts4 = torch.zeros(M, 4)
    pts4[:, :3] = torch.randn(M, 3, generator=gen) * 0.4
    d_raw4 = torch.randn(M, 4, generator=gen)
    dirs = F.normalize(torch.randn(M, 3, generator=gen), dim=-1)
    return pts4.to(DEV), d_raw4.to(DEV), dirs.to(DEV), gen


def run_compiled(cfg_kw, which, n_rays, S, precision="bf16", raw_ch=None, ray_bias=False, label=""):
    from nonrigid_nerf_amd import _lib
    cfg, model, _, ops = _compiled(tuple(sorted(cfg_kw.items())), which, precision)
    b16 = precision != "f32"
    D, W, M = ops.depth, ops.width, n_rays * S
    views = cfg.use_viewdirs
    nblk = n_rays * ((S + 31) // 32)
    pts4, d_raw4, dirs, gen = _inputs(n_rays, S, 100 * n_rays + S)
    rbias = (torch.randn(n_rays, 2, W, generator=gen) * 0.3).to(DEV) if ray_bias else None
    adt = torch.bfloat16 if b16 else torch.float32
    ashape = (D, nblk, W, 32) if b16 else (D, M, W)
    vshape = (nblk, W // 2, 32) if b16 else (M, W // 2)
    o = dict(acts=Out(ashape, adt), raw4=Out((M, 4), torch.float32), d_pre=Out(ashape, adt), d_pts4=Out((M, 4), torch.float32))
    if b16:
        o["relu_mask"] = Out((D, nblk, 64, W // 32), torch.int16)
    if raw_ch:
        o["raw"] = Out((M, raw_ch), torch.float32)
    if views:
        o.update(hv=Out(vshape, adt), d_pre_v=Out(vshape, adt), d_dirs=Out((M, 3), torch.float32))
        if b16:
            o["hv_mask"] = Out((nblk, 64, W // 64), torch.int16)
    a = _lib.TrunkArgs()
    a.struct_size = C.sizeof(_lib.TrunkArgs)
    a.which, a.n_rays, a.n_samples = which, n_rays, S
    a.pts4, a.acts, a.raw4 = pts4.data_ptr(), o["acts"].ptr, o["raw4"].ptr
    a.relu_mask = o["relu_mask"].ptr if b16 else None
    if raw_ch:
        a.raw, a.raw_ch = o["raw"].ptr, raw_ch
    if rbias is not None:
        a.ray_bias = rbias.data_ptr()
    if views:
        a.dirs, a.hv, a.hv_mask = dirs.data_ptr(), o["hv"].ptr, (o["hv_mask"].ptr if b16 else None)
    _lib.check(model.lib.nrnerf_trunk_forward(model.handle, C.byref(a), _stream()), "nrnerf_trunk_forward")
    a.d_raw4, a.d_pre, a.d_pts4 = d_raw4.data_ptr(), o["d_pre"].ptr, o["d_pts4"].ptr
    if views:
        a.d_pre_v, a.d_dirs = o["d_pre_v"].ptr, o["d_dirs"].ptr
    _lib.check(model.lib.nrnerf_trunk_backward(model.handle, C.byref(a), _stream()), "nrnerf_trunk_backward")
    torch.cuda.synchronize()

    rep = T.Report()
    sh3 = lambda t: t.view(n_rays, S, -1)
    if b16:
        acts, acts_pad = T.tiles_to_rows(o["acts"].t, n_rays, S)
        d_pre, d_pad = T.tiles_to_rows(o["d_pre"].t, n_rays, S)
        bits, _ = T.relu_records_to_bool(o["relu_mask"].t, n_rays, S)
        T.check_padding(rep, acts_pad, d_pad)
    else:
        acts, d_pre = T.rowmajor_to_rows(o["acts"].t, n_rays, S), T.rowmajor_to_rows(o["d_pre"].t, n_rays, S)
        bits = acts > 0
    written = dict(acts=acts, d_pre=d_pre, raw4=o["raw4"].t, d_pts4=o["d_pts4"].t)
    kw_f, kw_b = {}, {}
    if views:
        if b16:
            hv, hv_pad = T.tiles_to_rows(o["hv"].t, n_rays, S)
            zv, zv_pad = T.tiles_to_rows(o["d_pre_v"].t, n_rays, S)
            hv_bits, _ = T.relu_records_to_bool(o["hv_mask"].t, n_rays, S)
            T.check_padding(rep, hv_pad, zv_pad)
        else:
            hv, zv = sh3(o["hv"].t), sh3(o["d_pre_v"].t)
            hv_bits = hv > 0
        kw_f = dict(dirs=sh3(dirs), hv=hv, hv_bits=hv_bits)
        kw_b = dict(dirs=sh3(dirs), hv_bits=hv_bits, d_pre_v=zv, d_dirs=sh3(o["d_dirs"].t))
        written.update(hv=hv, d_pre_v=zv, d_dirs=o["d_dirs"].t)
    if raw_ch:
        written["raw"] = o["raw"].t
    T.check_compiled_forward(ops, b16, sh3(pts4)[..., :3], acts, bits if b16 else None, sh3(o["raw4"].t), sh3(o["raw"].t) if raw_ch else None,
                             ray_bias=rbias, rep=rep, **kw_f)
    T.check_compiled_backward(ops, b16, sh3(pts4)[..., :3], sh3(d_raw4), bits, d_pre, sh3(o["d_pts4"].t), rep=rep, **kw_b)
    _finish(rep, o, written, f"compiled trunk {precision} {label or cfg_kw} which {which} ({n_rays}, {S})")
    return rep


PLAIN, NARROW, VIEWS, TCB = {}, dict(netwidth=128), dict(use_viewdirs=True), dict(ray_bending=False, time_conditioned_baseline=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays,S,which,raw_ch", [(1, 3, 1, None), (5, 33, 0, 5), (3, 64, 1, 4), (2, 1024, 0, None)],
                         ids=["one_partial_block", "second_block_of_one_sample", "whole_blocks", "max_samples"])
def test_compiled_bf16_trunk_w256_layer_by_layer(n_rays, S, which, raw_ch):
    run_compiled(PLAIN, which, n_rays, S, raw_ch=raw_ch)


@pytest.mark.gpu
def test_compiled_bf16_trunk_second_trip_through_the_grid_stride_loop():
    """8 CUs + 3 blocks (rounded up to whole rays of two blocks): more blocks than the launch keeps waves resident, so some workgroups
    go through their loop twice, the weight ring carried across"""
    cus = torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count
    run_compiled(PLAIN, 1, (8 * cus + 3 + 1) // 2, 33)


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays,S", [(5, 33), (7, 85)])
def test_compiled_bf16_trunk_w128_layer_by_layer(n_rays, S):
    run_compiled(NARROW, 1, n_rays, S, raw_ch=5)


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays,S,which", [(5, 33, 1), (1, 3, 0)])
def test_compiled_bf16_trunk_with_the_view_dependent_head_layer_by_layer(n_rays, S, which):
    run_compiled(VIEWS, which, n_rays, S, raw_ch=4)


@pytest.mark.gpu
def test_compiled_bf16_trunk_with_per_ray_bias_layer_by_layer():
    run_compiled(TCB, 1, 4, 40, ray_bias=True)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_kw,n_rays,S", [(PLAIN, 5, 33), (PLAIN, 1, 3), (VIEWS, 5, 33)], ids=["plain_5x33", "plain_1x3", "views_5x33"])
def test_compiled_fp32_trunk_layer_by_layer(cfg_kw, n_rays, S):
    run_compiled(cfg_kw, 1, n_rays, S, precision="f32", raw_ch=4 if cfg_kw else 5)


# ---- the generic entry points -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _generic(cfg_items, precision):
    cfg = SceneConfig(N_importance=64, **dict(cfg_items))
    scene = make_scene(cfg, 1)
    rb, coarse, fine = build_modules(scene, device=DEV)
    for m in (rb, coarse, fine):
        if m is not None:
            m.requires_grad_(False)
    model = R.get_model(coarse, fine, precision=precision, device=torch.device(DEV))
    assert model.lib.nrnerf_model_trains_generic(model.handle) == 1
    return cfg, model, (rb, coarse, fine)


def run_generic(cfg_kw, n_rays, S, precision="bf16", which=1):
    from nonrigid_nerf_amd import _lib
    cfg, model, (rb, coarse, fine) = _generic(tuple(sorted(cfg_kw.items())), precision)
    net = fine if which == 1 else coarse
    b16 = precision != "f32"
    D, W, M = int(net.D), int(net.W), n_rays * S
    views = bool(net.use_viewdirs)
    slots = D + (2 if views else 0)
    n_enc = int(net.input_ch)
    skips = [int(k) for k in net.skips]
    pts4, d_raw4, dirs, gen = _inputs(n_rays, S, 7 * n_rays + S)
    adt = torch.bfloat16 if b16 else torch.float32
    C_out = 4 if views else int(net.output_linear.weight.shape[0])
    o = dict(acts=Out((slots, M, W), adt), raw4=Out((M, 4), torch.float32), raw=Out((M, C_out), torch.float32))
    a = _lib.GenericTrunkArgs()
    a.struct_size = C.sizeof(_lib.GenericTrunkArgs)
    a.which, a.n_rays, a.n_samples = which, n_rays, S
    a.pts4, a.acts, a.raw4, a.raw, a.raw_ch = pts4.data_ptr(), o["acts"].ptr, o["raw4"].ptr, o["raw"].ptr, C_out
    nbits = int(model.lib.nrnerf_generic_trunk_bits_bytes(model.handle, which, n_rays, S))
    assert (nbits > 0) == (b16 and not views), "the width-class route: bf16 handles with the plain head"
    if nbits:
        o["relu_bits"] = Out((nbits,), torch.uint8)
        a.relu_bits = o["relu_bits"].ptr
    if views:
        a.dirs = dirs.data_ptr()
    _lib.check(model.lib.nrnerf_generic_trunk_forward(model.handle, C.byref(a), _stream()), "nrnerf_generic_trunk_forward")
    torch.cuda.synchronize()
    rep = T.Report()
    sh3 = lambda t: t.view(n_rays, S, -1)
    acts = T.rowmajor_to_rows(o["acts"].t, n_rays, S)
    gx_bits = T.gx_relu_bits_to_bool(o["relu_bits"].t, D, n_rays, S, W) if nbits else None
    T.check_generic_forward(net, b16, sh3(pts4)[..., :3], acts, sh3(o["raw4"].t), sh3(o["raw"].t), dirs=sh3(dirs), gx_bits=gx_bits, rep=rep)
    half = int(net.views_linears[0].weight.shape[0]) if views else 0
    written = dict(acts=acts[:D], raw4=o["raw4"].t, raw=o["raw"].t)
    if views:
        written.update(feature=acts[D], colour=acts[D + 1][..., :half])
    # backward: on the width-class route with the forward's relu bits, and on the run-time-parameterised route without them
    for route, use_bits in (("width-class", True), ("run-time-parameterised", False)) if nbits else (("run-time-parameterised", False),):
        ob = dict(d_pre=Out((slots, M, W), adt), d_enc0=Out((M, n_enc), torch.float32))
        if skips:
            ob["d_enc1"] = Out((M, n_enc), torch.float32)
        if views:
            ob["d_encv"] = Out((M, int(net.input_ch_views)), torch.float32)
        a.d_raw4, a.d_pre, a.d_enc0 = d_raw4.data_ptr(), ob["d_pre"].ptr, ob["d_enc0"].ptr
        a.d_enc1 = ob["d_enc1"].ptr if skips else None
        a.d_encv = ob["d_encv"].ptr if views else None
        a.relu_bits = o["relu_bits"].ptr if use_bits else None
        _lib.check(model.lib.nrnerf_generic_trunk_backward(model.handle, C.byref(a), _stream()), "nrnerf_generic_trunk_backward")
        torch.cuda.synchronize()
        d_pre = T.rowmajor_to_rows(ob["d_pre"].t, n_rays, S)
        tag = f"{route}: "
        T.check_generic_backward(net, b16, sh3(d_raw4), gx_bits if use_bits else acts[:D] > 0, d_pre, sh3(ob["d_enc0"].t),
                                 sh3(ob["d_enc1"].t) if skips else None, sh3(ob["d_encv"].t) if views else None,
                                 hv_bits=(acts[D + 1][..., :half] > 0) if views else None, rep=rep, tag=tag)
        for k, v in ob.items():
            o[tag + k] = v
            if k != "d_pre":
                written[tag + k] = v.t
        written[tag + "d_pre"] = d_pre[:D]
        if views:
            written[tag + "d feature"], written[tag + "d colour"] = d_pre[D], d_pre[D + 1][..., :half]
    _finish(rep, o, written, f"generic trunk {precision} {cfg_kw} which {which} ({n_rays}, {S})")
    return rep


G192 = dict(netdepth=6, netwidth=192, skips=(2,))
G320 = dict(netdepth=5, netwidth=320, skips=(2,), multires=6)
G64 = dict(netdepth=3, netwidth=64, skips=())
GVIEWS = dict(netdepth=4, netwidth=128, skips=(1,), use_viewdirs=True, multires_views=2)


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays,S", [(1, 3), (3, 17), (5, 33)])
def test_generic_bf16_trunk_d6_w192_both_backward_routes_layer_by_layer(n_rays, S):
    run_generic(G192, n_rays, S)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_kw,n_rays,S", [(G320, 3, 21), (G64, 3, 21), (GVIEWS, 3, 21)], ids=["d5_w320_l6", "d3_w64_no_skip", "d4_w128_views_lv2"])
def test_generic_bf16_trunk_other_shapes_layer_by_layer(cfg_kw, n_rays, S):
    run_generic(cfg_kw, n_rays, S)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_kw,n_rays,S", [(G192, 3, 17), (GVIEWS, 3, 21)], ids=["d6_w192", "d4_w128_views_lv2"])
def test_generic_fp32_trunk_layer_by_layer(cfg_kw, n_rays, S):
    run_generic(cfg_kw, n_rays, S, precision="f32")
