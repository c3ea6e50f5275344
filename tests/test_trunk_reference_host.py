"""CPU-tier checks of tests/trunk_reference.py, the float64 layer reference the GPU tests of the trunk training kernels
(tests/test_trunk_layers.py) stand on: its decoders invert an encoder written the other way round, an EMULATED kernel (torch fp32
matmuls over the same rounded operands, relu, ``.bfloat16()``) stays inside every bound, the share of relu elements the bit check may
skip stays under 1e-3 in every layer, and deliberately damaged emulations are rejected -- the comparison has teeth before it ever sees
a GPU.  (That the kernels follow the layouts the decoders assume is what the GPU tests pin, not this file.)"""
import functools

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd.synthetic import SceneConfig, make_scene
from tests import trunk_reference as T


# ---- an encoder of the saved arrays, written from the kernel's side: per block, lane and register ---------------------------------
def encode_tiles(rows, pad_value):
    """rows [N, S, F] -> [B, F, 32]: block b of a ray holds samples 32 b .. 32 b + 31, the columns beyond the ray's end pad_value"""
    N, S, F = rows.shape
    bpr = (S + 31) // 32
    out = torch.full((N * bpr, F, 32), pad_value, dtype=rows.dtype)
    for ray in range(N):
        for blk in range(bpr):
            for j in range(32):
                s = 32 * blk + j
                if s < S:
                    out[ray * bpr + blk, :, j] = rows[ray, s]
    return out


def encode_relu_records(bits, pad_bit):
    """bool [N, S, F] -> int16 [B, 64, F / 32]: lane 32 h + j holds sample j; its 16 values of tile t are accumulator registers r = 0..15 =
    features 32 t + 4 h + (r & 3) + 8 (r >> 2) (the D layout of v_mfma_f32_32x32: four consecutive rows per register quad, quads 8 apart)"""
    N, S, F = bits.shape
    bpr, NT = (S + 31) // 32, F // 32
    out = np.zeros((N * bpr, 64, NT), dtype=np.uint16)
    b = bits.numpy()
    for ray in range(N):
        for blk in range(bpr):
            for lane in range(64):
                h, j = lane >> 5, lane & 31
                s = 32 * blk + j
                for t in range(NT):
                    m = 0
                    for r in range(16):
                        f = 32 * t + 4 * h + (r & 3) + 8 * (r >> 2)
                        m |= int(b[ray, s, f] if s < S else pad_bit) << r
                    out[ray * bpr + blk, lane, t] = m
    return torch.from_numpy(out.view(np.int16).copy())


@pytest.mark.parametrize("n_rays,S,F", [(1, 3, 64), (3, 33, 128), (2, 64, 64), (2, 85, 256)])
def test_decoders_invert_the_encoders_on_ragged_shapes(n_rays, S, F):
    gen = torch.Generator().manual_seed(S)
    rows = torch.randn(n_rays, S, F, generator=gen).to(torch.bfloat16)
    got, pad = T.tiles_to_rows(encode_tiles(rows, 7.0), n_rays, S)
    assert torch.equal(got, rows) and pad.shape[-2] == 32 * ((S + 31) // 32) - S and bool((pad == 7.0).all())
    stacked = torch.stack([encode_tiles(rows, 0.0), encode_tiles(-rows, 0.0)])
    assert torch.equal(T.tiles_to_rows(stacked, n_rays, S)[0], torch.stack([rows, -rows]))
    bits = torch.rand(n_rays, S, F, generator=gen) < 0.4
    got, pad = T.relu_records_to_bool(encode_relu_records(bits, True), n_rays, S)
    assert torch.equal(got, bits) and bool(pad.all())
    got, pad = T.relu_records_to_bool(torch.stack([encode_relu_records(bits, False), encode_relu_records(~bits, False)]), n_rays, S)
    assert torch.equal(got, torch.stack([bits, ~bits])) and not bool(pad.any())
    flat = torch.randn(3, n_rays * S, F, generator=gen)
    assert torch.equal(T.rowmajor_to_rows(flat, n_rays, S)[1, n_rays - 1, S - 1], flat[1, -1])


def encode_gx_relu_bits(bits):
    """bool [D, N, S, W] -> the width-class route's bytes [D][16-sample block][64 lanes][4 ceil(WC / 128)], from the kernel's side: lane
    16 g + n holds sample n; byte p of its record is tile pair p, whose packed fragment holds features 32 p + 4 g .. + 3 in elements 0..3
    and 32 p + 16 + 4 g .. + 3 in elements 4..7 (csrc/nrnerf_gx16.h keep)"""
    D, N, S, W = bits.shape
    WC = (W + 63) // 64 * 64
    NP, bpr = WC // 32, (S + 15) // 16
    bpl = 4 * ((NP + 3) // 4)
    buf = np.zeros((D, N * bpr, 64, bpl), np.uint8)
    b = bits.numpy()
    for l in range(D):
        for ray in range(N):
            for blk in range(bpr):
                for lane in range(64):
                    g, n = lane >> 4, lane & 15
                    s_ = blk * 16 + n
                    if s_ >= S:
                        continue
                    for p_ in range(NP):
                        byte = 0
                        for e in range(8):
                            f = 32 * p_ + 4 * g + e if e < 4 else 32 * p_ + 16 + 4 * g + e - 4
                            byte |= int(f < W and b[l, ray, s_, f]) << e
                        buf[l, ray * bpr + blk, lane, p_] = byte
    return torch.from_numpy(buf).reshape(-1)


@pytest.mark.parametrize("n_rays,S,W", [(1, 3, 64), (2, 21, 192), (2, 33, 320)])
def test_width_class_relu_bits_decoder_inverts_its_encoder(n_rays, S, W):
    bits = torch.rand(2, n_rays, S, W, generator=torch.Generator().manual_seed(W)) < 0.5
    assert torch.equal(T.gx_relu_bits_to_bool(encode_gx_relu_bits(bits), 2, n_rays, S, W), bits)


def test_relu_record_bit_map_is_the_accumulator_layout():
    """The decoder puts single bits where the formula stated in include/nrnerf.h says, at hand-worked positions.  (Decoder and encoder
    here share that formula: that the KERNEL follows it is pinned by the GPU tests' bit check, tests/test_trunk_layers.py.)"""
    for lane, t, r, want in ((0, 0, 0, 0), (0, 0, 3, 3), (0, 0, 4, 8), (0, 0, 15, 27), (32, 0, 0, 4), (37, 2, 9, 64 + 4 + 1 + 16), (63, 7, 15, 255)):
        rec = torch.zeros(1, 64, 8, dtype=torch.int16)
        rec[0, lane, t] = int(np.array(1 << r, dtype=np.uint16).view(np.int16))
        rows, _ = T.relu_records_to_bool(rec, 1, 32)
        assert rows.sum() == 1 and bool(rows[0, lane & 31, want]), (lane, t, r, want)
        assert T.tile_feature(t, lane >> 5, r) == want


# ---- the emulated kernel ------------------------------------------------------------------------------------------------------------
N_RAYS, S_ = 64, 64                   # 4096 points


@functools.lru_cache(maxsize=None)
def _setup(width):
    scene = make_scene(SceneConfig(N_importance=64, netwidth=width), 1)
    ops = T.compiled_operands(scene, 1, "bf16")
    gen = torch.Generator().manual_seed(21)
    pts = torch.randn(N_RAYS, S_, 3, generator=gen) * 0.4
    d_raw4 = torch.randn(N_RAYS, S_, 4, generator=gen)
    return scene, ops, pts, d_raw4


def _bf16_nearest(x):
    return x.bfloat16()


def _bf16_truncate(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def emulate(ops, pts, d_raw4, drop_slab=None, to_bf16=_bf16_nearest):
    """The kernels' arithmetic in torch: fp32 matmuls over the rounded operands, relu, bf16 stores; drop_slab = (layer, k-slab) leaves 32
    input columns of one forward layer out."""
    f = lambda t: t.float()
    cols = [pts]
    for k in range(ops.L):
        cols += [torch.sin(pts * 2.0 ** k), torch.cos(pts * 2.0 ** k)]
    enc = torch.cat(cols, -1).half().float()
    acts, bits = [], []
    h = None
    for i in range(ops.depth):
        X = enc if i == 0 else (torch.cat([enc, h], -1) if i - 1 == ops.skip else h)
        if drop_slab is not None and drop_slab[0] == i:
            X = X.clone()
            X[..., 32 * drop_slab[1]:32 * drop_slab[1] + 32] = 0.0
        acc = X @ f(ops.W[i]).T + f(ops.b[i])
        bits.append(acc > 0)
        acts.append(to_bf16(torch.relu(acc)))
        h = acts[-1].float()
    rawf = h @ f(ops.head[0]).T + f(ops.head[1])
    g = torch.cat([d_raw4.bfloat16().float(), torch.zeros_like(d_raw4)], -1)
    d_pre = [None] * ops.depth
    dh = g @ f(ops.head_t).T
    denc = 0.0
    for i in range(ops.depth - 1, -1, -1):
        d_pre[i] = to_bf16(torch.where(bits[i], dh, torch.zeros_like(dh)))
        z = d_pre[i].float()
        if i in ops.enc_t:
            denc = denc + z @ f(ops.enc_t[i]).T
        if i > 0:
            dh = z @ f(ops.hid_t[i]).T
    dp = denc[..., :3].clone()
    for k in range(ops.L):
        s, c = torch.sin(pts * 2.0 ** k), torch.cos(pts * 2.0 ** k)
        dp = dp + 2.0 ** k * (c * denc[..., 3 + 6 * k:6 + 6 * k] - s * denc[..., 6 + 6 * k:9 + 6 * k])
    d_pts4 = torch.cat([dp, torch.zeros_like(dp[..., :1])], -1)
    return dict(acts=acts, bits=bits, raw=rawf, raw4=rawf[..., :4].contiguous(), d_pre=d_pre, d_pts4=d_pts4)


def check(ops, pts, d_raw4, e, bits=None):
    rep = T.Report()
    bits = torch.stack(e["bits"]) if bits is None else bits
    acts, d_pre = torch.stack(e["acts"]), torch.stack(e["d_pre"])
    T.check_compiled_forward(ops, True, pts, acts, bits, e["raw4"], e["raw"], rep=rep)
    T.check_compiled_backward(ops, True, pts, d_raw4, bits, d_pre, e["d_pts4"], rep=rep)
    return rep


@pytest.mark.parametrize("width", [256, 128])
def test_emulated_kernel_stays_inside_every_bound(width):
    scene, ops, pts, d_raw4 = _setup(width)
    e = emulate(ops, pts, d_raw4)
    rep = check(ops, pts, d_raw4, e)
    print(f"\n[emulated bf16 trunk, W {width}, 4096 points] worst residual / bound: {rep.summary()}")
    assert not rep.failures, rep.failures
    assert len(rep.undecided) == ops.depth and max(rep.undecided.values()) <= T.UNDECIDED_CAP, rep.undecided
    assert rep.worst("") <= 1.0
    # the packed images' operands ARE the module's weights rounded with torch: f16 where a weight meets an encoding, bf16 elsewhere
    from nonrigid_nerf_amd.synthetic import build_modules
    _, _, fine = build_modules(scene)
    Wm, bm, extra = T.module_operands(fine, True)
    for i in range(ops.depth):
        assert torch.equal(Wm[i], ops.W[i]) and torch.equal(bm[i], ops.b[i]), i
    assert torch.equal(extra["output"][0], ops.head[0]) and torch.equal(extra["output"][1], ops.head[1])
    n_enc = 3 + 6 * ops.L
    for i in range(1, ops.depth):
        assert torch.equal(ops.hid_t[i], T.round_to(fine.pts_linears[i].weight[:, -width:].T, torch.bfloat16)), i
    assert torch.equal(ops.enc_t[0], T.round_to(fine.pts_linears[0].weight.T, torch.bfloat16))
    assert torch.equal(ops.enc_t[ops.skip + 1], T.round_to(fine.pts_linears[ops.skip + 1].weight[:, :n_enc].T, torch.bfloat16))
    assert torch.equal(ops.head_t[:, :5], T.round_to(fine.output_linear.weight.T, torch.bfloat16)) and not ops.head_t[:, 5:].any()


def test_damaged_emulations_are_rejected():
    scene, ops, pts, d_raw4 = _setup(128)
    good = emulate(ops, pts, d_raw4)
    # one 32-column k-slab of the skip layer dropped
    rep = check(ops, pts, d_raw4, emulate(ops, pts, d_raw4, drop_slab=(ops.skip + 1, 2)))
    assert any(f.startswith(f"acts[{ops.skip + 1}]") for f in rep.failures), rep.failures
    # ... and of an ordinary hidden layer
    rep = check(ops, pts, d_raw4, emulate(ops, pts, d_raw4, drop_slab=(2, 3)))
    assert any(f.startswith("acts[2]") for f in rep.failures), rep.failures
    # two features' relu bits swapped in one layer's record: the forward bit check and the backward layer that applies them both see it
    bits = torch.stack(good["bits"]).clone()
    bits[3, ..., 5], bits[3, ..., 6] = good["bits"][3][..., 6], good["bits"][3][..., 5]
    rep = check(ops, pts, d_raw4, good, bits=bits)
    assert any(f.startswith("relu[3]") for f in rep.failures) and any(f.startswith("d_pre[3]") for f in rep.failures), rep.failures
    # round toward zero instead of round to nearest
    rep = check(ops, pts, d_raw4, emulate(ops, pts, d_raw4, to_bf16=_bf16_truncate))
    assert any(f.startswith("acts[") for f in rep.failures) and any(f.startswith("d_pre[") for f in rep.failures), rep.failures
    # a nonzero gradient left in a padded column (ragged rays: 3 rays of 33 samples)
    e3 = dict(acts=[a[:3, :33] for a in good["acts"]], d_pre=[d[:3, :33] for d in good["d_pre"]])

    def tiles(rows, pad):
        return torch.stack([encode_tiles(r, pad) for r in rows])
    for pad_grad, bad in ((0.0, False), (2.0 ** -20, True)):
        _, acts_pad = T.tiles_to_rows(tiles(e3["acts"], 1.0), 3, 33)
        _, d_pad = T.tiles_to_rows(tiles(e3["d_pre"], pad_grad), 3, 33)
        rep = T.check_padding(T.Report(), acts_pad, d_pad)
        assert bool(rep.failures) == bad, rep.failures
    _, acts_pad = T.tiles_to_rows(tiles(e3["acts"], float("inf")), 3, 33)
    assert T.check_padding(T.Report(), acts_pad, None).failures


# ---- the generic kernels' operands: the module's weights rounded with torch ARE what the width-class image holds --------------------
def width_class_image_operands(coarse, fine, cfg):
    """The weight matrices and biases in the width-class trunk image (nrnerf_pack_host which = 12, bf16), read fragment by fragment
    (trunk_reference.frag16_image_operands, layout "gx")."""
    skip = cfg.skips[0] if cfg.skips else -1
    return T.frag16_image_operands(T._pack_image(coarse, fine, "bf16", 12), "bf16", cfg.netwidth, cfg.netdepth, cfg.multires, skip, "gx")


@pytest.mark.parametrize("cfg_kw", [dict(netdepth=6, netwidth=192, skips=(2,)), dict(netdepth=3, netwidth=64, skips=())], ids=["d6_w192", "d3_w64_no_skip"])
def test_module_operands_agree_with_the_width_class_image(cfg_kw):
    """The generic kernels' reference multiplies by the module's weights rounded with torch (trunk_reference.module_operands): f16 where a
    weight meets the encoding, bf16 elsewhere, biases as they are.  They are, value for value, what the packed width-class image holds
    (zero in the padding up to the width class)."""
    from nonrigid_nerf_amd.synthetic import build_modules
    cfg = SceneConfig(N_importance=64, **cfg_kw)
    _, coarse, fine = build_modules(make_scene(cfg, 1))
    layers, head = width_class_image_operands(coarse, fine, cfg)
    Ws, bs, extra = T.module_operands(fine, True)
    W, n_enc = cfg.netwidth, 3 + 6 * cfg.multires

    def same(got, want_w, want_b, n_lead):
        gw, gb = got
        ow = want_w.shape[0]
        assert torch.equal(gb[:ow], want_b) and not gb[ow:].any()
        assert torch.equal(gw[:ow, :n_lead], want_w[:, :n_lead]) and not gw[ow:].any()
        hid = want_w.shape[1] - n_lead
        assert torch.equal(gw[:ow, n_lead:n_lead + hid], want_w[:, n_lead:]) and not gw[:, n_lead + hid:].any()
    for i in range(cfg.netdepth):
        same(layers[i], Ws[i], bs[i], n_enc if (i == 0 or (i - 1) in cfg.skips) else 0)
    same(head, extra["output"][0], extra["output"][1], 0)
