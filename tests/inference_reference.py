"""A float64 model of what a 16-bit INFERENCE trunk computes, with the kernels' rounding points made explicit -- for net_kernel_x16
(csrc/nrnerf_net_x16.h), the 32x32x16 trunk kernels (csrc/nrnerf_net_mb.h / nrnerf_net_impl.h), gx16_kernel (csrc/nrnerf_gx16.h) and
gen_kernel's 16-bit modes (csrc/nrnerf_generic.h).  Plain torch; no kernels; imports without a GPU; every function runs on the device of
``pts``.  tests/test_inference_reference_host.py holds it to itself on the CPU, tests/test_inference_trunks.py holds the kernels to it.

The rounding points, and the line that decides each:

* the encoding is an f16 operand in BOTH 16-bit modes -- ``using PE = PolF16`` (nrnerf_net_x16.h; the mb kernels' ``PE``), ``(_Float16)sv``
  (nrnerf_gx16.h), ``gen_cvt<PE>`` (nrnerf_generic.h) -- of an fp32 sin / cos: the hardware path ``v_fract(x fl(1 / 2 pi) 2^f)`` ->
  ``v_sin_f32`` in the first three families (enc_sincos), libm ``sinf(x 2^f)`` in gen_kernel; both lie within
  ``trunk_reference.sincos_error_bound`` of the true value.  The identity columns are f16 of the fp32 coordinate.  The weights that meet an
  encoding column are f16 fragments (frag_is_f16, nrnerf_plan.h), every other weight has the mode's type;
* the layer behind the skip reads the SAME f16 encoding registers a second time (``dense_x16<PE, P, .., NS_E, NS_H>(st, bias_lane, enc, ha,
  ..)``), as the leading k-steps of its sum;
* a hidden activation is converted to the mode's 16-bit type, round to nearest even (v_cvt_pk_{bf16,f16}_f32), and the relu is taken of the
  ROUNDED value (``x16_pack``: ``__builtin_elementwise_max(q, 0)`` on the packed 16-bit integers; ``pack16``) -- gen_kernel takes ``fmaxf``
  first and converts then, which is the same value: rounding is monotone and keeps the sign;
* accumulation is fp32 (the MFMA's), the bias is its C operand; products of two 16-bit values are exact in fp32;
* the head's accumulators go to memory as they are: fp32, no rounding (``raw[b] = d0``).
* a view-dependent head (compiled kernels): views_linears[0] o feature_linear is ONE layer, folded on the host in float64 and rounded once
  (FoldedViews, csrc/nrnerf_pack.cpp); its direction-encoding columns are f16, its hidden columns the mode's type; alpha_linear and rgb_linear
  have the mode's type; the colour branch's activations are rounded like a hidden layer's.

The operand weights are the module's weights rounded with torch (``operands``); tests/test_inference_reference_host.py proves that the packed
images of every family a GPU case uses hold exactly those values."""
import dataclasses

import numpy as np
import torch

from tests.trunk_reference import U32, encoding64, encoding_operand, layer64, module_operands, round_to, sincos_error_bound

DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}


@dataclasses.dataclass
class Operands:
    """float64 tensors: W[i] [width, K_i] (columns [encoding | hidden] in layer 0 and behind a skip), b[i]; head (W, b) of a plain head;
    alpha, views (W_dir [half, 3 + 6 LV], W_hid [half, width], b: the folded layer), rgb of a view-dependent one."""
    W: list
    b: list
    head: tuple
    alpha: tuple
    views: tuple
    rgb: tuple
    reads_enc: list
    L: int
    LV: int

    def to(self, dev):
        mv = lambda t: None if t is None else tuple(x.to(dev) for x in t)
        return Operands([w.to(dev) for w in self.W], [b.to(dev) for b in self.b], mv(self.head), mv(self.alpha), mv(self.views), mv(self.rgb),
                        self.reads_enc, self.L, self.LV)


def folded_views(net):
    """views_linears[0] o feature_linear as csrc/nrnerf_pack.cpp FoldedViews forms it: float64 products summed in k order, rounded to fp32
    once.  -> (W_hid [half, width], W_dir [half, 3 + 6 LV], b [half]), fp32 values."""
    Wn = int(net.W)
    v = net.views_linears[0].weight.detach().cpu().double().numpy()
    vb = net.views_linears[0].bias.detach().cpu().double().numpy()
    f = net.feature_linear.weight.detach().cpu().double().numpy()
    fb = net.feature_linear.bias.detach().cpu().double().numpy()
    acc = np.zeros((v.shape[0], f.shape[1]))
    accb = vb.copy()
    for k in range(Wn):
        acc += v[:, k:k + 1] * f[k:k + 1, :]
        accb += v[:, k] * fb[k]
    t32 = lambda a: torch.from_numpy(a.astype(np.float32))
    return t32(acc), t32(v[:, Wn:]), t32(accb)


def operands(net, precision):
    """The operand weights of an inference trunk from the module's own weights, rounded with torch."""
    assert precision in DTYPE
    Ws, bs, extra = module_operands(net, precision)
    skips = [int(k) for k in net.skips]
    D = int(net.D)
    reads = [i == 0 or ((i - 1) in skips) for i in range(D)]
    L = (int(net.input_ch) - 3) // 6
    cpu = lambda t: t.cpu()
    Ws, bs = [cpu(w) for w in Ws], [cpu(b) for b in bs]
    if not net.use_viewdirs:
        return Operands(Ws, bs, tuple(cpu(t) for t in extra["output"]), None, None, None, reads, L, -1)
    LV = (int(net.input_ch_views) - 3) // 6
    w_hid, w_dir, b = folded_views(net)
    views = (round_to(w_dir, torch.float16), round_to(w_hid, DTYPE[precision]), b.double())
    return Operands(Ws, bs, None, tuple(cpu(t) for t in extra["alpha"]), views, tuple(cpu(t) for t in extra["rgb"]), reads, L, LV)


def r16(x, precision):
    """float64 -> the mode's 16-bit type through fp32, round to nearest even, as float64 (monotone)"""
    return x.to(torch.float32).to(DTYPE[precision]).double()


def _truncate16(x32, precision):
    """fp32 -> the 16-bit type, rounded TOWARD ZERO (the deliberately wrong conversion)"""
    if precision == "bf16":
        return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()
    h = x32.half()
    over = h.float().abs() > x32.abs()
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the network three times: exact, with the rounding points, and as another legitimate rounding
# ------------------------------------------------------------------------------------------------------------------------------------------
def exact64(net, pts, dirs=None):
    """The network in float64 with its fp32 weights and no rounding (run_nerf_helpers.py:272-306).  dirs [..., 3]: per point."""
    d64 = lambda t: t.detach().double().to(pts.device)
    skips = [int(k) for k in net.skips]
    enc = encoding64(pts, (int(net.input_ch) - 3) // 6)
    h = enc
    for i, l in enumerate(net.pts_linears):
        h = torch.relu(h @ d64(l.weight).T + d64(l.bias))
        if i in skips and i < len(net.pts_linears) - 1:
            h = torch.cat([enc, h], -1)
    if not net.use_viewdirs:
        return h @ d64(net.output_linear.weight).T + d64(net.output_linear.bias)
    alpha = h @ d64(net.alpha_linear.weight).T + d64(net.alpha_linear.bias)
    feat = h @ d64(net.feature_linear.weight).T + d64(net.feature_linear.bias)
    encv = encoding64(dirs, (int(net.input_ch_views) - 3) // 6)
    hv = torch.relu(torch.cat([feat, encv], -1) @ d64(net.views_linears[0].weight).T + d64(net.views_linears[0].bias))
    return torch.cat([hv @ d64(net.rgb_linear.weight).T + d64(net.rgb_linear.bias), alpha], -1)


def _run(ops, enc, encv, affine, store, layers=None):
    """The layer sequence on the encoding operand(s): affine(X, W, b, layer index) -> pre, store(pre) -> the next layer's input.
    layers: the hidden layers to evaluate (default: all)."""
    h = None
    for i in (range(len(ops.W)) if layers is None else layers):
        X = enc if i == 0 else (torch.cat([enc, h], -1) if ops.reads_enc[i] else h)
        h = store(affine(X, ops.W[i], ops.b[i], i))
    if ops.head is not None:
        return affine(h, ops.head[0], ops.head[1], "head")
    sigma = affine(h, ops.alpha[0], ops.alpha[1], "alpha")
    hv = store(affine(torch.cat([encv, h], -1), torch.cat([ops.views[0], ops.views[1]], 1), ops.views[2], "views"))
    return torch.cat([affine(hv, ops.rgb[0], ops.rgb[1], "rgb"), sigma], -1)


def _f16(x):
    return x.to(torch.float32).to(torch.float16).double()


def model64(net, pts, precision, dirs=None, ops=None, layers=None):
    """The network in float64 with the kernels' rounding points: operand weights and encoding rounded to the operand type, activations
    rounded to the 16-bit type after every hidden layer (round to nearest even), exact accumulation, unrounded head outputs."""
    ops = (ops or operands(net, precision)).to(pts.device)
    enc = _f16(encoding64(pts, ops.L))
    encv = _f16(encoding64(dirs, ops.LV)) if ops.views is not None else None
    return _run(ops, enc, encv, lambda X, W, b, i: X @ W.T + b, lambda pre: r16(torch.relu(pre), precision), layers)


def emulation(net, pts, precision, seed, dirs=None, rounding="nearest", garbage=None, drop_bias=None, ops=None):
    """A legitimate other rounding of the same model: fp32 accumulation in a seeded, permuted, chunked k order on top of the fp32 bias, the
    encoding perturbed before its f16 rounding by a seeded uniform draw within sincos_error_bound.  The deliberately WRONG variants of the
    self-test: rounding = "truncate" (activations rounded toward zero), garbage = (row, sample) (that sample's output replaced by another
    sample's), drop_bias = i (hidden layer i without its bias).  pts [N, S, 3]."""
    dev = pts.device
    ops = (ops or operands(net, precision)).to(dev)
    gen = torch.Generator().manual_seed(int(seed))
    draw = lambda shape: (torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1).to(dev)

    def encode(x, L):
        e = encoding64(x, L)
        return (e + draw(tuple(e.shape)) * sincos_error_bound(x, L)).to(torch.float32).to(torch.float16).float()

    def affine(X, W, b, i):
        K = X.shape[-1]
        perm = torch.randperm(K, generator=gen).to(dev)
        chunk = int(torch.randint(8, 65, (1,), generator=gen))
        acc = b.float().expand(*X.shape[:-1], -1).clone()
        if drop_bias is not None and i == drop_bias:
            acc.zero_()
        Xf, Wf = X.float(), W.float()
        for k0 in range(0, K, chunk):
            idx = perm[k0:k0 + chunk]
            acc = acc + Xf[..., idx] @ Wf[:, idx].T
        return acc

    def store(pre):
        h = torch.relu(pre)
        return (h.to(DTYPE[precision]) if rounding == "nearest" else _truncate16(h, precision)).float()

    assert rounding in ("nearest", "truncate")
    enc = encode(pts, ops.L)
    encv = encode(dirs, ops.LV) if ops.views is not None else None
    raw = _run(ops, enc, encv, affine, store).clone()
    if garbage is not None:
        row, sample = garbage
        N, S = raw.shape[0], raw.shape[1]
        other = ((row + 1) % N, (sample + S // 2) % S) if N * S > 1 else (row, sample)
        assert other != (row, sample), "no other sample to take the value from"
        raw[row, sample] = raw[other]
    return raw


# ------------------------------------------------------------------------------------------------------------------------------------------
# sandwich networks: the real architecture, every hidden layer the identity except layer 0 and at most one more
# ------------------------------------------------------------------------------------------------------------------------------------------
def live_sets(depth, skips):
    """{0}, {0, 1}, {0, the layer behind the skip}, {0, the last hidden layer}; each once"""
    sets = [(0,), (0, 1)]
    for k in skips:
        if 0 <= k < depth - 1 and (0, k + 1) not in sets:
            sets.append((0, k + 1))
    if (0, depth - 1) not in sets:
        sets.append((0, depth - 1))
    return sets


def sandwich_arrays(arrays, cfg, live):
    """The network's named arrays with every hidden layer outside ``live`` set to W = I (zero on the encoding columns behind the skip),
    b = 0: such a layer passes a non-negative 16-bit activation through exactly -- products, sum, relu and conversion are all exact."""
    out = {k: v.clone() for k, v in arrays.items()}
    W, n_enc = cfg.netwidth, cfg.input_ch
    assert 0 in live and len(live) <= 2
    for i in range(1, cfg.netdepth):
        if i in live:
            continue
        w = torch.zeros_like(out[f"pts_linears.{i}.weight"])
        w[:, -W:] = torch.eye(W)
        assert w.shape[1] in (W, W + n_enc)
        out[f"pts_linears.{i}.weight"] = w
        out[f"pts_linears.{i}.bias"] = torch.zeros_like(out[f"pts_linears.{i}.bias"])
    return out


def _interval(pre, B, precision):
    """rounding and relu are monotone: the kernel's stored value lies between the images of the ends"""
    return r16(torch.relu(pre - B), precision), r16(torch.relu(pre + B), precision)


def interval_bound(net, live, pts, precision, ops=None):
    """For a sandwich network, per element of raw the float64 centre and an a-priori radius the kernel's value must lie within.
    Layer 0: pre = op W^T + b, B = (K + 3) U32 A + delta |W_enc|^T (layer64); the output lies in [r16(relu(pre - B)), r16(relu(pre + B))].
    Identity layers pass the interval through unchanged.  The second live layer: centre c and radius rho of the interval, pre = c W^T + b,
    B = rho |W|^T + (K + 3) U32 A with A from the interval's upper end (+ the encoding term behind the skip); the interval of r16(relu(.))
    again.  The head: raw in pre +- B, and the fp32 store adds one U32 |raw|."""
    assert not net.use_viewdirs, "sandwiches have a plain head"
    ops = (ops or operands(net, precision)).to(pts.device)
    n_enc = 3 + 6 * ops.L
    op, delta = encoding_operand(pts, ops.L, True, clamp=False)
    pre, A, B = layer64(op, ops.W[0], ops.b[0], delta)
    lo, hi = _interval(pre, B, precision)

    def stage(W, b, with_enc):
        c, rho = (lo + hi) / 2, (hi - lo) / 2
        Wh = W[:, n_enc:] if with_enc else W
        X = torch.cat([op, c], -1) if with_enc else c
        Xhi = torch.cat([op, hi], -1) if with_enc else hi
        pre = X @ W.T + b
        A = Xhi.abs() @ W.abs().T + b.abs()
        B = rho @ Wh.abs().T + (X.shape[-1] + 3) * U32 * A
        if with_enc:
            B = B + delta @ W[:, :n_enc].abs().T
        return pre, B
    for i in live[1:]:
        pre, B = stage(ops.W[i], ops.b[i], ops.reads_enc[i])
        lo, hi = _interval(pre, B, precision)
    pre, B = stage(ops.head[0], ops.head[1], False)
    return pre, B + U32 * (pre.abs() + B)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the acceptance functions
# ------------------------------------------------------------------------------------------------------------------------------------------
RADIUS_CAP = 0.1            # per channel: median radius <= a tenth of the channel's standard deviation over the case's points
RMS_FACTOR, MAX_FACTOR = 1.3, 3.0      # mean within 30 %, maximum within 3 x (the rule of tests/test_gpu_parity.py), against the emulations


def radius_cap_failures(centre, radius):
    """per output channel, median radius / std of the centre; the channels over RADIUS_CAP"""
    c, r = centre.reshape(-1, centre.shape[-1]), radius.reshape(-1, radius.shape[-1])
    share = r.median(0).values / c.std(0)
    return [f"channel {k}: median radius {float(r.median(0).values[k]):.3g} is {float(share[k]):.3g} of the channel's std"
            for k in range(c.shape[-1]) if not float(share[k]) <= RADIUS_CAP], float(share.max())


def interval_failures(raw, centre, radius):
    """(the elements outside centre +- radius as text, worst residual / radius) -- no share of elements excused"""
    res = (raw.double() - centre).abs()
    bad = ~(res <= radius)
    ratio = torch.where(radius > 0, res / radius.clamp_min(1e-300), torch.where(res > 0, torch.full_like(res, float("inf")), torch.zeros_like(res)))
    worst = float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0
    fails = []
    if bool(bad.any()):
        idx = [tuple(int(v) for v in i) for i in bad.nonzero()[:4]]
        fails.append(f"{int(bad.sum())} of {bad.numel()} elements outside the bound (worst residual / bound {worst:.3g}), first at {idx}")
    return fails, worst


def rule_ratios(raw, model, emus):
    """per channel rms(raw - model) / max_k rms(emu_k - model) and max |raw - model| / max_k max |emu_k - model|: (worst rms ratio, worst
    max ratio)"""
    C_ = model.shape[-1]
    d = (raw.double() - model).reshape(-1, C_)
    de = [(e.double() - model).reshape(-1, C_) for e in emus]
    rms_ref = torch.stack([x.pow(2).mean(0).sqrt() for x in de]).max(0).values
    max_ref = torch.stack([x.abs().max(0).values for x in de]).max(0).values
    rms = torch.nan_to_num(d.pow(2).mean(0).sqrt() / rms_ref, nan=float("inf"))
    mx = torch.nan_to_num(d.abs().max(0).values / max_ref, nan=float("inf"))
    return float(rms.max()), float(mx.max())


def rule_failures(raw, model, emus):
    """rms(d(raw)) <= 1.3 max_k rms(d(emu_k)) and max |d(raw)| <= 3 max_k max |d(emu_k)| per channel, d(x) = x - model64"""
    rms, mx = rule_ratios(raw, model, emus)
    fails = []
    if not rms <= RMS_FACTOR:
        fails.append(f"rms deviation from the model is {rms:.3g} x the emulations' largest (cap {RMS_FACTOR})")
    if not mx <= MAX_FACTOR:
        fails.append(f"max deviation from the model is {mx:.3g} x the emulations' largest (cap {MAX_FACTOR})")
    return fails, rms, mx


def budget_share(raw, model, exact):
    """rms(raw - exact64) / rms(model64 - exact64), worst channel: how much of the rounding design's error budget the kernel uses"""
    C_ = model.shape[-1]
    a = (raw.double() - exact).reshape(-1, C_).pow(2).mean(0).sqrt()
    b = (model - exact).reshape(-1, C_).pow(2).mean(0).sqrt()
    return float((a / b).max())


# ------------------------------------------------------------------------------------------------------------------------------------------
# the cases, shared by the host tests and the GPU tests
# ------------------------------------------------------------------------------------------------------------------------------------------
# family -> (SceneConfig arguments, RENDER_NO_X16, the name plan_query gives the network step, nrnerf_pack_host image, decoder)
FAMILIES = {
    "x16_w256":   (dict(), False, "net_kernel_x16", 10, "x16"),
    "x16_w128":   (dict(netwidth=128), False, "net_kernel_x16", 10, "x16"),
    "trunk_w256": (dict(), True, "net_kernel (trunk only)", 2, "mb"),
    "trunk_w128": (dict(netwidth=128), True, "net_kernel (trunk only)", 2, "mb"),
    "net_w256":   (dict(ray_bending=False), False, "net_kernel", 0, "mb"),
    "gx_d6_w192": (dict(netdepth=6, netwidth=192, multires=8), False, "gx16_kernel", 11, "gx"),
    "gx_d3_w448": (dict(netdepth=3, netwidth=448, skips=()), False, "gx16_kernel", 11, "gx"),
    "gx_d5_w96":  (dict(netdepth=5, netwidth=96, skips=(1,)), False, "gx16_kernel", 11, "gx"),
    "gen_d6_w192": (dict(netdepth=6, netwidth=192, multires=8), True, "gen_kernel", 7, "gen"),
}
VIEWS_FAMILY = ("views_w256", (dict(ray_bending=False, use_viewdirs=True), False, "net_kernel (a record per point)", 0, "mb"))
PRECISIONS = ("bf16", "f16")
SANDWICH_SHAPES = [(1, 1), (3, 5), (37, 33), (5, 85), (2, 1024)]
FULL_SHAPES = [(37, 33), (19, 70)]
SCENE_SEED = 3
EMULATION_SEEDS = (11, 12, 13, 14, 15)


def family_config(family):
    from nonrigid_nerf_amd.synthetic import SceneConfig
    kw = VIEWS_FAMILY[1][0] if family == VIEWS_FAMILY[0] else FAMILIES[family][0]
    return SceneConfig(N_importance=0, **kw)


def family_scene(family, live=None):
    """The stress scene of a family (its real bender, if it has one); live: the sandwich of its coarse network."""
    from nonrigid_nerf_amd.synthetic import Scene, make_scene
    cfg = family_config(family)
    scene = make_scene(cfg, SCENE_SEED)
    if live is not None:
        scene = Scene(cfg, scene.bender, sandwich_arrays(scene.coarse, cfg, live), None)
    return cfg, scene


POINT_SEED = 1         # (with seed 0 the single point of the (1, 1) case sat where one family's radius is 0.105 of the channel's spread)


def case_points(shape, seed=POINT_SEED):
    """The caller's points of a case: [N, S, 3] fp32 in the volume the scenes are calibrated on."""
    n, s = shape
    g = torch.Generator().manual_seed(1000 * n + s + seed)
    return (torch.rand(n, s, 3, generator=g) * 2 - 1) * 0.9


def case_dirs(shape, seed=0):
    n, s = shape
    g = torch.Generator().manual_seed(77 * n + s + seed)
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)


def case_latents(shape, latent_size, seed=0):
    g = torch.Generator().manual_seed(31 * shape[0] + seed)
    return torch.randn(shape[0], latent_size, generator=g) * 0.1
