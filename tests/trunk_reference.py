"""A float64 reference of ONE trunk layer at a time, for the training kernels (csrc/nrnerf_train.h, nrnerf_generic.h, nrnerf_gx16*.h).

The training kernels save, per layer, exactly the values they feed the next layer (``store_tile_bf16`` writes the B-operand fragment
``pack_tile`` produced; ``mask_store`` does the same for d z).  So a layer can be checked on its own: take the kernel's OWN saved input
to the layer (exact in float64), the weights the kernel multiplies by (the packed images, decoded here), form the product in float64 and
compare the kernel's saved output with an a-priori rounding bound.  Nothing drifts through the layers and nothing is excused.

Plain torch / numpy; no kernels; imports without a GPU.  Three parts:

* decoders of the saved arrays (bf16 block tiles, relu records, row-major arrays),
* the operand weights: the packed forward / backward images of ``nrnerf_pack_host`` probed with one-hot inputs through the register
  dataflow emulation of tests/test_packing.py (which proves those images reproduce the network), or -- generic architectures -- the
  module's weights rounded with torch (tests/test_trunk_reference_host.py: value for value what the width-class image holds),
* the float64 layer products and the bounds.

Unit roundoffs: U32 = 2^-24 (fp32), U16 = 2^-8 (bf16, round to nearest even), UH = 2^-11 (f16).  An fp32 accumulation of K products and
a bias in any order is off by at most (K + 3) U32 A, A = |x| |w|^T + |b| (products of two bf16 / two f16 values are exact in fp32; fp32
products carry one rounding each, which the K + 3 of the any-order bound gamma_(K+1) still covers).
"""
import ctypes as C
import dataclasses

import numpy as np
import torch

U32, U16, UH = 2.0 ** -24, 2.0 ** -8, 2.0 ** -11
EPS_SC = 1e-4               # the hardware sine path's stated bound (enc_sincos, csrc/nrnerf_net_impl.h)
EPS_HW = 2.0 ** -18         # v_sin_f32 / v_cos_f32 on a reduced argument (sincos_error_bound)
UNDECIDED_CAP = 1e-3        # share of relu elements with |pre| <= B the bit check may skip, per layer


# ------------------------------------------------------------------------------------------------------------------------
# decoders of the saved arrays
# ------------------------------------------------------------------------------------------------------------------------
def tile_feature(t, h, r):
    """Feature of accumulator register r of tile t in lane half h (store_half_bf16 / keep, csrc/nrnerf_train.h)."""
    return 32 * t + 4 * h + (r & 3) + 8 * (r >> 2)


def tiles_to_rows(tiles, n_rays, S):
    """Block tiles [..., B, F, 32 samples] (B = n_rays * ceil(S / 32)) -> rows [..., n_rays, S, F] and the padded columns
    [..., n_rays, 32 ceil(S / 32) - S, F] (the samples beyond a ray's end)."""
    bpr = (S + 31) // 32
    lead, (B, F, w) = tuple(tiles.shape[:-3]), tiles.shape[-3:]
    assert B == n_rays * bpr and w == 32, (tuple(tiles.shape), n_rays, S)
    x = tiles.reshape(*lead, n_rays, bpr, F, 32).transpose(-1, -2).reshape(*lead, n_rays, bpr * 32, F)
    return x[..., :S, :], x[..., S:, :]


def relu_records_to_bool(rec, n_rays, S):
    """Relu records [..., B, 64 lanes, NT] (16 bits per lane and tile: relu_mask with NT = W / 32, hv_mask with NT = W / 64) -> bool
    rows [..., n_rays, S, 32 NT] and the padded columns.  Lane 32 h + j holds sample j of the block, bit r of tile t is feature
    tile_feature(t, h, r)."""
    NT = int(rec.shape[-1])
    lead, B = tuple(rec.shape[:-3]), int(rec.shape[-3])
    bpr = (S + 31) // 32
    assert B == n_rays * bpr and rec.shape[-2] == 64
    m = rec.to(torch.int32) & 0xffff
    r = torch.arange(16, device=rec.device, dtype=torch.int32)
    bits = ((m.unsqueeze(-1) >> r) & 1).bool()                                           # [..., B, 64, NT, 16]
    bits = bits.reshape(*lead, B, 2, 32, NT, 16).transpose(-4, -3).reshape(*lead, B, 32, 2 * NT * 16)      # [..., B, j, (h, t, r)]
    inv = torch.empty(32 * NT, dtype=torch.long)
    for h in range(2):
        for t in range(NT):
            for q in range(16):
                inv[tile_feature(t, h, q)] = (h * NT + t) * 16 + q
    rows = bits[..., inv.to(rec.device)].reshape(*lead, n_rays, bpr * 32, 32 * NT)
    return rows[..., :S, :], rows[..., S:, :]


def rowmajor_to_rows(arr, n_rays, S):
    """fp32 mode and the generic entry points: [slots][M][width] -> [slots][n_rays][S][width] (no padding)."""
    return arr.reshape(arr.shape[0], n_rays, S, arr.shape[-1])


# ------------------------------------------------------------------------------------------------------------------------
# the encoding in float64
# ------------------------------------------------------------------------------------------------------------------------
def encoding64(x, L):
    """Embedder.embed of fp32 3-vectors in float64, reference column order [x, sin(2^0 x), cos(2^0 x), ...]."""
    x = x.double()
    cols = [x]
    for k in range(L):
        cols += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(cols, -1)


def sincos_error_bound(x, L):
    """How far the hardware path's sin / cos (enc_sincos: rev = fl(x fl(1 / 2 pi)), scaled by the exact 2^f, v_fract, v_sin_f32 / v_cos_f32)
    can be from the true value, per column of the encoding.  The one rounded product carries a relative error of at most 2 U32 (the
    constant's rounding and the product's), which the exact scaling and the exact v_fract pass on: at most 2 pi 2 U32 |x / 2 pi| 2^f =
    2 U32 2^f |x| radians, taken as 3 U32 2^f |x|; the instruction itself, an fp32 transcendental on an argument in [0, 1), is given
    EPS_HW = 2^-18 (32 fp32 ulps at 1).  That is the frequency dependence behind the project's "<= ~1e-4 at the highest frequency", and
    it is never taken above EPS_SC, the issue's flat figure.  Zero on the identity columns."""
    x = x.double().abs()
    cols = [torch.zeros_like(x)]
    for f in range(L):
        e = (EPS_HW + 3 * U32 * 2.0 ** f * x).clamp_max(EPS_SC)
        cols += [e, e]
    return torch.cat(cols, -1)


def encoding_operand(x, L, sixteen_bit, clamp=True):
    """The operand the reference multiplies by -- f16(enc64), enc64 the float64 encoding of the fp32 3-vectors x -- and how far the kernel's
    may be from it, per element.  16-bit modes: the kernel's sin / cos is an fp32 value hw within eps = sincos_error_bound of enc64, rounded to
    f16; rounding is monotone, so its operand lies in [f16(enc64 - eps), f16(enc64 + eps)]: where both ends ARE the reference's operand the
    allowance is zero, else the distance to the farther end -- never more than the issue's UH |e| + EPS_SC.  The identity columns are f16 of
    the same fp32 value on both sides: zero (the issue allows one f16 neighbour).  fp32 mode: sincosf of the exact fp32 product,
    4 U32 max(|e|, 1); the identity columns are exact.  clamp=False leaves the issue's figure out: it is half an f16 ulp of e plus EPS_SC, and
    where the two roundings differ they differ by a WHOLE ulp -- more than that figure for |e| in the lower part of a binade -- so a bound
    that must hold for every element (tests/inference_reference.py interval_bound) takes the distance to the farther end as it is."""
    e64 = encoding64(x, L)
    if sixteen_bit:
        f16 = lambda t: t.to(torch.float32).to(torch.float16).double()
        op, eps = f16(e64), sincos_error_bound(x, L)
        delta = torch.maximum(f16(e64 + eps) - op, op - f16(e64 - eps))
        if clamp:
            delta = delta.clamp_max(UH * e64.abs() + EPS_SC)
        delta[..., :3] = 0.0
    else:
        op = e64.to(torch.float32).double()
        delta = 4 * U32 * e64.abs().clamp_min(1.0)
        delta[..., :3] = 0.0
    return op, delta


# ------------------------------------------------------------------------------------------------------------------------
# one layer in float64, and the bounds
# ------------------------------------------------------------------------------------------------------------------------
def layer64(X, Wq, b=None, delta=None, extra=None):
    """pre64 = X Wq^T + b (+ extra), A = |X| |Wq|^T + |b| (+ |extra|), B = (K + 3 (+ 1)) U32 A (+ delta |Wq[:, :n_enc]|^T): X [M, K] the
    kernel's saved input (exact), Wq [O, K] the operand weights, delta [M, n_enc] the allowance on the leading (encoding) columns,
    extra [M, O] a second fp32 addend (the per-ray bias)."""
    X, Wq = X.double(), Wq.double()
    pre = X @ Wq.T
    A = X.abs() @ Wq.abs().T
    K = X.shape[-1]
    if b is not None:
        pre, A = pre + b.double(), A + b.double().abs()
    if extra is not None:
        pre, A, K = pre + extra.double(), A + extra.double().abs(), K + 1
    B = (K + 3) * U32 * A
    if delta is not None:
        B = B + delta.double() @ Wq[:, :delta.shape[-1]].abs().T
    return pre, A, B


def _ratio(res, bound):
    """max residual / bound (inf where a residual meets a zero bound)"""
    r = torch.where(bound > 0, res / bound.clamp_min(1e-300), torch.where(res > 0, torch.full_like(res, float("inf")), torch.zeros_like(res)))
    return float(r.max()) if r.numel() else 0.0


def hidden_ratio(stored, pre, B, sixteen_bit, bit=None):
    """Worst |stored - relu(pre64)| / bound of a forward hidden layer (bit = None), or |stored - bit * pre64| / bound of a backward one:
    bound = U16 |pre64| + (1 + U16) B for a bf16 store, B for an fp32 one."""
    want = torch.relu(pre) if bit is None else torch.where(bit, pre, torch.zeros_like(pre))
    bound = U16 * pre.abs() + (1 + U16) * B if sixteen_bit else B
    return _ratio((stored.double() - want).abs(), bound)


def linear_ratio(stored, pre, B):
    """Worst |stored - pre64| / B of an fp32 output without relu (heads, encoding gradients)."""
    return _ratio((stored.double() - pre).abs(), B)


def relu_bit_check(bit, pre, B, stored=None):
    """(share of undecided elements, number of wrong bits, number of elements): bit == (pre64 > 0) wherever |pre64| > B -- the elements
    with |pre64| <= B are undecided, the only ones skipped, and only by this comparison -- and bit == (stored > 0) on EVERY element (it
    needs no reference)."""
    decided = pre.abs() > B
    wrong = decided & (bit != (pre > 0))
    if stored is not None:
        wrong = wrong | (bit != (stored > 0))
    return float((~decided).double().mean()), int(wrong.sum()), pre.numel()


def encoding_backward64(x, denc, B_enc, L, eps_sc):
    """The gradient wrt 3-vectors x from the gradient of their encoding (reference column order) through the float64 Jacobian, and its
    bound: each term 2^f (cos d_sin - sin d_cos) carries 2^f ((|d_sin| + |d_cos|) eps_sc + B_sin + B_cos); the fp32 sum of the terms and
    the cross-half add (2 L + 3) U32 sum |terms|."""
    x = x.double()
    g = denc[..., :3].clone()
    mag = denc[..., :3].abs()
    bound = B_enc[..., :3].clone()
    for f in range(L):
        s, c = torch.sin(x * 2.0 ** f), torch.cos(x * 2.0 ** f)
        ds, dc = denc[..., 3 + 6 * f:6 + 6 * f], denc[..., 6 + 6 * f:9 + 6 * f]
        g = g + 2.0 ** f * (c * ds - s * dc)
        mag = mag + 2.0 ** f * ((c * ds).abs() + (s * dc).abs())
        bound = bound + 2.0 ** f * ((ds.abs() + dc.abs()) * eps_sc + B_enc[..., 3 + 6 * f:6 + 6 * f] + B_enc[..., 6 + 6 * f:9 + 6 * f])
    return g, bound + (2 * L + 3) * U32 * mag


# ------------------------------------------------------------------------------------------------------------------------
# operand weights of the compiled kernels: the packed images, probed with one-hot inputs
# ------------------------------------------------------------------------------------------------------------------------
def enc_slot_col(L, hh, q):
    """Encoding slot q of lane half hh -> reference column, or -1 (nrnerf_plan.h enc_col; tests/test_packing.py)."""
    F0 = (L + 1) // 2
    if q == 0:
        return 2 if hh else 0
    if q == 1:
        return -1 if hh else 1
    pi, fn = (q - 2) // 2, (q - 2) % 2
    fl, c = pi // 3, pi % 3
    return 3 + 6 * (hh * F0 + fl) + 3 * fn + c if (fl < F0 and hh * F0 + fl < L) else -1


def _pack_image(coarse, fine, precision, which, with_units=False):
    from nonrigid_nerf_amd import _lib
    from nonrigid_nerf_amd.render import build_model_desc
    desc, keep = build_model_desc(coarse, fine, precision, 0)
    lib = _lib.load()
    info = _lib.PackedInfo()
    _lib.check(lib.nrnerf_pack_host(C.byref(desc), which, C.byref(info), None, 0, C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)()), "size query")
    stream = np.zeros(info.stream_bytes, dtype=np.uint8)
    units = np.zeros(info.n_units + 1, dtype=np.uint32)
    bias = np.zeros(info.n_bias_tiles * 32, dtype=np.float32)
    _lib.check(lib.nrnerf_pack_host(C.byref(desc), which, C.byref(info), stream.ctypes.data_as(C.c_void_p), stream.nbytes,
                                    units.ctypes.data_as(C.POINTER(C.c_uint32)), bias.ctypes.data_as(C.POINTER(C.c_float))), "pack")
    return (info, stream, bias, units) if with_units else (info, stream, bias)


class _Prober:
    """Reads one layer after the other off a packed image: the layer's weight matrix [32 nt, K] (true feature rows; columns in the
    order of the input groups) and bias, by running tests/test_packing.py's emulation of the kernel's register dataflow on one-hot inputs."""

    def __init__(self, info, stream, bias, precision):
        from tests.test_packing import FragReader
        self.fr = FragReader(stream, precision, info.frag_bytes)
        self.KH = 1 if precision == "f32" else 8
        self.bias, self.tile0, self.info = bias, 0, info

    def layer(self, nt, groups):
        """groups: [("enc", L) | ("vec16", n) | ("vec", n) | ("hid", n)], the f16 ones (encodings, latent columns: vec16) first"""
        from tests.test_packing import dense_emul, repack, tile_row, vec_slabs
        KH = self.KH
        K = sum((3 + 6 * n) if kind == "enc" else n for kind, n in groups)
        slabs, off, n16 = [], 0, 0
        for kind, n in groups:
            if kind == "enc":
                F0 = (n + 1) // 2
                nslot = -(-(2 + 6 * F0) // KH) * KH
                for s in range(nslot // KH):
                    sl = np.zeros((2 * KH, K))
                    for h in range(2):
                        for e in range(KH):
                            col = enc_slot_col(n, h, s * KH + e)
                            if col >= 0:
                                sl[KH * h + e, off + col] = 1.0
                    slabs.append(sl)
                off += 3 + 6 * n
                n16 = len(slabs)
            elif kind in ("vec", "vec16"):
                v = np.zeros((n, K))
                v[np.arange(n), off + np.arange(n)] = 1.0
                slabs += vec_slabs(v, KH, lambda x: x)
                off += n
                if kind == "vec16":
                    n16 = len(slabs)
            else:
                tiles = []
                for t in range(n // 32):
                    D = np.zeros((32, K))
                    D[np.arange(32), off + 32 * t + np.arange(32)] = 1.0
                    tiles.append(D)
                slabs += repack(tiles, KH, False)
                off += n
        out = dense_emul(self.fr, np.zeros_like(self.bias), self.tile0, len(slabs), nt, slabs, f16_slabs=n16)
        b = np.zeros(32 * nt)
        for t in range(nt):
            for h in range(2):
                for r in range(16):
                    b[32 * t + tile_row(r, h)] = self.bias[(self.tile0 + t) * 32 + h * 16 + r]
        self.tile0 += nt
        return np.concatenate(out, 0), b

    def done(self):
        used = self.fr.pos * self.info.frag_bytes
        assert self.tile0 == self.info.n_bias_tiles and used <= self.info.stream_bytes, "the image holds other layers than the probe read"


def _slots_to_cols(Wt, L, n_tiles):
    """Rows of an encoding-gradient block in slot order ([32 n_tiles, K]) -> reference column order [3 + 6 L, K]."""
    from tests.test_packing import tile_row
    out = np.zeros((3 + 6 * L, Wt.shape[1]))
    for te in range(n_tiles):
        for hh in range(2):
            for r in range(16):
                col = enc_slot_col(L, hh, te * 16 + r)
                row = Wt[32 * te + tile_row(r, hh)]
                if col >= 0:
                    out[col] = row
                else:
                    assert not row.any(), "a slot without a column carries no weight"
    return out


@dataclasses.dataclass
class CompiledOperands:
    """What the compiled training kernels multiply by, float64 tensors.  Forward: W[i] [W, K_i] (columns [encoding | hidden] for layer 0
    and skip + 1), b[i]; head [5 | -, W]; view-dependent head: alpha, views (columns [direction encoding | hidden], the FOLDED layer), rgb.
    Backward (transposed images, bf16 throughout): head_t [W, 8] (columns = d raw channels), hid_t[i] [W, W] (d h_(i-1) = d z_i hid_t[i]^T,
    i >= 1), enc_t {0, skip + 1} [3 + 6 L, W]; views: rgb_t [W / 2, 8], join_t [W, 8 + W / 2], encv_t [3 + 6 LV, 8 + W / 2]."""
    W: list
    b: list
    head: tuple
    alpha: tuple
    views: tuple
    rgb: tuple
    head_t: object
    hid_t: dict
    enc_t: dict
    rgb_t: object
    join_t: object
    encv_t: object
    depth: int
    width: int
    skip: int
    L: int
    LV: int


def probe_forward_image(image, precision, D, Wd, L, LV, skip, views, latent=0):
    """The forward layers of a 32x32 trunk image (nrnerf_pack_host which = 0 | 1, or 2: the trunk half of a split image), probed layer by
    layer: (W [D], b [D], head | None, alpha, views (the FOLDED layer, columns [direction encoding | hidden]), rgb | None), float64.
    latent > 0 (time-conditioned baseline): the latent columns behind the encoding are probed and left out."""
    NT, n_enc = Wd // 32, 3 + 6 * L
    lat = [("vec16", latent)] if latent else []
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    pr = _Prober(*image, precision)
    Ws, bs = [], []
    for i in range(D):
        groups = ([("enc", L)] + lat if (i == 0 or i - 1 == skip) else []) + ([("hid", Wd)] if i > 0 else [])
        Wm, b = pr.layer(NT, groups)
        if latent and (i == 0 or i - 1 == skip):     # the latent columns reach the training kernels through ray_bias
            Wm = np.concatenate([Wm[:, :n_enc], Wm[:, n_enc + latent:]], 1)
        Ws.append(t64(Wm)); bs.append(t64(b))
    head = alpha = vw = rgb = None
    if views:
        Wm, b = pr.layer(1, [("hid", Wd)])
        alpha = (t64(Wm[:1]), t64(b[:1]))
        Wm, b = pr.layer(NT // 2, [("enc", LV), ("hid", Wd)])
        vw = (t64(Wm), t64(b))
        Wm, b = pr.layer(1, [("hid", Wd // 2)])
        rgb = (t64(Wm[:3]), t64(b[:3]))
    else:
        Wm, b = pr.layer(1, [("hid", Wd)])
        rows = [0, 1, 2, 3, 8]                    # accumulator registers 0..4 of the lower lane half (tile_row(r, 0))
        head = (t64(Wm[rows]), t64(b[rows]))
    pr.done()
    return Ws, bs, head, alpha, vw, rgb


def frag16_image_operands(image, precision, W, D, L, skip, layout):
    """The weight matrices and biases of a plain-headed trunk image of the 16x16x32 kernels, read fragment by fragment in the order
    tests/test_packing.py consumes them (test_x16_stream_reproduces_the_trunk, test_width_class_stream_reproduces_any_plain_trunk): a fragment
    is W[16 rows][32 positions], lane (r, g) holding positions 8 g .. 8 g + 7; tiles in pairs with their k-steps interleaved, an odd last tile
    alone; encoding k-steps f16, hidden k-step s position 8 g + e = feature 32 s + 4 g + e (e < 4) or 32 s + 16 + 4 g + e - 4.
    layout "gx" (nrnerf_pack_host which = 11 | 12, csrc/nrnerf_gx16.h): the width padded to a multiple of 64, every layer padded to whole
    4-unit ring periods, encoding positions [x, y, z, -, (sin, cos) pairs]; layout "x16" (which = 10, csrc/nrnerf_net_x16.h): the layers back
    to back, the encoding in the slots of nrnerf_plan.h x16_enc_col.  -> ([(W [16 nt, n_enc (if read) + WC], bias [16 nt])] per layer, head)."""
    info, stream, bias = image[:3]
    gx = layout == "gx"
    WC = (W + 63) // 64 * 64 if gx else W
    n_enc = 3 + 6 * L
    as_bf16 = (stream.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    as_f16 = stream.view(np.float16).astype(np.float64)
    pos, tile = [0], [0]
    if gx:
        def enc_col(q):
            if q < 3:
                return q
            if q == 3:
                return -1
            m, b = (q - 4) // 2, (q - 4) & 1
            return 3 + 6 * (m // 3) + 3 * b + (m % 3) if m < 3 * L else -1
    else:
        from tests.test_packing import _x16_enc_col
        enc_col = lambda q: _x16_enc_col(L, q // 32, (q % 32) // 8, q % 8)

    def hid_col(q):
        s, g, e = q // 32, (q % 32) // 8, q % 8
        return 32 * s + 4 * g + e if e < 4 else 32 * s + 16 + 4 * g + e - 4
    enc_cols = [enc_col(q) for q in range(64)]
    hid_cols = [hid_col(q) for q in range(WC)]

    def layer(nt, n_enc_steps, n_hid_steps):
        start, ns = pos[0], n_enc_steps + n_hid_steps
        lead = n_enc if n_enc_steps else 0
        out = np.zeros((16 * nt, lead + (WC if n_hid_steps else 0)))

        def take(t, s):
            f16 = s < n_enc_steps
            f = (as_f16 if (f16 or precision == "f16") else as_bf16)[pos[0] * 512:(pos[0] + 1) * 512].reshape(64, 8)
            pos[0] += 1
            for g in range(4):
                for e in range(8):
                    c = enc_cols[32 * s + 8 * g + e] if f16 else lead + hid_cols[32 * (s - n_enc_steps) + 8 * g + e]
                    col = f[16 * g:16 * g + 16, e]
                    if c >= 0:
                        out[16 * t:16 * t + 16, c] = col
                    else:
                        assert not col.any(), "a position without a column carries no weight"
        for p_ in range(0, nt - 1, 2):
            for s in range(ns):
                take(p_, s)
                take(p_ + 1, s)
        if nt & 1:
            for s in range(ns):
                take(nt - 1, s)
        b = bias[tile[0] * 16:(tile[0] + nt) * 16].astype(np.float64)
        tile[0] += nt
        if gx:
            units = -(-(pos[0] - start) // 16)
            pos[0] = start + (-(-units // 4) * 4) * 16
        return torch.from_numpy(out), torch.from_numpy(b)

    NT = WC // 16
    layers = [layer(NT, 2, 0)]
    for i in range(1, D):
        layers.append(layer(NT, 2 if i - 1 == skip else 0, WC // 32))
    head = layer(1, 0, WC // 32)
    assert tile[0] == info.n_bias_tiles, "the image holds other layers than were read"
    if not gx:
        assert pos[0] * 1024 <= info.stream_bytes and not stream[pos[0] * 1024:].any(), "the stream goes on behind the head"
    return layers, head


def generic_program_operands(image, precision):
    """The layers of a run-time-parameterised kernel's program (nrnerf_pack_host which = 7 | 8, csrc/nrnerf_generic.h), decoded as
    tests/test_packing.py::_run_generic_program walks them: per layer dict(W = {source buffer: [32 nt, positions]}, b [32 nt], relu, dst,
    o_col, o_rows); buffers 0 = E (the encoding in reference column order [, latent]), 1 = H (hidden), 2 = V (direction encoding); fragments
    against E / V are f16.  16-bit modes only."""
    from tests.test_packing import tile_row
    info, stream, bias, units = image
    assert info.frag_bytes == 1024 and precision in ("bf16", "f16")
    u = units.astype(np.int64)
    n_layers = int(u[0])
    prog = u[1:1 + 11 * n_layers].reshape(n_layers, 11)
    raw16 = stream.view(np.uint16)
    rows = np.array([tile_row(r, h) for h in range(2) for r in range(16)])
    out = []
    for (w_frag, bias_tile, nt, src0, ns0, src1, ns1, dst, relu, o_col, o_rows) in prog:
        ns = int(ns0 + ns1)
        mats = {}
        b = np.zeros(32 * nt)
        for t in range(int(nt)):
            b[32 * t + rows] = bias[(bias_tile + t) * 32:(bias_tile + t) * 32 + 32]
            for sl in range(ns):
                src, s = (int(src0), sl) if sl < ns0 else (int(src1), sl - int(ns0))
                fi = int(w_frag) + t * ns + sl
                bits = raw16[fi * 512:(fi + 1) * 512].reshape(64, 8)
                as_f16 = precision == "f16" or src != 1
                fr = bits.view(np.float16).astype(np.float64) if as_f16 else (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
                M = mats.setdefault(src, np.zeros((32 * int(nt), 16 * int(ns0 if sl < ns0 else ns1))))
                for h in range(2):
                    M[32 * t:32 * t + 32, 16 * s + 8 * h:16 * s + 8 * h + 8] = fr[32 * h:32 * h + 32]
        out.append(dict(W={k: torch.from_numpy(v) for k, v in mats.items()}, b=torch.from_numpy(b), relu=bool(relu), dst=int(dst),
                        o_col=int(o_col), o_rows=int(o_rows)))
    return out


def compiled_operands(scene, which, precision):
    """The operand weights of nrnerf_trunk_forward / _backward for ``scene``'s coarse (which = 0) or fine (1) network, from the packed
    images (nrnerf_pack_host which = 0 | 1 forward, 4 | 5 backward-data) of the same networks WITHOUT the ray bender: the trunk-only image
    the training kernels stream (tests/test_packing.py: the split images are the two halves of the fused stream, byte for byte)."""
    from nonrigid_nerf_amd.synthetic import Scene, build_modules
    cfg = scene.cfg
    _, coarse, fine = build_modules(Scene(cfg, None, scene.coarse, scene.fine))
    views, tcb = cfg.use_viewdirs, cfg.time_conditioned_baseline
    fcfg = cfg.for_fine() if which == 1 else cfg
    Wd, D, L, LV, skip = fcfg.netwidth, fcfg.netdepth, cfg.multires, cfg.multires_views, cfg.skips[0]
    NT, n_enc = Wd // 32, 3 + 6 * cfg.multires
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    Ws, bs, head, alpha, vw, rgb = probe_forward_image(_pack_image(coarse, fine, precision, which), precision, D, Wd, L, LV, skip, views,
                                                       cfg.latent_size if tcb else 0)
    # backward-data: head^T (view-dependent: rgb_linear^T, then the joined layer), pts_linears[D-1 .. 1]^T, pts_linears[0]^T
    if tcb:
        # nrnerf_pack_host hands out no backward image of the time-conditioned baseline: its transposed weights by the rule the other
        # configurations' images follow (tests/test_trunk_reference_host.py asserts it): bf16 of the weights throughout, fp32 as they are
        net = fine if which == 1 else coarse
        rt = (lambda w: round_to(w, torch.bfloat16)) if precision != "f32" else (lambda w: w.detach().double())
        head_t = torch.cat([rt(net.output_linear.weight.T), torch.zeros(Wd, 8 - net.output_linear.weight.shape[0], dtype=torch.float64)], 1)
        hid_t = {i: rt(net.pts_linears[i].weight[:, -Wd:].T) for i in range(1, D)}
        enc_t = {0: rt(net.pts_linears[0].weight[:, :n_enc].T), skip + 1: rt(net.pts_linears[skip + 1].weight[:, :n_enc].T)}
        return CompiledOperands(Ws, bs, head, alpha, vw, rgb, head_t, hid_t, enc_t, None, None, None, D, Wd, skip, L, LV)
    pb = _Prober(*_pack_image(coarse, fine, precision, 4 + which), precision)
    assert not pb.bias.any(), "backward layers have no bias"
    head_t = rgb_t = join_t = encv_t = None
    if views:
        rgb_t = t64(pb.layer(NT // 2, [("vec", 8)])[0])
        Wm = pb.layer(1 + NT, [("vec", 8), ("hid", Wd // 2)])[0]
        encv_t, join_t = t64(_slots_to_cols(Wm[:32], LV, 1)), t64(Wm[32:])
    else:
        head_t = t64(pb.layer(NT, [("vec", 8)])[0])
    hid_t, enc_t = {}, {}
    for i in range(D - 1, 0, -1):
        if i - 1 == skip:
            Wm = pb.layer(NT + 2, [("hid", Wd)])[0]
            enc_t[i], hid_t[i] = t64(_slots_to_cols(Wm[:64], L, 2)), t64(Wm[64:])
        else:
            hid_t[i] = t64(pb.layer(NT, [("hid", Wd)])[0])
    enc_t[0] = t64(_slots_to_cols(pb.layer(2, [("hid", Wd)])[0], L, 2))
    pb.done()
    return CompiledOperands(Ws, bs, head, alpha, vw, rgb, head_t, hid_t, enc_t, rgb_t, join_t, encv_t, D, Wd, skip, L, LV)


def round_to(x, dtype):
    """float64 values of x rounded to ``dtype`` (round to nearest even, through fp32 like the packers)"""
    return x.detach().to(torch.float32).to(dtype).double()


def module_operands(net, sixteen_bit):
    """The operand weights of a non-compiled trunk from the module's own weights rounded with torch: bf16, and f16 in the columns that meet
    an encoding (layer 0, the encoding columns of the layer behind the skip, the direction columns of the views layer); fp32 mode: as
    they are.  Returns (W [depth], b [depth], extra) with extra = dict of the head's layers (output | alpha, feature, views, rgb).
    ``sixteen_bit`` may also name the precision: "f16" rounds every weight to f16 (the inference kernels' second 16-bit mode)."""
    hdt = torch.float16 if sixteen_bit == "f16" else torch.bfloat16
    sixteen_bit = sixteen_bit not in (False, "f32")
    wdt = (lambda w: round_to(w, hdt)) if sixteen_bit else (lambda w: w.detach().double())
    edt = (lambda w: round_to(w, torch.float16)) if sixteen_bit else (lambda w: w.detach().double())
    n_enc = int(net.input_ch)
    skips = [int(k) for k in net.skips]
    Ws, bs = [], []
    for i, l in enumerate(net.pts_linears):
        w = l.weight
        if i == 0:
            wq = edt(w)
        elif (i - 1) in skips:
            wq = torch.cat([edt(w[:, :n_enc]), wdt(w[:, n_enc:])], 1)
        else:
            wq = wdt(w)
        Ws.append(wq); bs.append(l.bias.detach().double())
    lin = lambda m: (wdt(m.weight), m.bias.detach().double())
    extra = {}
    if net.use_viewdirs:
        Wn = int(net.W)
        vw = net.views_linears[0].weight
        extra = dict(alpha=lin(net.alpha_linear), feature=lin(net.feature_linear), rgb=lin(net.rgb_linear),
                     views=(torch.cat([wdt(vw[:, :Wn]), edt(vw[:, Wn:])], 1), net.views_linears[0].bias.detach().double()))
    else:
        extra = dict(output=lin(net.output_linear))
    return Ws, bs, extra


# ------------------------------------------------------------------------------------------------------------------------
# the whole check of one compiled call, layer by layer, from the kernel's saved arrays
# ------------------------------------------------------------------------------------------------------------------------
class Report:
    """Worst residual / bound per array, worst undecided share per relu array, and what failed."""

    def __init__(self):
        self.ratio, self.undecided, self.failures = {}, {}, []

    def add(self, name, ratio):
        self.ratio[name] = max(self.ratio.get(name, 0.0), ratio)
        if not ratio <= 1.0:
            self.failures.append(f"{name}: residual / bound {ratio:.3g}")

    def bits(self, name, share, wrong, n):
        """UNDECIDED_CAP of the layer's n elements, in whole elements; at least one (a layer of three samples has 768 elements)"""
        self.undecided[name] = max(self.undecided.get(name, 0.0), share)
        if round(share * n) > max(1, int(UNDECIDED_CAP * n)):
            self.failures.append(f"{name}: undecided share {share:.2e} over the cap {UNDECIDED_CAP:.0e}")
        if wrong:
            self.failures.append(f"{name}: {wrong} relu bits wrong")

    def exact(self, name, ok, what):
        if not ok:
            self.failures.append(f"{name}: {what}")

    def worst(self, prefix):
        vals = [v for k, v in self.ratio.items() if k.startswith(prefix)]
        return max(vals) if vals else 0.0

    def summary(self):
        groups = {}
        for k, v in self.ratio.items():
            g = k.split("[")[0]
            groups[g] = max(groups.get(g, 0.0), v)
        und = max(self.undecided.values(), default=0.0)
        return ", ".join(f"{g} {v:.3f}" for g, v in groups.items()) + f"; worst undecided share {und:.1e}"


def check_padding(rep, acts_pad=None, d_pre_pad=None):
    """The columns beyond a ray's end: finite activations, exactly zero gradients."""
    if acts_pad is not None:
        rep.exact("acts padding", bool(torch.isfinite(acts_pad.float()).all()), "a padded activation column is not finite")
    if d_pre_pad is not None:
        rep.exact("d_pre padding", bool((d_pre_pad.float() == 0).all()), "a padded gradient column is not exactly zero")
    return rep


def check_compiled_forward(ops, sixteen_bit, pts, acts, bits, raw4, raw=None, ray_bias=None, dirs=None, hv=None, hv_bits=None, rep=None):
    """Every forward layer of nrnerf_trunk_forward from its own saved input.  pts [N, S, 3] fp32; acts [D, N, S, W] decoded rows (any
    float type); bits [D, N, S, W] bool (the kernel's relu record; fp32 mode: None, the stored sign decides); raw4 [N, S, 4];
    raw [N, S, c] or None; ray_bias [N, 2, W] or None; dirs [N, S, 3], hv [N, S, W / 2], hv_bits: the view-dependent head."""
    rep = rep or Report()
    dev = pts.device
    op, delta = encoding_operand(pts, ops.L, sixteen_bit)
    for i in range(ops.depth):
        reads_enc = i == 0 or i - 1 == ops.skip
        X = op if i == 0 else (torch.cat([op, acts[i - 1].double()], -1) if reads_enc else acts[i - 1].double())
        extra = None
        if ray_bias is not None and reads_enc:
            extra = ray_bias[:, 0 if i == 0 else 1].double().unsqueeze(1)
        pre, A, B = layer64(X, ops.W[i].to(dev), ops.b[i].to(dev), delta if reads_enc else None, extra)
        rep.add(f"acts[{i}]", hidden_ratio(acts[i], pre, B, sixteen_bit))
        bit = bits[i] if bits is not None else acts[i] > 0
        rep.bits(f"relu[{i}]", *relu_bit_check(bit, pre, B, acts[i]))
    h = acts[ops.depth - 1].double()
    if ops.head is not None:
        pre, A, B = layer64(h, ops.head[0].to(dev), ops.head[1].to(dev))
        rep.add("raw4", linear_ratio(raw4, pre[..., :4], B[..., :4]))
        if raw is not None:
            c = raw.shape[-1]
            rep.add("raw", linear_ratio(raw, pre[..., :c], B[..., :c]))
    else:
        pre, A, B = layer64(h, ops.alpha[0].to(dev), ops.alpha[1].to(dev))
        rep.add("raw4.sigma", linear_ratio(raw4[..., 3:4], pre, B))
        opv, deltav = encoding_operand(dirs, ops.LV, sixteen_bit)
        pre, A, B = layer64(torch.cat([opv, h], -1), ops.views[0].to(dev), ops.views[1].to(dev), deltav)
        rep.add("hv", hidden_ratio(hv, pre, B, sixteen_bit))
        rep.bits("relu[hv]", *relu_bit_check(hv_bits if hv_bits is not None else hv > 0, pre, B, hv))
        pre, A, B = layer64(hv.double(), ops.rgb[0].to(dev), ops.rgb[1].to(dev))
        rep.add("raw4.rgb", linear_ratio(raw4[..., :3], pre, B))
        if raw is not None:
            rep.exact("raw", torch.equal(raw, raw4), "the view-dependent head's raw is raw4")
    return rep


def check_compiled_backward(ops, sixteen_bit, pts, d_raw4, bits, d_pre, d_pts4, dirs=None, hv_bits=None, d_pre_v=None, d_dirs=None, rep=None):
    """Every backward layer of nrnerf_trunk_backward from its own stored input: d_pre [D, N, S, W] decoded rows, bits the forward's relu
    record (fp32 mode: acts > 0), d_pts4 [N, S, 4]; the view-dependent head's d_pre_v [N, S, W / 2], hv_bits, d_dirs [N, S, 3] or None."""
    rep = rep or Report()
    dev = pts.device
    g = round_to(d_raw4, torch.bfloat16) if sixteen_bit else d_raw4.double()
    g8 = torch.cat([g, torch.zeros_like(g)], -1)
    eps_sc = EPS_SC if sixteen_bit else 4 * U32
    top = ops.depth - 1
    if ops.head_t is not None:
        pre, A, B = layer64(g8, ops.head_t.to(dev))
    else:
        pre, A, B = layer64(g8, ops.rgb_t.to(dev))
        rep.add("d_pre_v", hidden_ratio(d_pre_v, pre, B, sixteen_bit, hv_bits))
        Xj = torch.cat([g8, d_pre_v.double()], -1)
        if d_dirs is not None:
            dencv, _, Bv = layer64(Xj, ops.encv_t.to(dev))
            want, bound = encoding_backward64(dirs, dencv, Bv, ops.LV, eps_sc)
            rep.add("d_dirs", _ratio((d_dirs.double() - want).abs(), bound))
        pre, A, B = layer64(Xj, ops.join_t.to(dev))
    rep.add(f"d_pre[{top}]", hidden_ratio(d_pre[top], pre, B, sixteen_bit, bits[top]))
    denc = Benc = None
    for i in range(top, 0, -1):
        Z = d_pre[i].double()
        pre, A, B = layer64(Z, ops.hid_t[i].to(dev))
        rep.add(f"d_pre[{i - 1}]", hidden_ratio(d_pre[i - 1], pre, B, sixteen_bit, bits[i - 1]))
        if i in ops.enc_t:
            denc, _, Benc = layer64(Z, ops.enc_t[i].to(dev))
    d0, A0, B0 = layer64(d_pre[0].double(), ops.enc_t[0].to(dev))
    if denc is None:
        denc, Benc = d0, B0
    else:                       # the two sources are added in fp32
        denc, Benc = denc + d0, Benc + B0 + U32 * (denc + d0).abs()
    want, bound = encoding_backward64(pts, denc, Benc, ops.L, eps_sc)
    rep.add("d_pts4", _ratio((d_pts4[..., :3].double() - want).abs(), bound))
    rep.exact("d_pts4", bool((d_pts4[..., 3] == 0).all()), "the fourth component is exactly 0")
    return rep


# ------------------------------------------------------------------------------------------------------------------------
# the generic entry points (nrnerf_generic_trunk_forward / _backward): row-major arrays, any depth / width / skip
# ------------------------------------------------------------------------------------------------------------------------
def gx_relu_bits_to_bool(bits, depth, n_rays, S, width):
    """The width-class route's ``relu_bits`` (csrc/nrnerf_gx16.h ``keep`` / nrnerf_gx16_bwd.h): bytes [layer][16-sample block][64 lanes]
    [4 ceil(WC / 128)], WC = width rounded up to 64; lane 16 g + n holds sample n of the block, byte p of its record is tile pair p and
    bit e of it element e of the lane's packed fragment: feature 32 p + 4 g + e (e < 4) or 32 p + 16 + 4 g + e - 4.  A bit says the STORED
    activation is nonzero.  -> bool [layer][n_rays][S][width]."""
    WC = (width + 63) // 64 * 64
    NP = WC // 32
    bpl = 4 * ((NP + 3) // 4)
    bpr = (S + 15) // 16
    b = bits.reshape(depth, n_rays * bpr, 4, 16, bpl)[..., :NP].to(torch.int32)
    e = torch.arange(8, device=bits.device, dtype=torch.int32)
    x = ((b.unsqueeze(-1) >> e) & 1).bool()                                              # [layer, block, g, n, p, e]
    x = x.permute(0, 1, 3, 2, 4, 5).reshape(depth, n_rays * bpr, 16, 4 * NP * 8)
    inv = torch.empty(WC, dtype=torch.long)
    for g in range(4):
        for p in range(NP):
            for q in range(8):
                inv[32 * p + 4 * g + q if q < 4 else 32 * p + 16 + 4 * g + q - 4] = (g * NP + p) * 8 + q
    rows = x[..., inv.to(bits.device)].reshape(depth, n_rays, bpr * 16, WC)
    return rows[:, :, :S, :width]


def check_generic_forward(net, sixteen_bit, pts, acts, raw4, raw=None, dirs=None, gx_bits=None, rep=None):
    """Every forward layer of nrnerf_generic_trunk_forward from its own saved input.  acts [depth (+ 2), N, S, W] rows; gx_bits: the decoded
    relu_bits of the width-class route ([depth, N, S, W] bool) or None."""
    rep = rep or Report()
    Ws, bs, extra = module_operands(net, sixteen_bit)
    D, Wn, L = int(net.D), int(net.W), (int(net.input_ch) - 3) // 6
    skips = [int(k) for k in net.skips]
    op, delta = encoding_operand(pts, L, sixteen_bit)
    dev = pts.device
    for i in range(D):
        reads_enc = i == 0 or (i - 1) in skips
        X = op if i == 0 else (torch.cat([op, acts[i - 1].double()], -1) if reads_enc else acts[i - 1].double())
        pre, A, B = layer64(X, Ws[i].to(dev), bs[i].to(dev), delta if reads_enc else None)
        rep.add(f"acts[{i}]", hidden_ratio(acts[i], pre, B, sixteen_bit))
        rep.bits(f"relu[{i}]", *relu_bit_check(acts[i] > 0, pre, B))
        if gx_bits is not None:
            rep.bits(f"relu_bits[{i}]", *relu_bit_check(gx_bits[i], pre, B, acts[i]))
            rep.exact(f"relu_bits[{i}]", torch.equal(gx_bits[i], acts[i] != 0), "a bit is not 'the stored activation is nonzero'")
    h = acts[D - 1].double()
    if raw is not None:
        rep.exact("raw", torch.equal(raw[..., :4], raw4), "the first four channels of raw are raw4")
    if not net.use_viewdirs:
        pre, A, B = layer64(h, extra["output"][0].to(dev), extra["output"][1].to(dev))
        rep.add("raw4", linear_ratio(raw4, pre[..., :4], B[..., :4]))
        if raw is not None:
            c = raw.shape[-1]
            rep.add("raw", linear_ratio(raw, pre[..., :c], B[..., :c]))
        return rep
    LV = (int(net.input_ch_views) - 3) // 6
    half = int(net.views_linears[0].weight.shape[0])
    pre, A, B = layer64(h, extra["alpha"][0].to(dev), extra["alpha"][1].to(dev))
    rep.add("raw4.sigma", linear_ratio(raw4[..., 3:4], pre, B))
    pre, A, B = layer64(h, extra["feature"][0].to(dev), extra["feature"][1].to(dev))
    keep_all = torch.ones_like(pre, dtype=torch.bool)
    rep.add(f"acts[{D}] (feature)", hidden_ratio(acts[D], pre, B, sixteen_bit, keep_all))
    opv, deltav = encoding_operand(dirs, LV, sixteen_bit)
    Wv = extra["views"][0].to(dev)
    hv = acts[D + 1][..., :half]
    Wvq = torch.cat([Wv[:, Wn:], Wv[:, :Wn]], 1)
    pre, A, B = layer64(torch.cat([opv, acts[D].double()], -1), Wvq, extra["views"][1].to(dev), deltav)
    rep.add(f"acts[{D + 1}] (colour)", hidden_ratio(hv, pre, B, sixteen_bit))
    rep.bits(f"relu[{D + 1}]", *relu_bit_check(hv > 0, pre, B))
    pre, A, B = layer64(hv.double(), extra["rgb"][0].to(dev), extra["rgb"][1].to(dev))
    rep.add("raw4.rgb", linear_ratio(raw4[..., :3], pre, B))
    return rep


def check_generic_backward(net, sixteen_bit, d_raw4, bits, d_pre, d_enc0, d_enc1=None, d_encv=None, hv_bits=None, rep=None, tag=""):
    """Every backward layer of nrnerf_generic_trunk_backward from its own stored input; transposed weights bf16 throughout (fp32 mode: as
    they are).  bits [depth, N, S, W]: the mask the route applies (the forward's relu_bits, or acts > 0); hv_bits: acts[depth + 1] > 0."""
    rep = rep or Report()
    dev = d_raw4.device
    wt = (lambda w: round_to(w, torch.bfloat16).to(dev)) if sixteen_bit else (lambda w: w.detach().double().to(dev))
    D, Wn, n_enc = int(net.D), int(net.W), int(net.input_ch)
    skips = [int(k) for k in net.skips]
    g = round_to(d_raw4, torch.bfloat16) if sixteen_bit else d_raw4.double()
    if not net.use_viewdirs:
        pre, A, B = layer64(g, wt(net.output_linear.weight[:4].T))
    else:
        half = int(net.views_linears[0].weight.shape[0])
        pre, A, B = layer64(g[..., :3], wt(net.rgb_linear.weight.T))
        zv = d_pre[D + 1][..., :half]
        rep.add(f"{tag}d_pre[{D + 1}] (colour)", hidden_ratio(zv, pre, B, sixteen_bit, hv_bits))
        Wv = net.views_linears[0].weight
        pre, A, B = layer64(zv.double(), wt(Wv[:, Wn:].T))
        rep.add(f"{tag}d_encv", linear_ratio(d_encv, pre, B))
        pre, A, B = layer64(zv.double(), wt(Wv[:, :Wn].T))
        rep.add(f"{tag}d_pre[{D}] (feature)", hidden_ratio(d_pre[D], pre, B, sixteen_bit, torch.ones_like(pre, dtype=torch.bool)))
        X = torch.cat([d_pre[D].double(), g[..., 3:4]], -1)
        pre, A, B = layer64(X, torch.cat([wt(net.feature_linear.weight.T), wt(net.alpha_linear.weight.T)], 1))
    rep.add(f"{tag}d_pre[{D - 1}]", hidden_ratio(d_pre[D - 1], pre, B, sixteen_bit, bits[D - 1]))
    for i in range(D - 1, 0, -1):
        Z = d_pre[i].double()
        w = net.pts_linears[i].weight
        if (i - 1) in skips:
            pre, A, B = layer64(Z, wt(w[:, :n_enc].T))
            rep.add(f"{tag}d_enc1", linear_ratio(d_enc1, pre, B))
            w = w[:, n_enc:]
        pre, A, B = layer64(Z, wt(w.T))
        rep.add(f"{tag}d_pre[{i - 1}]", hidden_ratio(d_pre[i - 1], pre, B, sixteen_bit, bits[i - 1]))
    pre, A, B = layer64(d_pre[0].double(), wt(net.pts_linears[0].weight.T))
    rep.add(f"{tag}d_enc0", linear_ratio(d_enc0, pre, B))
    return rep
