"""A float64 reference of ONE layer at a time of the ray bender's training kernels (csrc/nrnerf_train_bend.h: bend_fwd_train, bend_bwd,
bend_div_fwd, bend_div_bwd, bend_wgrad, bend_wgrad16 behind nrnerf_bender_forward / _backward / _wgrad and nrnerf_bender_divergence_*).

The principle is tests/trunk_reference.py's: the kernels save, per layer, the values they hand to the next layer, so every layer is
checked on its own from the kernel's OWN saved input to it (exact in float64) with an a-priori rounding bound, and nothing drifts through
the layers.  These kernels are simpler to hold than the trunk's: the saved arrays are plain row-major [layer][M][width], the operand
weights are the module's own fp32 weights, and the relu mask of every backward layer is the sign of the kernel's own saved activation --
no element is excused anywhere.

Bounds.  An fp32 accumulation of K products and a bias in any order: (K + 3) U32 A, A = |x| |W|^T + |b| (trunk_reference.layer64), plus a
floor of K 2^-126 per element in case the fp32 matrix pipe flushes denormals.  bf16 model: the chain itself runs in fp32 registers and
only the SAVED arrays are bf16, each stored value a rounding of what the next layer consumed, so a layer's input is known to
U16 |saved| per element: B widens by U16 |saved_in| |W|^T and a stored hidden value is held to U16 |pre64| + (1 + U16) B.  The scalar
expressions of the heads (nrnerf_train_bend.h: the lines after the loads in bend_bwd and bend_div_bwd, the tail of bend_div_fwd) are
evaluated in float64 with a running error bound in the standard model: one U32 per fp32 operation on the magnitude of its result, input
errors propagated to first order with their cross terms (`_V`).  A fused multiply-add rounds once where the separate operations round
twice, so the bound holds whichever products the compiler contracts; 1 - th^2 carries U32 (th^2 + |1 - th^2|), an absolute error.

tanhf: TANH_ULP = 5, the OpenCL C table's figure for tanh.  The device math library ships no accuracy table of its own with the
toolchain (none is installed next to it), so the table it follows is used.  It is the only number here that is not derived; the share of
the off4.w bound it makes up is reported (Report.tanh_share).

Plain torch, float64, no kernels; imports without a GPU.  Every function works on whatever device its tensors live on.
"""
import dataclasses

import torch

from tests.trunk_reference import U16, U32, Report, _ratio, hidden_ratio, layer64, linear_ratio

TANH_ULP = 5.0              # ulp allowance of tanhf (OpenCL C table); see the module docstring
DENORM = 2.0 ** -126        # smallest normal fp32: what one flushed product or operation can lose
SLOT = 64 * 64 + 64         # NRNERF_BENDER_WGRAD_SLOT: dW [64][64] then db [64]


@dataclasses.dataclass
class Knobs:
    """The editing knobs of a call (has_rigidity_cutoff / has_test_time_scaling and the values behind them); None = off."""
    cutoff: float | None = None
    scaling: float | None = None


def weights64(rb, device="cpu"):
    """The operand weights: the module's own, float64.  (Wb, bb): the offset MLP (the last layer has no bias: None); (Wr, br): rigidity."""
    d = lambda t: None if t is None else t.detach().double().to(device)
    return dict(Wb=[d(l.weight) for l in rb.network], bb=[d(l.bias) for l in rb.network],
                Wr=[d(l.weight) for l in rb.rigidity_network], br=[d(l.bias) for l in rb.rigidity_network])


def points_fp32(rays, z):
    """p = o + d z as the kernels form it (__fmul_rn, __fadd_rn): one rounded product and one rounded sum -- two separate torch fp32 ops
    give the same bits.  rays [N, >= 6] fp32, z [N, S] fp32 -> [N S, 3] fp32.  It is exact input to the first layers."""
    assert rays.dtype == torch.float32 and z.dtype == torch.float32
    prod = rays[:, None, 3:6] * z[:, :, None]
    return (rays[:, None, 0:3] + prod).reshape(-1, 3)


def per_sample(latents, S, L):
    """[N, >= L] per-ray codes -> [N S, L]"""
    return latents[:, None, :L].expand(latents.shape[0], S, L).reshape(-1, L)


def _f32(x, like):
    return torch.tensor(float(x), dtype=torch.float32, device=like.device)


def mask_fp32(th, knobs):
    """The rigidity mask from the stored tanh, in the precision of th -- fp32 for a kernel's array, as the kernels compute it:
    (th + 1) / 2, 0 where the cutoff bites (the knob is an fp32 number).  Returns (mask, cut bool)."""
    mask = (th + 1.0) / 2.0
    cut = torch.zeros_like(mask, dtype=torch.bool)
    if knobs.cutoff is not None:
        cut = mask <= _f32(knobs.cutoff, th)
        mask = torch.where(cut, torch.zeros_like(mask), mask)
    return mask, cut


def bent4_expected(p, off4, knobs):
    """bent4 from the kernel's own off4, bit for bit: every operation is an explicit round-to-nearest one in the kernel
    (bent = p + fl(fl(mask off) scaling), .w = the mask after the cutoff)."""
    assert p.dtype == torch.float32 and off4.dtype == torch.float32
    mask, _ = mask_fp32(off4[:, 3], knobs)
    mo = mask[:, None] * off4[:, :3]
    if knobs.scaling is not None:
        mo = mo * _f32(knobs.scaling, p)
    return torch.cat([p + mo, mask[:, None]], 1)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_bent4(rep, bent4, p, off4, knobs):
    want = bent4_expected(p, off4, knobs)
    if not bits_equal(bent4, want):
        n = (bent4.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum(0).tolist()
        rep.exact("bent4", False, f"not bit for bit p + fl(fl(mask off) scaling) of the kernel's own off4: {n} elements of x, y, z, mask differ")


# ------------------------------------------------------------------------------------------------------------------------
# one layer, one chain
# ------------------------------------------------------------------------------------------------------------------------
def _lin(X, W, b=None, widen=False):
    """pre64, A, B of one layer from its saved input X (trunk_reference.layer64) with the denormal floor; widen: X is a bf16 rounding
    of what the kernel multiplied, known to U16 |X| per element."""
    pre, A, B = layer64(X, W, b)
    B = B + X.shape[-1] * DENORM
    if widen:
        B = B + U16 * (X.double().abs() @ W.double().abs().T)
    return pre, A, B


def _value_chain(rep, name, Ws, bs, x0, acts, sixteen):
    """Hidden layers 0 .. n-2 of an MLP from their saved inputs; returns (pre64, B) of the last, linear layer."""
    n = len(Ws)
    for i in range(n - 1):
        pre, _, B = _lin(x0 if i == 0 else acts[i - 1], Ws[i], bs[i], widen=sixteen and i > 0)
        rep.add(f"{name}[{i}]", hidden_ratio(acts[i], pre, B, sixteen))
    pre, _, B = _lin(acts[n - 2], Ws[n - 1], bs[n - 1], widen=sixteen)
    return pre, B


def _tangent_chain(rep, name, Ws, t0, acts, tacts, sixteen):
    """tz_i = th_(i-1) W_i^T, th_i = [stored activation > 0] tz_i, th_0 = (probe, 0): only the point columns of W_0 meet a nonzero.
    Returns (pre64, B) of the last layer's tangent (no bias anywhere)."""
    n = len(Ws)
    for i in range(n - 1):
        pre, _, B = _lin(t0 if i == 0 else tacts[i - 1], Ws[0][:, :3] if i == 0 else Ws[i], None, widen=sixteen and i > 0)
        bit = acts[i] > 0
        rep.add(f"{name}[{i}]", hidden_ratio(tacts[i], pre, B, sixteen, bit))
        rep.exact(f"{name}[{i}]", bool((tacts[i][~bit] == 0).all()), "a tangent under a dead relu is not exactly 0")
    pre, _, B = _lin(tacts[n - 2], Ws[n - 1], None, widen=sixteen)
    return pre, B


def _backward_chain(rep, name, Ws, g_out, acts, dz, sixteen):
    """dz_(i-1) = [stored activation_(i-1) > 0] (dz_i W_i), from the kernel's own stored dz_i (g_out, fp32, for the top layer);
    K = the out-features of the layer above.  Every element is decided; a gradient under a dead relu is exactly 0."""
    n = len(Ws)
    for i in range(n - 1, 0, -1):
        pre, _, B = _lin(g_out if i == n - 1 else dz[i], Ws[i].T, None, widen=sixteen and i < n - 1)
        bit = acts[i - 1] > 0
        rep.add(f"{name}[{i - 1}]", hidden_ratio(dz[i - 1], pre, B, sixteen, bit))
        rep.exact(f"{name}[{i - 1}]", bool((dz[i - 1][~bit] == 0).all()), "a gradient under a dead relu is not exactly 0")


def _latent_rows(rep, Wb0, dz0, d_lat, sixteen):
    L = d_lat.shape[-1]
    pre, _, B = _lin(dz0, Wb0[:, 3:3 + L].T, None, widen=sixteen)
    rep.add("d_latents", linear_ratio(d_lat, pre, B))
    return pre, B


# ------------------------------------------------------------------------------------------------------------------------
# scalar fp32 expressions: float64 value + running bound
# ------------------------------------------------------------------------------------------------------------------------
class _V:
    """a float64 value v of an fp32 quantity and a bound e on |computed - v|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v.double()
        self.e = torch.zeros_like(self.v) if e is None else e

    def _round(self, v, e):
        return _V(v, e + U32 * (v.abs() + e) + DENORM)

    def __mul__(self, o):
        return self._round(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def __add__(self, o):
        return self._round(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return self._round(self.v - o.v, self.e + o.e)

    def half(self):                 # an exact scaling
        return _V(0.5 * self.v, 0.5 * self.e)

    def where(self, cond, other=0.0):
        return _V(torch.where(cond, torch.full_like(self.v, other), self.v), torch.where(cond, torch.zeros_like(self.e), self.e))

    def col(self, c):
        return _V(self.v[:, c], self.e[:, c])


def _stack(cols):
    return _V(torch.stack([c.v for c in cols], 1), torch.stack([c.e for c in cols], 1))


def _one_minus_sq(th):
    """1 - th^2 of an exact fp32 th: error U32 (th^2 + |1 - th^2|), absolute (the cancellation near |th| = 1)"""
    return _V(torch.ones_like(th.v)) - th * th


def _render_head(mask, off4, knobs, g_bent4, g_bent4_b, g_unmasked, g_mask):
    """The head of bend_bwd (and of bend_div_bwd's render cotangents): from the gradients of (bent point, unmasked offsets, rigidity mask)
        g_off[c] = gb[c] mask sc + g_unmasked[c],   g_m = g_mask + sum_c gb[c] off[c] sc,   gb = g_bent4 + g_bent4_b
    with mask the kernel's own (after the cutoff), off the kernel's own off4.  Returns (g_off [M,3], g_m [M]) as _V."""
    M = off4.shape[0]
    zero3 = torch.zeros(M, 3, dtype=torch.float64, device=off4.device)
    gb = _V(g_bent4[:, :3]) if g_bent4 is not None else _V(zero3)
    if g_bent4_b is not None:
        gb = gb + _V(g_bent4_b[:, :3])
    sc = None if knobs.scaling is None else _V(_f32(knobs.scaling, off4).expand(M))
    m, g_offs = _V(mask), []
    g_m = _V(g_mask.reshape(M)) if g_mask is not None else _V(zero3[:, 0])
    for c in range(3):
        t = gb.col(c) * m
        if sc is not None:
            t = t * sc
        if g_unmasked is not None:
            t = t + _V(g_unmasked[:, c])
        g_offs.append(t)
        t = gb.col(c) * _V(off4[:, c])
        if sc is not None:
            t = t * sc
        g_m = g_m + t
    return _stack(g_offs), g_m


def bender_head_backward(off4, bent4, knobs, g_bent4, g_bent4_b=None, g_unmasked=None, g_mask=None):
    """dz_out4 of bend_bwd in float64 with its bound: (g_off xyz, g_logit = g_m (1 - th^2) / 2, exactly 0 where the cutoff bites --
    decided in fp32 from the stored th, as the kernel does).  Returns _V [M,4]."""
    th = off4[:, 3]
    _, cut = mask_fp32(th, knobs)
    g_off, g_m = _render_head(bent4[:, 3], off4, knobs, g_bent4, g_bent4_b, g_unmasked, g_mask)
    g_logit = (g_m.half() * _one_minus_sq(_V(th))).where(cut)
    return _stack([g_off.col(0), g_off.col(1), g_off.col(2), g_logit])


def divergence_head_forward(off4, toff4, probe, knobs):
    """divergence = s e . (tm off + m toff) and tangent = s (tm off + m toff) from the kernel's own off4 / toff4:
    m = (th + 1) / 2 (fp32, exact from the stored th), tm = (1 - th^2) / 2 tl, both 0 where the cutoff bites.  Returns (_V [M], _V [M,3])."""
    th, tl = off4[:, 3], toff4[:, 3]
    mask, cut = mask_fp32(th, knobs)
    m = _V(mask)
    tm = (_one_minus_sq(_V(th)).half() * _V(tl)).where(cut)
    M = off4.shape[0]
    sc = None if knobs.scaling is None else _V(_f32(knobs.scaling, off4).expand(M))
    d, tv = None, []
    for c in range(3):
        v = tm * _V(off4[:, c]) + m * _V(toff4[:, c])
        t = _V(probe[:, c]) * v
        d = t if d is None else d + t
        tv.append(v if sc is None else sc * v)
    if sc is not None:
        d = d * sc
    return d, _stack(tv)


def divergence_head_backward(off4, toff4, probe, knobs, g_divergence=None, g_tangent=None, render=None):
    """dz_out4 / dtz_out4 of bend_div_bwd (nrnerf_train_bend.h, the head comment of the divergence kernels):
        gv = g_tangent s  or  g_divergence s e
        g_off = gv tm (+ render's),  g_toff = gv m,  g_m = gv . toff (+ render's),  g_tm = gv . off
        g_logit = g_m (1 - t^2) / 2 - g_tm tl t (1 - t^2),   g_tl = g_tm (1 - t^2) / 2;   both 0 where the cutoff bites
    render: dict(g_bent4, g_bent4_b, g_unmasked, g_mask) or None -- they enter as in bend_bwd, with this call's own mask.
    Returns (_V [M,4], _V [M,4])."""
    th, tl = off4[:, 3], toff4[:, 3]
    mask, cut = mask_fp32(th, knobs)
    M = off4.shape[0]
    m, q = _V(mask), _one_minus_sq(_V(th))
    s2 = q.half()
    tm = (s2 * _V(tl)).where(cut)
    one = _V(torch.ones(M, dtype=torch.float64, device=off4.device))
    sc = one if knobs.scaling is None else _V(_f32(knobs.scaling, off4).expand(M))
    exact_one = knobs.scaling is None                       # a product with 1.0f is exact
    times_sc = (lambda x: x) if exact_one else (lambda x: x * sc)
    if g_tangent is not None:
        gv = [times_sc(_V(g_tangent[:, c])) for c in range(3)]
    else:
        g = times_sc(_V(g_divergence.reshape(M)))
        gv = [g * _V(probe[:, c]) for c in range(3)]
    g_off = [gv[c] * tm for c in range(3)]
    g_toff = [gv[c] * m for c in range(3)]
    g_m = g_tm = None
    for c in range(3):
        a, b = gv[c] * _V(toff4[:, c]), gv[c] * _V(off4[:, c])
        g_m = a if g_m is None else g_m + a
        g_tm = b if g_tm is None else g_tm + b
    if render is not None and any(v is not None for v in render.values()):
        r_off, r_m = _render_head(mask, off4, knobs, render.get("g_bent4"), render.get("g_bent4_b"), render.get("g_unmasked"), render.get("g_mask"))
        g_off = [g_off[c] + r_off.col(c) for c in range(3)]
        g_m = g_m + r_m
    g_logit = (g_m * s2 - ((g_tm * _V(tl)) * _V(th)) * q).where(cut)
    g_tl = (g_tm * s2).where(cut)
    return _stack(g_off + [g_logit]), _stack(g_toff + [g_tl])


def _check_v(rep, name, stored, want):
    rep.add(name, _ratio((stored.double() - want.v).abs(), want.e))


# ------------------------------------------------------------------------------------------------------------------------
# the checks of one call
# ------------------------------------------------------------------------------------------------------------------------
def _check_heads_forward(rep, off_pre, off_B, logit_pre, logit_B, off4):
    rep.add("off4.xyz", linear_ratio(off4[:, :3], off_pre, off_B))
    th64 = torch.tanh(logit_pre[:, 0])
    t_term = TANH_ULP * U32 * th64.abs()
    bound = logit_B[:, 0] + t_term                       # |tanh'| <= 1
    rep.add("off4.w", _ratio((off4[:, 3].double() - th64).abs(), bound))
    share = float((t_term / bound.clamp_min(1e-300)).max()) if bound.numel() else 0.0
    rep.tanh_share = max(getattr(rep, "tanh_share", 0.0), share)


def check_bender_forward(rb, sixteen, knobs, rays, z, latents, out, rep=None):
    """nrnerf_bender_forward.  rays [N, >= 6], z [N, S], latents [N, >= L] (fp32); out: acts_offsets [D-1, M, 64], acts_rigidity
    [RD-1, M, 32] (fp32 or bf16), off4, bent4 [M, 4]."""
    rep = rep or Report()
    w = weights64(rb, rays.device)
    L = w["Wb"][0].shape[1] - 3
    p = points_fp32(rays, z)
    x0 = torch.cat([p, per_sample(latents, z.shape[1], L)], 1)
    off_pre, off_B = _value_chain(rep, "acts_offsets", w["Wb"], w["bb"], x0, out["acts_offsets"], sixteen)
    lg_pre, lg_B = _value_chain(rep, "acts_rigidity", w["Wr"], w["br"], p, out["acts_rigidity"], sixteen)
    _check_heads_forward(rep, off_pre, off_B, lg_pre, lg_B, out["off4"])
    _check_bent4(rep, out["bent4"], p, out["off4"], knobs)
    return rep


def check_bender_backward(rb, sixteen, knobs, out, g_bent4, g_bent4_b=None, g_unmasked=None, g_mask=None, rep=None):
    """nrnerf_bender_backward from the forward's arrays (acts_*, off4, bent4) and its own (dz_offsets, dz_rigidity, dz_out4, d_latents)."""
    rep = rep or Report()
    w = weights64(rb, out["off4"].device)
    head = bender_head_backward(out["off4"], out["bent4"], knobs, g_bent4, g_bent4_b, g_unmasked, g_mask)
    _check_v(rep, "dz_out4", out["dz_out4"], head)
    _, cut = mask_fp32(out["off4"][:, 3], knobs)
    rep.exact("dz_out4", bool((out["dz_out4"][:, 3][cut] == 0).all()), "the logit's gradient is not exactly 0 where the cutoff bites")
    _backward_chain(rep, "dz_offsets", w["Wb"], out["dz_out4"][:, :3], out["acts_offsets"], out["dz_offsets"], sixteen)
    _backward_chain(rep, "dz_rigidity", w["Wr"], out["dz_out4"][:, 3:4], out["acts_rigidity"], out["dz_rigidity"], sixteen)
    _latent_rows(rep, w["Wb"][0], out["dz_offsets"][0], out["d_latents"], sixteen)
    return rep


def check_divergence_forward(rb, sixteen, knobs, points, latents, probe, out, rep=None):
    """nrnerf_bender_divergence_forward.  points, probe [M, 3], latents [M, L] one row per point (the caller expands a single code);
    out: acts_*, tacts_*, off4, toff4, divergence [M], optionally tangent [M, 3] and bent4 [M, 4]."""
    rep = rep or Report()
    w = weights64(rb, points.device)
    x0 = torch.cat([points, latents], 1)
    off_pre, off_B = _value_chain(rep, "acts_offsets", w["Wb"], w["bb"], x0, out["acts_offsets"], sixteen)
    lg_pre, lg_B = _value_chain(rep, "acts_rigidity", w["Wr"], w["br"], points, out["acts_rigidity"], sixteen)
    _check_heads_forward(rep, off_pre, off_B, lg_pre, lg_B, out["off4"])
    toff_pre, toff_B = _tangent_chain(rep, "tacts_offsets", w["Wb"], probe, out["acts_offsets"], out["tacts_offsets"], sixteen)
    tl_pre, tl_B = _tangent_chain(rep, "tacts_rigidity", w["Wr"], probe, out["acts_rigidity"], out["tacts_rigidity"], sixteen)
    rep.add("toff4.xyz", linear_ratio(out["toff4"][:, :3], toff_pre, toff_B))
    rep.add("toff4.w", linear_ratio(out["toff4"][:, 3:4], tl_pre, tl_B))        # the tangent of the logit is linear: no tanh in it
    d, tv = divergence_head_forward(out["off4"], out["toff4"], probe, knobs)
    _check_v(rep, "divergence", out["divergence"], d)
    if out.get("tangent") is not None:
        _check_v(rep, "tangent", out["tangent"], tv)
    if out.get("bent4") is not None:
        _check_bent4(rep, out["bent4"], points, out["off4"], knobs)
    return rep


def check_divergence_backward(rb, sixteen, knobs, points, latents, probe, out, g_divergence=None, g_tangent=None, render=None,
                              partials=None, n_partials=None, rep=None):
    """nrnerf_bender_divergence_backward: the head, both chains layer by layer, d_latents, and (partials given) the weight gradients.
    Returns (rep, results of check_wgrad or None)."""
    rep = rep or Report()
    w = weights64(rb, points.device)
    hz, htz = divergence_head_backward(out["off4"], out["toff4"], probe, knobs, g_divergence, g_tangent, render)
    _check_v(rep, "dz_out4", out["dz_out4"], hz)
    _check_v(rep, "dtz_out4", out["dtz_out4"], htz)
    _, cut = mask_fp32(out["off4"][:, 3], knobs)
    rep.exact("dz_out4", bool((out["dz_out4"][:, 3][cut] == 0).all() and (out["dtz_out4"][:, 3][cut] == 0).all()),
              "the logit's gradients are not exactly 0 where the cutoff bites")
    for nm, ws, acts in (("offsets", w["Wb"], out["acts_offsets"]), ("rigidity", w["Wr"], out["acts_rigidity"])):
        col = slice(0, 3) if nm == "offsets" else slice(3, 4)
        _backward_chain(rep, f"dz_{nm}", ws, out["dz_out4"][:, col], acts, out[f"dz_{nm}"], sixteen)
        _backward_chain(rep, f"dtz_{nm}", ws, out["dtz_out4"][:, col], acts, out[f"dtz_{nm}"], sixteen)
    _latent_rows(rep, w["Wb"][0], out["dz_offsets"][0], out["d_latents"], sixteen)
    res = None
    if partials is not None:
        res = check_wgrad(rep, partials, divergence_jobs(sixteen, points, latents, probe, out), points.shape[0], n_partials, sixteen)
    return rep, res


# ------------------------------------------------------------------------------------------------------------------------
# weight gradients
# ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Job:
    """One job of bend_wgrad / bend_wgrad16: dW[:out, :inn] = dz^T x (+ dz2^T x2), db[:out] = column sums of db_src.  dz, x, dz2, x2: the
    OPERANDS, float64 (bf16 model: the fp32 rows already rounded to bf16); db_src: dz as stored (the bias sum is taken before any rounding)."""
    name: str
    dz: torch.Tensor
    x: torch.Tensor
    out: int
    inn: int
    db_src: torch.Tensor
    dz2: torch.Tensor | None = None
    x2: torch.Tensor | None = None


def _operand(t, sixteen):
    """An fp32 row as the contraction takes it: bf16 model -- rounded to bf16 (nearest even) in registers; a bf16 array is taken as stored."""
    if sixteen and t.dtype == torch.float32:
        return t.to(torch.bfloat16).double()
    return t.double()


def _chain_jobs(name, sixteen, x0, acts, dz, g_out, t0=None, tacts=None, dtz=None, tg_out=None):
    n = acts.shape[0] + 1
    op = lambda t: None if t is None else _operand(t, sixteen)
    two = dtz is not None
    jobs = []
    for label, x, t in x0:
        jobs.append(Job(f"{name}[0]{label}", op(dz[0]), op(x), dz.shape[-1], x.shape[-1], dz[0].double(),
                        op(dtz[0]) if (two and t is not None) else None, op(t) if two else None))
    for i in range(1, n - 1):
        jobs.append(Job(f"{name}[{i}]", op(dz[i]), op(acts[i - 1]), dz.shape[-1], acts.shape[-1], dz[i].double(),
                        op(dtz[i]) if two else None, op(tacts[i - 1]) if two else None))
    jobs.append(Job(f"{name}[{n - 1}]", op(g_out), op(acts[n - 2]), g_out.shape[-1], acts.shape[-1], g_out.double(),
                    op(tg_out) if two else None, op(tacts[n - 2]) if two else None))
    return jobs


def bender_jobs(sixteen, p, lat, out):
    """The jobs of nrnerf_bender_wgrad in its order: network[0 .. depth-1], rigidity_network[0 .. rigidity_depth-1]; the first layers' inputs
    are the rows [point, latent code] / [point] formed from the ray records: p [M, 3] (points_fp32), lat [M, L] (per_sample)."""
    x0 = torch.cat([p, lat], 1)
    g = out["dz_out4"]
    return _chain_jobs("network", sixteen, [("", x0, None)], out["acts_offsets"], out["dz_offsets"], g[:, :3]) + \
        _chain_jobs("rigidity_network", sixteen, [("", p, None)], out["acts_rigidity"], out["dz_rigidity"], g[:, 3:4])


def divergence_jobs(sixteen, points, latents, probe, out):
    """The jobs of nrnerf_bender_divergence_backward: network[0] split into its point columns (second product: dtz_0^T probe) and its
    latent columns (one product), network[1 ..], rigidity_network[0 ..]; the second product dtz^T th goes into dW, not into db."""
    g, tg = out["dz_out4"], out["dtz_out4"]
    return _chain_jobs("network", sixteen, [(".point", points, probe), (".latent", latents, None)], out["acts_offsets"], out["dz_offsets"], g[:, :3],
                       probe, out["tacts_offsets"], out["dtz_offsets"], tg[:, :3]) + \
        _chain_jobs("rigidity_network", sixteen, [("", points, probe)], out["acts_rigidity"], out["dz_rigidity"], g[:, 3:4],
                    probe, out["tacts_rigidity"], out["dtz_rigidity"], tg[:, 3:4])


def partial_span(M, n_partials, sixteen):
    """Samples per wave, per the kernels' own split: the fp32 kernel splits PAIRS of samples, per = ceil(ceil(M / 2) / n_partials); the bf16
    kernel splits chunks of 16.  Partial k owns samples [k span, min((k + 1) span, M)) -- empty from ceil(M / span) on."""
    unit = 16 if sixteen else 2
    units = (M + unit - 1) // unit
    return ((units + n_partials - 1) // n_partials) * unit


def check_wgrad(rep, partials, jobs, M, n_partials, sixteen):
    """partials [n_partials, n_jobs, SLOT] fp32.  Per job: the partials added in float64 against dz^T x (+ dz2^T x2) and the column sums of
    dz over all M, bound = sum over the partials of (n_p + 3) U32 A_p, n_p the products a wave accumulates per element (its samples, twice
    with the second product); every meaningful element of every partial finite, an empty range's exactly 0.
    Returns {job name: (dW64, bound, db64, bound)}."""
    assert partials.shape == (n_partials, len(jobs), SLOT), (tuple(partials.shape), n_partials, len(jobs))
    span = partial_span(M, n_partials, sixteen)
    filled = (M + span - 1) // span
    last0 = (filled - 1) * span
    n_last = M - last0
    res = {}
    for j, jb in enumerate(jobs):
        P = partials[:, j]
        dWp, dbp = P[:, :4096].reshape(n_partials, 64, 64)[:, :jb.out, :jb.inn], P[:, 4096:4096 + jb.out]
        rep.exact(f"partials {jb.name}", bool(torch.isfinite(dWp).all() and torch.isfinite(dbp).all()), "a partial's slot was not written")
        rep.exact(f"partials {jb.name}", bool((dWp[filled:] == 0).all() and (dbp[filled:] == 0).all()), "the slot of an empty range is not exactly 0")
        passes = 2 if jb.dz2 is not None else 1
        want = jb.dz.T @ jb.x
        A = jb.dz.abs().T @ jb.x.abs()
        A_last = jb.dz[last0:].abs().T @ jb.x[last0:].abs()
        if passes == 2:
            want = want + jb.dz2.T @ jb.x2
            A = A + jb.dz2.abs().T @ jb.x2.abs()
            A_last = A_last + jb.dz2[last0:].abs().T @ jb.x2[last0:].abs()
        bound = U32 * ((passes * span + 3) * (A - A_last).clamp_min(0) + (passes * n_last + 3) * A_last) + passes * M * DENORM
        dW = dWp.double().sum(0)
        rep.add(f"dW {jb.name}", _ratio((dW - want).abs(), bound))
        want_b = jb.db_src.sum(0)
        Ab, Ab_last = jb.db_src.abs().sum(0), jb.db_src[last0:].abs().sum(0)
        bound_b = U32 * ((span + 3) * (Ab - Ab_last).clamp_min(0) + (n_last + 3) * Ab_last) + M * DENORM
        db = dbp.double().sum(0)
        rep.add(f"db {jb.name}", _ratio((db - want_b).abs(), bound_b))
        res[jb.name] = (dW, bound, db, bound_b)
    return res


def check_bender_wgrad(rb, sixteen, rays, z, latents, out, partials, n_partials, rep=None):
    """nrnerf_bender_wgrad from the arrays nrnerf_bender_forward / _backward wrote.  Returns (rep, results of check_wgrad)."""
    rep = rep or Report()
    M = z.shape[0] * z.shape[1]
    L = rb.network[0].weight.shape[1] - 3
    jobs = bender_jobs(sixteen, points_fp32(rays, z), per_sample(latents, z.shape[1], L), out)
    return rep, check_wgrad(rep, partials, jobs, M, n_partials, sixteen)


# ------------------------------------------------------------------------------------------------------------------------
# the same expressions evaluated end to end in float64 (tests/test_bender_reference_host.py holds them to torch autograd)
# ------------------------------------------------------------------------------------------------------------------------
def _mlp64(Ws, bs, x):
    acts, h = [], x.double()
    for i in range(len(Ws) - 1):
        h = torch.relu(h @ Ws[i].T + bs[i])
        acts.append(h)
    y = h @ Ws[-1].T
    return torch.stack(acts), (y if bs[-1] is None else y + bs[-1])


def forward64(w, p, lat):
    """acts_offsets, acts_rigidity, off4 = (offsets, tanh(logit)) in float64 from the point p [M,3] and the codes lat [M,L]"""
    acts_b, off = _mlp64(w["Wb"], w["bb"], torch.cat([p.double(), lat.double()], 1))
    acts_r, logit = _mlp64(w["Wr"], w["br"], p)
    return dict(acts_offsets=acts_b, acts_rigidity=acts_r, off4=torch.cat([off, torch.tanh(logit)], 1))


def tangent64(w, probe, acts_b, acts_r):
    """tacts_offsets, tacts_rigidity, toff4 in float64 from the saved activations' signs"""
    def chain(Ws, acts):
        t, keep = probe.double() @ Ws[0][:, :3].T, []
        for i in range(len(Ws) - 1):
            if i:
                t = t @ Ws[i].T
            t = torch.where(acts[i] > 0, t, torch.zeros_like(t))
            keep.append(t)
        return torch.stack(keep), t @ Ws[-1].T
    tb, toff = chain(w["Wb"], acts_b)
    tr, tl = chain(w["Wr"], acts_r)
    return dict(tacts_offsets=tb, tacts_rigidity=tr, toff4=torch.cat([toff, tl], 1))


def backward_chain64(Ws, g_out, acts):
    """[dz_0 .. dz_(n-2)] in float64 from the gradient wrt the MLP's outputs"""
    n, g, dz = len(Ws), g_out.double(), [None] * (len(Ws) - 1)
    for i in range(n - 1, 0, -1):
        g = g @ Ws[i]
        g = torch.where(acts[i - 1] > 0, g, torch.zeros_like(g))
        dz[i - 1] = g
    return torch.stack(dz)


def job_products64(jobs):
    """{job name: (dW, db)} in float64"""
    return {jb.name: (jb.dz.T @ jb.x + (jb.dz2.T @ jb.x2 if jb.dz2 is not None else 0.0), jb.db_src.sum(0)) for jb in jobs}


# ------------------------------------------------------------------------------------------------------------------------
# the fused use of the divergence backward against the separate pair
# ------------------------------------------------------------------------------------------------------------------------
def parameter_gradients(res, rb, split_first):
    """{parameter name: (gradient, bound)} from check_wgrad's results; split_first: network[0] came as a point job and a latent job"""
    out = {}
    for net, mlp in (("network", rb.network), ("rigidity_network", rb.rigidity_network)):
        for i, lin in enumerate(mlp):
            if net == "network" and i == 0 and split_first:
                a, b = res["network[0].point"], res["network[0].latent"]
                dW, bW, db, bb = torch.cat([a[0], b[0]], 1), torch.cat([a[1], b[1]], 1), b[2], b[3]
            else:
                dW, bW, db, bb = res[f"{net}[{i}]"]
            out[f"{net}.{i}.weight"] = (dW, bW)
            if lin.bias is not None:
                out[f"{net}.{i}.bias"] = (db, bb)
    return out


def _chain_gap(Ws, routes, head_gap, sixteen):
    """A-priori bound on |dz_first[i] - sum over the other routes of dz[i]| per element, hidden layers i = 0 .. n-2, for calls whose
    cotangents add up (routes: (g_out, acts, dz) per call; head_gap bounds the same difference of g_out).  The chains are linear where
    the relu masks agree: the gap of the layer above goes through |W|, and every route adds the bound its own layer is held to
    (_backward_chain).  Where the masks of two routes differ the stored magnitudes themselves are the bound."""
    n = len(Ws)
    gaps, gap_in = [None] * (n - 1), head_gap
    for i in range(n - 1, 0, -1):
        own = 0.0
        for g_out, acts, dz in routes:
            pre, _, B = _lin(g_out if i == n - 1 else dz[i], Ws[i].T, None, widen=sixteen and i < n - 1)
            own = own + (U16 * pre.abs() + (1 + U16) * B if sixteen else B)
        bits = [acts[i - 1] > 0 for _, acts, _ in routes]
        same = torch.ones_like(bits[0])
        for b in bits[1:]:
            same = same & (b == bits[0])
        lin = torch.where(bits[0], gap_in @ Ws[i].abs(), torch.zeros_like(own)) + own
        worst = sum(dz[i - 1].double().abs() for _, _, dz in routes)
        gaps[i - 1] = gap_in = torch.where(same, lin, worst)
    return gaps


def check_fused_against_pair(rep, rb, sixteen, knobs, points, lat, probe, g_divergence, render, fused, bender, alone):
    """The parameter and latent gradients of ONE nrnerf_bender_divergence_backward with the render pass' cotangents (fused) against the sum of
    nrnerf_bender_backward + nrnerf_bender_wgrad (bender) and nrnerf_bender_divergence_backward without them (alone) on the same samples.
    Each of fused / bender / alone: (out arrays, results of check_wgrad).  Bound: the three calls' own bounds, plus what their roundings
    can put between the stored gradients the products are taken of -- the heads' bounds carried down the (linear) chains, _chain_gap."""
    w = weights64(rb, points.device)
    (oF, rF), (oA, rA), (oB, rB) = fused, bender, alone
    hF, tF = divergence_head_backward(oF["off4"], oF["toff4"], probe, knobs, g_divergence, None, render)
    hB, tB = divergence_head_backward(oB["off4"], oB["toff4"], probe, knobs, g_divergence, None, None)
    hA = bender_head_backward(oA["off4"], oA["bent4"], knobs, render.get("g_bent4"), render.get("g_bent4_b"), render.get("g_unmasked"), render.get("g_mask"))
    gap_h = (hF.v - hA.v - hB.v).abs() + hF.e + hA.e + hB.e
    gap_t = (tF.v - tB.v).abs() + tF.e + tB.e
    op = lambda t: _operand(t, sixteen)
    x0 = torch.cat([points, lat], 1)
    extra = {}
    for net, key, nm, col in (("network", "Wb", "offsets", slice(0, 3)), ("rigidity_network", "Wr", "rigidity", slice(3, 4))):
        Ws, n = w[key], len(w[key])
        gz = _chain_gap(Ws, [(o["dz_out4"][:, col], o[f"acts_{nm}"], o[f"dz_{nm}"]) for o in (oF, oA, oB)], gap_h[:, col], sixteen)
        gt = _chain_gap(Ws, [(o["dtz_out4"][:, col], o[f"acts_{nm}"], o[f"dtz_{nm}"]) for o in (oF, oB)], gap_t[:, col], sixteen)
        top_z, top_t = gap_h[:, col], gap_t[:, col]
        if sixteen:                     # the heads' rows are rounded to bf16 for the products, each call's on its own
            top_z = top_z + U16 * sum(o["dz_out4"][:, col].double().abs() for o in (oF, oA, oB))
            top_t = top_t + U16 * sum(o["dtz_out4"][:, col].double().abs() for o in (oF, oB))
        for i in range(n):
            x_in = x0[:, :Ws[0].shape[1]] if i == 0 else None
            xF = op(x_in) if i == 0 else op(oF[f"acts_{nm}"][i - 1])
            xA = xF if i == 0 else op(oA[f"acts_{nm}"][i - 1])
            tx = op(probe) if i == 0 else op(oF[f"tacts_{nm}"][i - 1])
            dz_gap, dt_gap = (gz[i], gt[i]) if i < n - 1 else (top_z, top_t)
            dzA = op(oA[f"dz_{nm}"][i]) if i < n - 1 else op(oA["dz_out4"][:, col])
            eW = dz_gap.T @ xF.abs() + dzA.abs().T @ (xA - xF).abs()
            eW[:, :3] = eW[:, :3] + (dt_gap.T @ tx.abs() if i == 0 else 0.0)
            if i > 0:
                eW = eW + dt_gap.T @ tx.abs()
            bias_gap = gz[i] if i < n - 1 else gap_h[:, col]
            extra[f"{net}.{i}.weight"], extra[f"{net}.{i}.bias"] = eW, bias_gap.sum(0)
        if nm == "offsets":
            L = oF["d_latents"].shape[-1]
            lat_extra = gz[0] @ Ws[0][:, 3:3 + L].abs()
    rep.exact("fused vs pair", torch.equal(oF["acts_offsets"], oB["acts_offsets"]) and torch.equal(oF["off4"], oB["off4"]) and torch.equal(oF["toff4"], oB["toff4"]),
              "two divergence forwards of the same points differ")
    pF, pA, pB = parameter_gradients(rF, rb, True), parameter_gradients(rA, rb, False), parameter_gradients(rB, rb, True)
    for k in pF:
        diff = (pF[k][0] - pA[k][0] - pB[k][0]).abs()
        rep.add(f"fused vs pair {k}", _ratio(diff, pF[k][1] + pA[k][1] + pB[k][1] + extra[k]))
    bounds = [_latent_rows(Report(), w["Wb"][0], o["dz_offsets"][0], o["d_latents"], sixteen)[1] for o in (oF, oA, oB)]
    diff = (oF["d_latents"].double() - oA["d_latents"].double() - oB["d_latents"].double()).abs()
    rep.add("fused vs pair d_latents", _ratio(diff, sum(bounds) + lat_extra))
    return rep
