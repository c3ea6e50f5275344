"""CPU-tier checks of tests/inference_reference.py, the float64 model the GPU tests of the 16-bit inference trunks
(tests/test_inference_trunks.py) stand on:

1. the packed inference images of every family a GPU case uses hold exactly the operand values the model multiplies by (the module's
   weights rounded with torch), decoded through the register-dataflow emulation of tests/test_packing.py (``trunk_reference._Prober``: the
   32x32 images IMG_COARSE and IMG_COARSE_TRUNK), fragment by fragment in the order that file's emulations consume them (the 16x16x32 images
   IMG_*_TRUNK_X16 and IMG_GX_*) or layer by layer off the program (IMG_GEN_*) -- every family could be decoded;
2. the identity layers of a sandwich network are exact in the model; 3. every legitimate emulation lies inside the a-priori bound;
4. the bound is tight (median radius <= a tenth of the channel's standard deviation) for every GPU case; 5. each emulation passes the
   30 % / 3 x rule against the other four for every GPU case; 6. the acceptance functions reject deliberately wrong results.

A channel's standard deviation needs points to be taken over: the cases of fewer than 100 points ((1, 1) has none at all, (3, 5) fifteen
values) take it from the same network on the (37, 33) points, drawn from the same distribution.  The families behind a ray bender are held
here on the caller's points; on the GPU their trunk reads the bent ones, which the stress scene's bender moves within the same volume."""
import functools

import pytest
import torch

from nonrigid_nerf_amd.synthetic import build_modules
from tests import inference_reference as I
from tests import trunk_reference as T

ALL_FAMILIES = list(I.FAMILIES) + [I.VIEWS_FAMILY[0]]


def _spec(family):
    return I.VIEWS_FAMILY[1] if family == I.VIEWS_FAMILY[0] else I.FAMILIES[family]


@functools.lru_cache(maxsize=None)
def _net(family, live=None):
    cfg, scene = I.family_scene(family, live)
    _, coarse, _ = build_modules(scene)
    coarse.requires_grad_(False)
    return cfg, coarse


@functools.lru_cache(maxsize=None)
def _ops(family, live, precision):
    return I.operands(_net(family, live)[1], precision)


# ---- 1. the packed images hold the model's operands ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", I.PRECISIONS)
@pytest.mark.parametrize("family", ALL_FAMILIES)
def test_packed_inference_images_hold_the_models_operands(family, precision):
    cfg, net = _net(family)
    ops = I.operands(net, precision)
    _, _, _, which, decoder = _spec(family)
    D, W, L, n_enc = cfg.netdepth, cfg.netwidth, cfg.multires, cfg.input_ch
    skip = cfg.skips[0] if cfg.skips else -1
    och = cfg.output_ch

    def same_padded(got_w, got_b, want_w, want_b, n_lead):
        """rows / hidden columns beyond the network's are the width class' padding: zero"""
        ow, hid = want_w.shape[0], want_w.shape[1] - n_lead
        assert torch.equal(got_b[:ow], want_b) and not got_b[ow:].any()
        assert torch.equal(got_w[:ow, :n_lead], want_w[:, :n_lead]) and not got_w[ow:].any()
        assert torch.equal(got_w[:ow, n_lead:n_lead + hid], want_w[:, n_lead:]) and not got_w[:, n_lead + hid:].any()

    if decoder == "mb":
        image = T._pack_image(net, None, precision, which)
        Ws, bs, head, alpha, vw, rgb = T.probe_forward_image(image, precision, D, W, L, cfg.multires_views, skip, cfg.use_viewdirs)
        for i in range(D):
            assert torch.equal(Ws[i], ops.W[i]) and torch.equal(bs[i], ops.b[i]), i
        if cfg.use_viewdirs:
            n_dir = 3 + 6 * cfg.multires_views
            assert torch.equal(alpha[0], ops.alpha[0]) and torch.equal(alpha[1], ops.alpha[1])
            assert torch.equal(vw[0][:, :n_dir], ops.views[0]) and torch.equal(vw[0][:, n_dir:], ops.views[1]) and torch.equal(vw[1], ops.views[2])
            assert torch.equal(rgb[0], ops.rgb[0]) and torch.equal(rgb[1], ops.rgb[1])
        else:
            assert torch.equal(head[0][:och], ops.head[0]) and torch.equal(head[1][:och], ops.head[1])
    elif decoder in ("x16", "gx"):
        layers, head = T.frag16_image_operands(T._pack_image(net, None, precision, which), precision, W, D, L, skip, decoder)
        for i in range(D):
            same_padded(*layers[i], ops.W[i], ops.b[i], n_enc if ops.reads_enc[i] else 0)
        same_padded(*head, ops.head[0], ops.head[1], 0)
    else:
        prog = T.generic_program_operands(T._pack_image(net, None, precision, which, with_units=True), precision)
        assert len(prog) == D + 1
        for i in range(D):
            ly = prog[i]
            assert ly["relu"] and ly["dst"] == 1 and set(ly["W"]) == ({0} if i == 0 else ({0, 1} if ops.reads_enc[i] else {1}))
            got = torch.cat(([ly["W"][0][:, :n_enc]] if ops.reads_enc[i] else []) + ([ly["W"][1][:, :W]] if i else []), 1)
            assert not (ops.reads_enc[i] and ly["W"][0][:, n_enc:].any()) and not (i and ly["W"][1][:, W:].any())
            same_padded(got, ly["b"], ops.W[i], ops.b[i], 0)
        ly = prog[D]
        assert not ly["relu"] and ly["dst"] != 1 and ly["o_col"] == 0 and ly["o_rows"] == och and set(ly["W"]) == {1}
        assert not ly["W"][1][:, W:].any()
        same_padded(ly["W"][1][:, :W], ly["b"], ops.head[0], ops.head[1], 0)


# ---- 2.-4. the sandwiches ------------------------------------------------------------------------------------------------------------------
def _sandwich_cases():
    for family, (kw, *_rest) in I.FAMILIES.items():
        cfg = I.family_config(family)
        for live in I.live_sets(cfg.netdepth, cfg.skips):
            for precision in I.PRECISIONS:
                yield family, live, precision


SANDWICH_CASES = list(_sandwich_cases())
_ids = lambda c: f"{c[0]}-live{'_'.join(map(str, c[1]))}-{c[2]}"


@functools.lru_cache(maxsize=None)
def _spread(family, live, precision):
    """the channels' standard deviation of the sandwich on the (37, 33) points"""
    centre, _ = I.interval_bound(_net(family, live)[1], live, I.case_points((37, 33)), precision, ops=_ops(family, live, precision))
    return centre.reshape(-1, centre.shape[-1]).std(0)


@pytest.mark.parametrize("case", SANDWICH_CASES, ids=_ids)
def test_sandwich_bound_is_exact_on_identity_layers_holds_every_emulation_and_is_tight(case):
    family, live, precision = case
    cfg, net = _net(family, live)
    ops = _ops(family, live, precision)
    worst_cap = worst_ratio = 0.0
    for shape in I.SANDWICH_SHAPES:
        pts = I.case_points(shape)
        # 2. the identity layers are exact: all layers == the live ones alone, bit for bit
        full = I.model64(net, pts, precision, ops=ops)
        assert torch.equal(full, I.model64(net, pts, precision, ops=ops, layers=list(live))), shape
        centre, radius = I.interval_bound(net, live, pts, precision, ops=ops)
        assert bool(((full - centre).abs() <= radius).all()), shape         # (the model is itself a rounding the bound admits)
        # 4. the bound is tight
        c2, r2 = centre.reshape(-1, centre.shape[-1]), radius.reshape(-1, radius.shape[-1])
        std = c2.std(0) if c2.shape[0] >= 100 else _spread(family, live, precision)
        share = r2.median(0).values / std
        worst_cap = max(worst_cap, float(share.max()))
        assert bool((share <= I.RADIUS_CAP).all()), (shape, share.tolist())
        # 3. every legitimate emulation lies inside
        for seed in I.EMULATION_SEEDS:
            fails, ratio = I.interval_failures(I.emulation(net, pts, precision, seed, ops=ops), centre, radius)
            worst_ratio = max(worst_ratio, ratio)
            assert not fails, (shape, seed, fails)
    print(f"\n[{_ids(case)}] worst emulation residual / bound {worst_ratio:.3f}; worst median radius / std {worst_cap:.4f}")


# ---- 5. full networks: the reference alone stays inside its own rule -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full(family, precision, shape):
    cfg, net = _net(family)
    ops = _ops(family, None, precision)
    pts = I.case_points(shape)
    dirs = I.case_dirs(shape)[:, None, :].expand(-1, shape[1], -1) if cfg.use_viewdirs else None
    model = I.model64(net, pts, precision, dirs, ops=ops)
    emus = [I.emulation(net, pts, precision, seed, dirs, ops=ops) for seed in I.EMULATION_SEEDS]
    return net, ops, pts, dirs, model, emus


@pytest.mark.parametrize("shape", I.FULL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", I.PRECISIONS)
@pytest.mark.parametrize("family", ALL_FAMILIES)
def test_each_emulation_passes_the_rule_against_the_other_four(family, precision, shape):
    net, ops, pts, dirs, model, emus = _full(family, precision, shape)
    worst = (0.0, 0.0)
    for k, e in enumerate(emus):
        fails, rms, mx = I.rule_failures(e, model, emus[:k] + emus[k + 1:])
        worst = (max(worst[0], rms), max(worst[1], mx))
        assert not fails, (k, fails)
    exact = I.exact64(net, pts, dirs)
    print(f"\n[{family} / {precision} / {shape}] leave-one-out: worst rms ratio {worst[0]:.3f}, worst max ratio {worst[1]:.3f}; "
          f"rms(emulation - exact64) / rms(model64 - exact64) {I.budget_share(emus[0], model, exact):.3f}")


# ---- 6. the acceptance functions reject wrong results -----------------------------------------------------------------------------------
WRONG = [("x16_w256", "bf16"), ("gx_d5_w96", "f16")]


@pytest.mark.parametrize("family,precision", WRONG)
def test_truncating_conversions_fail_the_rule(family, precision):
    net, ops, pts, dirs, model, emus = _full(family, precision, (37, 33))
    fails, rms, mx = I.rule_failures(I.emulation(net, pts, precision, 99, ops=ops, rounding="truncate"), model, emus)
    print(f"\n[{family} / {precision}] truncation: rms ratio {rms:.2f}, max ratio {mx:.2f}")
    assert fails


def _sandwich_setup(family, precision):
    cfg = I.family_config(family)
    live = I.live_sets(cfg.netdepth, cfg.skips)[-1]
    _, net = _net(family, live)
    ops = _ops(family, live, precision)
    pts = I.case_points((37, 33))
    return net, ops, live, pts, I.interval_bound(net, live, pts, precision, ops=ops)


@pytest.mark.parametrize("family,precision", WRONG)
def test_one_sample_replaced_by_another_fails_both_checks(family, precision):
    net, ops, live, pts, (centre, radius) = _sandwich_setup(family, precision)
    assert not I.interval_failures(I.emulation(net, pts, precision, 5, ops=ops), centre, radius)[0]
    assert I.interval_failures(I.emulation(net, pts, precision, 5, ops=ops, garbage=(20, 17)), centre, radius)[0]
    net, ops, pts, dirs, model, emus = _full(family, precision, (37, 33))
    fails, rms, mx = I.rule_failures(I.emulation(net, pts, precision, 99, ops=ops, garbage=(20, 17)), model, emus)
    print(f"\n[{family} / {precision}] one sample replaced: rms ratio {rms:.2f}, max ratio {mx:.2f}")
    assert any("max deviation" in f for f in fails), fails


@pytest.mark.parametrize("family,precision", WRONG)
def test_a_dropped_bias_fails_both_checks(family, precision):
    net, ops, live, pts, (centre, radius) = _sandwich_setup(family, precision)
    assert I.interval_failures(I.emulation(net, pts, precision, 5, ops=ops, drop_bias=live[-1]), centre, radius)[0]
    net, ops, pts, dirs, model, emus = _full(family, precision, (37, 33))
    fails, rms, mx = I.rule_failures(I.emulation(net, pts, precision, 99, ops=ops, drop_bias=2), model, emus)
    print(f"\n[{family} / {precision}] hidden layer 2 without its bias: rms ratio {rms:.2f}, max ratio {mx:.2f}")
    assert fails
