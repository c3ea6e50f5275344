"""tests/bender_reference.py proved before it judges a kernel (no GPU).

1. Its expressions, evaluated end to end in float64, are torch autograd's: the same ray_bending module in float64 gives the three outputs,
   `.backward()` on random cotangents the parameter and latent gradients, and the divergence (and the tangent J e) with their gradients
   come from create_graph=True as oracle/nrnerf_oracle.py's compute_divergence_loss forms them -- all within 1e-12 relative, both bender
   depths, with and without each knob, with and without the render pass' cotangents.
2. Fed its own float64 results cast to the kernels' storage types (fp32; bf16 saved arrays for a bf16 model) as "kernel output", every
   check_* passes.
3. Each check_* rejects a planted error: one activation of one layer off by 4 B, one dz element nonzero under a dead relu, one partial slot
   left NaN, one dW entry off by 4 x its bound, bent4 off by one ulp.
4. check_fused_against_pair holds on the reference's own results and rejects a pair that does not add up."""
import pytest
import torch
import torch.nn.functional as F

from nonrigid_nerf_amd.synthetic import SceneConfig, build_modules, make_rays, make_scene
from tests import bender_reference as BR

f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))           # the knobs reach the kernels as fp32 numbers
KNOBS = {"plain": BR.Knobs(), "cutoff_scaling": BR.Knobs(f32(0.58), f32(0.7)), "scaling": BR.Knobs(None, f32(0.7))}
N, S = 7, 9


def _bender(depth):
    scene = make_scene(SceneConfig(N_importance=64, bend_depth=depth), 2)
    rb = build_modules(scene)[0]
    with torch.no_grad():                      # masks around 0.5, so that the cutoff bites
        rb.rigidity_network[-1].weight.mul_(0.02)
        rb.rigidity_network[-1].bias.zero_()
    return rb.requires_grad_(True)


def _inputs(seed=3):
    gen = torch.Generator().manual_seed(seed)
    rays, latents = make_rays(N, 5)
    z = (2.0 + 4.0 * torch.rand(N, S, generator=gen)).sort(-1).values
    M = N * S
    g = dict(g_bent4=torch.randn(M, 4, generator=gen), g_bent4_b=torch.randn(M, 4, generator=gen), g_unmasked=torch.randn(M, 3, generator=gen),
             g_mask=torch.randn(M, generator=gen))
    probe = torch.randn(M, 3, generator=gen)
    g_div, g_tan = torch.randn(M, generator=gen), torch.randn(M, 3, generator=gen)
    return rays, latents, z, g, probe, g_div, g_tan


def module_forward(rb, p, lat, knobs):
    """ray_bending.forward (run_nerf_helpers.py:507-577) on the module's layers, under autograd"""
    h = torch.cat([p, lat], -1)
    for i, lin in enumerate(rb.network):
        h = lin(h)
        if i != len(rb.network) - 1:
            h = F.relu(h)
    r = p
    for i, lin in enumerate(rb.rigidity_network):
        r = lin(r)
        if i != len(rb.rigidity_network) - 1:
            r = F.relu(r)
    mask = (torch.tanh(r) + 1) / 2
    if knobs.cutoff is not None:
        mask = torch.where(mask <= knobs.cutoff, torch.zeros_like(mask), mask)
    masked = mask * h
    if knobs.scaling is not None:
        masked = masked * knobs.scaling
    return p + masked, h, mask[:, 0], masked


def close(got, want, what):
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1e-30), (what, float((got - want).abs().max()), scale)


def bent64(p, off4, knobs):
    mask, _ = BR.mask_fp32(off4[:, 3], knobs)
    mo = mask[:, None] * off4[:, :3] * (1.0 if knobs.scaling is None else knobs.scaling)
    return torch.cat([p + mo, mask[:, None]], 1)


def param_grads(rb, products, split_first):
    """{parameter name: gradient} from job_products64's {job: (dW, db)}"""
    out = {}
    for net, mlp in (("network", rb.network), ("rigidity_network", rb.rigidity_network)):
        for i, lin in enumerate(mlp):
            if net == "network" and i == 0 and split_first:
                dW = torch.cat([products["network[0].point"][0], products["network[0].latent"][0]], 1)
                db = products["network[0].latent"][1]
                close(products["network[0].point"][1], db, "both jobs of network[0] carry its db")
            else:
                dW, db = products[f"{net}[{i}]"]
            out[f"{net}.{i}.weight"] = dW
            if lin.bias is not None:
                out[f"{net}.{i}.bias"] = db
    return out


def _zero_grads(rb):
    for p in rb.parameters():
        p.grad = None


@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
@pytest.mark.parametrize("depth", [5, 7])
def test_float64_bender_expressions_are_autograds(depth, knobs):
    kn = KNOBS[knobs]
    rb = _bender(depth).double()
    rays, latents, z, g, _, _, _ = _inputs()
    rays, z, g = rays.double(), z.double(), {k: v.double() for k, v in g.items()}
    p = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    lat = latents.double().requires_grad_(True)
    _zero_grads(rb)
    bent, off, mask, _ = module_forward(rb, p, BR.per_sample(lat, S, 32), kn)
    gb = g["g_bent4"][:, :3] + g["g_bent4_b"][:, :3]
    ((bent * gb).sum() + (off * g["g_unmasked"]).sum() + (mask * g["g_mask"]).sum()).backward()

    w = BR.weights64(rb)
    lat_s = BR.per_sample(latents.double(), S, 32)
    out = BR.forward64(w, p, lat_s)
    out["bent4"] = bent64(p, out["off4"], kn)
    close(out["bent4"][:, :3], bent.detach(), "bent")
    close(out["off4"][:, :3], off.detach(), "offsets")
    close(out["bent4"][:, 3], mask.detach(), "mask")
    if kn.cutoff is not None:
        assert float((mask == 0).double().mean()) > 0.02
    head = BR.bender_head_backward(out["off4"], out["bent4"], kn, g["g_bent4"], g["g_bent4_b"], g["g_unmasked"], g["g_mask"])
    out["dz_out4"] = head.v
    out["dz_offsets"] = BR.backward_chain64(w["Wb"], head.v[:, :3], out["acts_offsets"])
    out["dz_rigidity"] = BR.backward_chain64(w["Wr"], head.v[:, 3:4], out["acts_rigidity"])
    d_lat = out["dz_offsets"][0] @ w["Wb"][0][:, 3:]
    close(d_lat.view(N, S, -1).sum(1), lat.grad, "latents")
    grads = param_grads(rb, BR.job_products64(BR.bender_jobs(False, p, lat_s, out)), False)
    named = dict(rb.named_parameters())
    assert set(grads) == set(named)
    for k, v in grads.items():
        close(v, named[k].grad, k)


@pytest.mark.parametrize("render", [False, True], ids=["alone", "with_render_cotangents"])
@pytest.mark.parametrize("mode", ["divergence", "tangent"])
@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
@pytest.mark.parametrize("depth", [5, 7])
def test_float64_divergence_expressions_are_autograds_double_backward(depth, knobs, mode, render):
    kn = KNOBS[knobs]
    rb = _bender(depth).double()
    rays, latents, z, g, probe, g_div, g_tan = _inputs()
    g, probe, g_div, g_tan = {k: v.double() for k, v in g.items()}, probe.double(), g_div.double(), g_tan.double()
    p = BR.points_fp32(rays, z).double()
    M = p.shape[0]
    _zero_grads(rb)
    pts = p.clone().requires_grad_(True)                                            # rnh:39
    lat = torch.randn(M, 32, generator=torch.Generator().manual_seed(9), dtype=torch.float64).mul(0.1).requires_grad_(True)
    bent, off, mask, masked = module_forward(rb, pts, lat, kn)
    u = torch.zeros(M, 3, dtype=torch.float64, requires_grad=True)
    e_dydx = torch.autograd.grad(masked, pts, probe, create_graph=True)[0]          # rnh:107-109: J^T e
    div = (e_dydx * probe).sum(1)                                                   # rnh:110-112
    jt_u = torch.autograd.grad(masked, pts, u, create_graph=True)[0]
    je = torch.autograd.grad(jt_u, u, probe, create_graph=True)[0]                  # J e: the derivative of J^T u along u
    loss = (div * g_div).sum() if mode == "divergence" else (je * g_tan).sum()
    if render:
        loss = loss + (bent * (g["g_bent4"][:, :3] + g["g_bent4_b"][:, :3])).sum() + (off * g["g_unmasked"]).sum() + (mask * g["g_mask"]).sum()
    loss.backward()

    w = BR.weights64(rb)
    out = BR.forward64(w, p, lat.detach())
    out.update(BR.tangent64(w, probe, out["acts_offsets"], out["acts_rigidity"]))
    d, tv = BR.divergence_head_forward(out["off4"], out["toff4"], probe, kn)
    close(d.v, div.detach(), "divergence")
    close(tv.v, je.detach(), "tangent")
    close(bent64(p, out["off4"], kn)[:, :3], bent.detach(), "bent")
    hz, htz = BR.divergence_head_backward(out["off4"], out["toff4"], probe, kn, g_div if mode == "divergence" else None,
                                          g_tan if mode == "tangent" else None, g if render else None)
    out["dz_out4"], out["dtz_out4"] = hz.v, htz.v
    for nm, key in (("offsets", "Wb"), ("rigidity", "Wr")):
        col = slice(0, 3) if nm == "offsets" else slice(3, 4)
        out[f"dz_{nm}"] = BR.backward_chain64(w[key], hz.v[:, col], out[f"acts_{nm}"])
        out[f"dtz_{nm}"] = BR.backward_chain64(w[key], htz.v[:, col], out[f"acts_{nm}"])
    close(out["dz_offsets"][0] @ w["Wb"][0][:, 3:], lat.grad, "latents")
    grads = param_grads(rb, BR.job_products64(BR.divergence_jobs(False, p, lat.detach(), probe, out)), True)
    named = dict(rb.named_parameters())
    assert set(grads) == set(named)
    for k, v in grads.items():
        close(v, named[k].grad, k)


# ---- the checks on the reference's own results in the kernels' storage types -----------------------------------------------------------
def emulate_partials(jobs, M, n_partials, sixteen):
    """what bend_wgrad / bend_wgrad16 promise: one fp32 partial per wave and job over the wave's own range of samples"""
    span = BR.partial_span(M, n_partials, sixteen)
    P = torch.zeros(n_partials, len(jobs), BR.SLOT)
    for k in range(n_partials):
        s = slice(min(k * span, M), min((k + 1) * span, M))
        for j, jb in enumerate(jobs):
            dW = jb.dz[s].T @ jb.x[s]
            if jb.dz2 is not None:
                dW = dW + jb.dz2[s].T @ jb.x2[s]
            slot = torch.zeros(64, 64, dtype=torch.float64)
            slot[:jb.out, :jb.inn] = dW
            P[k, j, :4096] = slot.reshape(-1).float()
            P[k, j, 4096:4096 + jb.out] = jb.db_src[s].sum(0).float()
    return P


def bender_call(depth, kn, sixteen, n_partials=8):
    """(rb, inputs, out, partials) of an emulated nrnerf_bender_forward / _backward / _wgrad: every array the float64 value of the layer
    evaluated FROM THE STORED INPUT, as a kernel would, cast to its storage type"""
    sa = torch.bfloat16 if sixteen else torch.float32
    rb = _bender(depth)
    rays, latents, z, g, _, _, _ = _inputs()
    w = BR.weights64(rb)
    p, lat_s = BR.points_fp32(rays, z), BR.per_sample(latents, S, 32)
    f = BR.forward64(w, p, lat_s)
    out = dict(acts_offsets=f["acts_offsets"].to(sa), acts_rigidity=f["acts_rigidity"].to(sa), off4=f["off4"].float())
    out["bent4"] = BR.bent4_expected(p, out["off4"], kn)
    head = BR.bender_head_backward(out["off4"], out["bent4"], kn, g["g_bent4"], g["g_bent4_b"], g["g_unmasked"], g["g_mask"])
    out["dz_out4"] = head.v.float()
    dzb = BR.backward_chain64(w["Wb"], out["dz_out4"][:, :3], out["acts_offsets"])
    dzr = BR.backward_chain64(w["Wr"], out["dz_out4"][:, 3:4], out["acts_rigidity"])
    out.update(dz_offsets=dzb.to(sa), dz_rigidity=dzr.to(sa), d_latents=(dzb[0] @ w["Wb"][0][:, 3:]).float())
    partials = emulate_partials(BR.bender_jobs(sixteen, p, lat_s, out), N * S, n_partials, sixteen)
    return rb, (rays, latents, z, g), out, partials


def run_bender_checks(rb, kn, sixteen, inputs, out, partials, n_partials=8):
    rays, latents, z, g = inputs
    rep = BR.check_bender_forward(rb, sixteen, kn, rays, z, latents, out)
    BR.check_bender_backward(rb, sixteen, kn, out, g["g_bent4"], g["g_bent4_b"], g["g_unmasked"], g["g_mask"], rep=rep)
    _, res = BR.check_bender_wgrad(rb, sixteen, rays, z, latents, out, partials, n_partials, rep=rep)
    return rep, res


@pytest.mark.parametrize("n_partials", [4, 8, 64])
@pytest.mark.parametrize("sixteen", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
@pytest.mark.parametrize("depth", [5, 7])
def test_bender_checks_pass_on_the_references_own_results(depth, knobs, sixteen, n_partials):
    rb, inputs, out, partials = bender_call(depth, KNOBS[knobs], sixteen, n_partials)
    rep, _ = run_bender_checks(rb, KNOBS[knobs], sixteen, inputs, out, partials, n_partials)
    assert not rep.failures, rep.failures
    assert rep.worst("") <= 1.0 and rep.tanh_share < 1.0


def divergence_call(depth, kn, sixteen, mode, render, stride0=False, n_partials=8):
    sa = torch.bfloat16 if sixteen else torch.float32
    rb = _bender(depth)
    rays, latents, z, g, probe, g_div, g_tan = _inputs()
    w = BR.weights64(rb)
    p = BR.points_fp32(rays, z)
    M = p.shape[0]
    lat = latents[:1].expand(M, 32).contiguous() if stride0 else BR.per_sample(latents, S, 32).contiguous()
    f = BR.forward64(w, p, lat)
    out = dict(acts_offsets=f["acts_offsets"].to(sa), acts_rigidity=f["acts_rigidity"].to(sa), off4=f["off4"].float())
    t = BR.tangent64(w, probe, out["acts_offsets"], out["acts_rigidity"])
    out.update(tacts_offsets=t["tacts_offsets"].to(sa), tacts_rigidity=t["tacts_rigidity"].to(sa), toff4=t["toff4"].float())
    d, tv = BR.divergence_head_forward(out["off4"], out["toff4"], probe, kn)
    out.update(divergence=d.v.float(), tangent=tv.v.float(), bent4=BR.bent4_expected(p, out["off4"], kn))
    cot = dict(g_divergence=g_div if mode == "divergence" else None, g_tangent=g_tan if mode == "tangent" else None, render=g if render else None)
    hz, htz = BR.divergence_head_backward(out["off4"], out["toff4"], probe, kn, **cot)
    out.update(dz_out4=hz.v.float(), dtz_out4=htz.v.float())
    for nm, key in (("offsets", "Wb"), ("rigidity", "Wr")):
        col = slice(0, 3) if nm == "offsets" else slice(3, 4)
        dz = BR.backward_chain64(w[key], out["dz_out4"][:, col], out[f"acts_{nm}"])
        out[f"dz_{nm}"] = dz.to(sa)
        out[f"dtz_{nm}"] = BR.backward_chain64(w[key], out["dtz_out4"][:, col], out[f"acts_{nm}"]).to(sa)
        if nm == "offsets":
            out["d_latents"] = (dz[0] @ w["Wb"][0][:, 3:]).float()
    partials = emulate_partials(BR.divergence_jobs(sixteen, p, lat, probe, out), M, n_partials, sixteen)
    return rb, (p, lat, probe, cot), out, partials


@pytest.mark.parametrize("render", [False, True], ids=["alone", "with_render_cotangents"])
@pytest.mark.parametrize("mode", ["divergence", "tangent"])
@pytest.mark.parametrize("sixteen", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
@pytest.mark.parametrize("depth", [5, 7])
def test_divergence_checks_pass_on_the_references_own_results(depth, knobs, sixteen, mode, render):
    kn = KNOBS[knobs]
    rb, (p, lat, probe, cot), out, partials = divergence_call(depth, kn, sixteen, mode, render, stride0=(mode == "tangent"))
    rep = BR.check_divergence_forward(rb, sixteen, kn, p, lat, probe, out)
    BR.check_divergence_backward(rb, sixteen, kn, p, lat, probe, out, partials=partials, n_partials=8, rep=rep, **cot)
    assert not rep.failures, rep.failures


# ---- planted errors ----------------------------------------------------------------------------------------------------------------------
KN = KNOBS["cutoff_scaling"]


def _rejected(rep, name):
    assert any(f.startswith(name) for f in rep.failures), (name, rep.failures)


def test_an_activation_off_by_four_bounds_is_rejected():
    rb, inputs, out, partials = bender_call(5, KN, False)
    w = BR.weights64(rb)
    pre, _, B = BR._lin(out["acts_offsets"][1], w["Wb"][2], w["bb"][2])
    m, f = [int(v) for v in (pre > 4 * B).nonzero()[0]]
    out["acts_offsets"][2, m, f] = float(pre[m, f] + 4 * B[m, f])
    _rejected(BR.check_bender_forward(rb, False, KN, inputs[0], inputs[2], inputs[1], out), "acts_offsets[2]")
    rb, (p, lat, probe, cot), out, partials = divergence_call(5, KN, False, "divergence", True)
    pre, _, B = BR._lin(out["tacts_rigidity"][0], w["Wr"][1], None)
    m, f = [int(v) for v in (out["acts_rigidity"][1] > 0).nonzero()[0]]
    out["tacts_rigidity"][1, m, f] = float(pre[m, f] + 4 * B[m, f])
    _rejected(BR.check_divergence_forward(rb, False, KN, p, lat, probe, out), "tacts_rigidity[1]")


@pytest.mark.parametrize("sixteen", [False, True], ids=["f32", "bf16"])
def test_a_gradient_under_a_dead_relu_is_rejected(sixteen):
    rb, inputs, out, partials = bender_call(5, KN, sixteen)
    m, f = [int(v) for v in (out["acts_offsets"][1] <= 0).nonzero()[0]]
    out["dz_offsets"][1, m, f] = 1e-30
    g = inputs[3]
    _rejected(BR.check_bender_backward(rb, sixteen, KN, out, g["g_bent4"], g["g_bent4_b"], g["g_unmasked"], g["g_mask"]), "dz_offsets[1]")
    rb, (p, lat, probe, cot), out, partials = divergence_call(5, KN, sixteen, "divergence", False)
    m, f = [int(v) for v in (out["acts_rigidity"][0] <= 0).nonzero()[0]]
    out["dtz_rigidity"][0, m, f] = -1e-30
    rep, _ = BR.check_divergence_backward(rb, sixteen, KN, p, lat, probe, out, **cot)
    _rejected(rep, "dtz_rigidity[0]")


@pytest.mark.parametrize("sixteen", [False, True], ids=["f32", "bf16"])
def test_a_partial_slot_left_unwritten_or_an_empty_one_not_zero_is_rejected(sixteen):
    rb, inputs, out, partials = bender_call(5, KN, sixteen, 64)
    bad = partials.clone()
    bad[63, 2, 64 * 5 + 7] = float("nan")
    rep, _ = run_bender_checks(rb, KN, sixteen, inputs, out, bad, 64)
    _rejected(rep, "partials network[2]")
    span = BR.partial_span(N * S, 64, sixteen)
    assert span * 63 >= N * S, "the last partial's range is empty"
    bad = partials.clone()
    bad[63, 6, 4096] = 1e-20
    rep, _ = run_bender_checks(rb, KN, sixteen, inputs, out, bad, 64)
    _rejected(rep, "partials rigidity_network[1]")


@pytest.mark.parametrize("sixteen", [False, True], ids=["f32", "bf16"])
def test_a_weight_gradient_off_by_four_bounds_is_rejected(sixteen):
    rb, inputs, out, partials = bender_call(5, KN, sixteen)
    rep, res = run_bender_checks(rb, KN, sixteen, inputs, out, partials)
    assert not rep.failures, rep.failures
    bad = partials.clone()
    bad[1, 3, 64 * 11 + 13] += float(4 * res["network[3]"][1][11, 13])
    _rejected(run_bender_checks(rb, KN, sixteen, inputs, out, bad)[0], "dW network[3]")
    bad = partials.clone()
    bad[0, 5, 4096 + 2] += float(4 * res["rigidity_network[0]"][3][2])
    _rejected(run_bender_checks(rb, KN, sixteen, inputs, out, bad)[0], "db rigidity_network[0]")
    rb, (p, lat, probe, cot), out, partials = divergence_call(5, KN, sixteen, "divergence", True)
    rep, res = BR.check_divergence_backward(rb, sixteen, KN, p, lat, probe, out, partials=partials, n_partials=8, **cot)
    assert not rep.failures, rep.failures
    partials[2, 0, 64 * 9 + 1] += float(4 * res["network[0].point"][1][9, 1])
    rep, _ = BR.check_divergence_backward(rb, sixteen, KN, p, lat, probe, out, partials=partials, n_partials=8, **cot)
    _rejected(rep, "dW network[0].point")


def test_bent4_off_by_one_ulp_is_rejected():
    rb, inputs, out, partials = bender_call(5, KN, False)
    out["bent4"].view(torch.int32)[5, 1] += 1
    _rejected(BR.check_bender_forward(rb, False, KN, inputs[0], inputs[2], inputs[1], out), "bent4")
    rb, (p, lat, probe, cot), out, partials = divergence_call(5, KN, False, "divergence", False)
    out["bent4"].view(torch.int32)[11, 3] += 1
    _rejected(BR.check_divergence_forward(rb, False, KN, p, lat, probe, out), "bent4")


def test_a_head_gradient_that_ignores_the_cutoff_is_rejected():
    rb, inputs, out, partials = bender_call(5, KN, False)
    _, cut = BR.mask_fp32(out["off4"][:, 3], KN)
    out["dz_out4"][int(cut.nonzero()[0]), 3] = 1e-30
    g = inputs[3]
    _rejected(BR.check_bender_backward(rb, False, KN, out, g["g_bent4"], g["g_bent4_b"], g["g_unmasked"], g["g_mask"]), "dz_out4")


# ---- the fused use of the divergence backward against the separate pair ------------------------------------------------------------------
def _three_routes(kn, sixteen, scale_pair=1.0):
    rb, inputs, oA, pA = bender_call(5, kn, sixteen)
    repA, rA = run_bender_checks(rb, kn, sixteen, inputs, oA, pA * scale_pair)
    rb, (p, lat, probe, cotF), oF, pF = divergence_call(5, kn, sixteen, "divergence", True)
    repF, rF = BR.check_divergence_backward(rb, sixteen, kn, p, lat, probe, oF, partials=pF, n_partials=8, **cotF)
    rb, (_, _, _, cotB), oB, pB = divergence_call(5, kn, sixteen, "divergence", False)
    repB, rB = BR.check_divergence_backward(rb, sixteen, kn, p, lat, probe, oB, partials=pB, n_partials=8, **cotB)
    return BR.check_fused_against_pair(BR.Report(), rb, sixteen, kn, p, lat, probe, cotF["g_divergence"], cotF["render"], (oF, rF), (oA, rA), (oB, rB))


@pytest.mark.parametrize("sixteen", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
def test_fused_divergence_backward_adds_up_to_the_separate_pair(knobs, sixteen):
    rep = _three_routes(KNOBS[knobs], sixteen)
    assert not rep.failures, rep.failures
    assert len(rep.ratio) == len(list(_bender(5).parameters())) + 1 and rep.worst("fused vs pair") <= 1.0


def test_a_pair_that_does_not_add_up_to_the_fused_call_is_rejected():
    rep = _three_routes(KN, False, scale_pair=1.0 + 1e-4)
    _rejected(rep, "fused vs pair network")
