"""free_viewpoint_rendering.py's (fvr) per-frame images and scores on the device (nonrigid_nerf_amd.visualize, C ABI 9).

CPU tier: this file's own torch restatements of the maps and scores (in numpy's dtypes; SSIM in float64) reproduce the fixture
tests/golden/visualize/visualize_96x72.npz (written by tools/make_visualization_golden.py from the reference's own functions), the ABI structures
match their ctypes mirror, and render_path's default return values are unchanged.  GPU tier: the kernels against the fixture and the
restatements, at the fixture's size and at 2x3, 17x31, 384x512 and 1080x1920."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from nonrigid_nerf_amd import _lib
from nonrigid_nerf_amd import visualize as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
DEV = "cuda:0"



def _fixture():
    z = dict(np.load(os.path.join(GOLD, "visualize", "visualize_96x72.npz")))
    seq = np.load(os.path.join(GOLD, "example_sequence_96x72.npz"))
    gt = seq["images"][z["frames"]].astype(np.float32) / np.float32(255)
    gt[0, :int(z["mask_rows"])] = 0.0
    z["gt"] = gt
    z["fixed_rgb"] = np.concatenate([z["rgb_in"][:1], z["fixed_rgb_tail"]])        # the trio's first frame is frame 0's render
    return z


# ---------------------------------------------------------------------------------------------------------------------------------
# restatements (torch, CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def _jet_lut():
    """cm.jet's segment data (matplotlib _cm.py) evaluated at i / 255, then to8b -- no matplotlib needed."""
    seg = {"r": ((0.0, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1, 0.5, 0.5)),
           "g": ((0.0, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.64, 1, 1), (0.91, 0, 0), (1, 0, 0)),
           "b": ((0.0, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1, 0, 0))}
    # matplotlib's LinearSegmentedColormap with N = 256: lut = interpolation on linspace(0, 1, 256), indexed by the integer
    x = np.linspace(0, 1, 256)
    cols = []
    for ch in "rgb":
        xs = np.array([p[0] for p in seg[ch]])
        ys = np.array([p[1] for p in seg[ch]])
        cols.append(np.clip(np.interp(x, xs, ys), 0, 1))
    return torch.from_numpy((255 * np.clip(np.stack(cols, -1), 0, 1)).astype(np.uint8))


JET = _jet_lut()


def r_to8b(x):
    return (255 * x.clamp(0, 1)).to(torch.uint8)


def r_jet(x):
    """rnh:701-715 / fvr:804-814 then to8b: the uint8 index in x's dtype, the table."""
    idx = (255.0 * x.clamp(0, 1)).to(torch.uint8).long()
    return JET[idx]


def r_gradient(d, sp):
    """np.gradient(d, sp) of a float32 [H,W]: (zy, zx), float32 quotients by float32(2 sp) / float32(sp)."""
    s1, s2 = torch.tensor(sp, dtype=torch.float32), torch.tensor(2.0 * sp, dtype=torch.float32)

    def ax(t):
        o = torch.empty_like(t)
        o[1:-1] = (t[2:] - t[:-2]) / s2
        o[0] = (t[1] - t[0]) / s1
        o[-1] = (t[-1] - t[-2]) / s1
        return o
    return ax(d), ax(d.t()).t()


def r_phong(d):
    """rnh:718-791 on float32 [H,W] in numpy's dtypes, then to8b."""
    H, W = d.shape
    zy, zx = r_gradient(d, 2.0 / (H - 1))
    n0, n1, n2 = -zx, zy, torch.ones_like(d)
    nl = torch.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    n0, n1, n2 = n0 / nl, n1 / nl, n2 / nl
    vi = (torch.arange(W, dtype=torch.float32) / torch.tensor(float(W), dtype=torch.float32)).expand(H, W)
    vj = (torch.arange(H, dtype=torch.float32) / torch.tensor(float(W), dtype=torch.float32))[:, None].expand(H, W)
    l0, l1, l2 = 1.0 + (-vi).double(), 1.0 + (-vj).double(), 1.0 + (-d).double()
    dist = torch.sqrt((l0 * l0 + l1 * l1) + l2 * l2)
    l0, l1, l2 = l0 / dist, l1 / dist, l2 / dist
    dist = (dist + 1.0) * (dist + 1.0)
    lamb = ((l0 * n0.double() + l1 * n1.double()) + l2 * n2.double()).clamp(min=0.0)
    invalid = lamb <= 0.0
    w0, w1, w2 = -vi, -vj, -d
    wl = torch.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    h0, h1, h2 = l0 + (w0 / wl).double(), l1 + (w1 / wl).double(), l2 + (w2 / wl).double()
    hl = torch.sqrt((h0 * h0 + h1 * h1) + h2 * h2)
    h0, h1, h2 = h0 / hl, h1 / hl, h2 / hl
    sa = ((h0 * (-n0).double() + h1 * (-n1).double()) + h2 * (-n2).double()).clamp(min=0.0)
    spec = torch.where(invalid, torch.zeros_like(sa), sa * sa)
    specular = ((spec * 1.0) * 1.0) * 2.0 / dist
    cols = [(((lamb * dc) * 1.0) * 2.0 / dist + specular) + ac for dc, ac in ((0.5, 0.1), (0.0, 0.0), (0.0, 0.0))]
    return r_to8b(torch.stack(cols, -1))


def r_disparity(disp):
    """fvr:351-378 per frame: {"disp", "disp_jet", "disp_phong"} of float32 [F,H,W]."""
    out = {"disp": [], "disp_jet": [], "disp_phong": []}
    for d in disp:
        x = d / d.max()
        out["disp"].append(r_to8b(x))
        out["disp_jet"].append(r_jet(x))
        out["disp_phong"].append(r_phong(x))
    return {k: torch.stack(v) for k, v in out.items()}


def r_correspondences(pts, mn, mx, voxels=100):
    mn, mx = torch.as_tensor(mn, dtype=torch.float64), torch.as_tensor(mx, dtype=torch.float64)
    c = (pts.double() - mn) / (mx - mn)
    c = c * float(voxels)
    return r_to8b(c - torch.trunc(c))


def _reflect(i, n):
    if n == 1:
        return torch.zeros_like(i)
    i = i % (2 * n)
    return torch.where(i < n, i, 2 * n - 1 - i)


def _gauss():
    x = torch.arange(-5, 6, dtype=torch.float64)
    phi = torch.exp(-0.5 / 2.25 * x ** 2)
    return phi / phi.sum()


def r_filter(a):
    """scipy.ndimage.gaussian_filter(a, 1.5, truncate=3.5) of float64 [H,W] ('reflect'): axis 0, then axis 1."""
    H, W = a.shape
    w = _gauss()
    k = torch.arange(-5, 6)
    iy = _reflect(torch.arange(H)[:, None] + k[None, :], H)
    a = (a[iy] * w[None, :, None]).sum(1)
    ix = _reflect(torch.arange(W)[:, None] + k[None, :], W)
    return (a[:, ix] * w[None, None, :]).sum(-1)


def r_metrics(gt, ren, mask_ref):
    """fvr:813-860 for float32 [F,H,W,3]: psnr (double, from float32 differences), mean SSIM, the SSIM map, both error maps."""
    mask = (mask_ref.sum(-1) == 0) if mask_ref is not None else torch.zeros(gt.shape[1:3], dtype=torch.bool)
    res = {"psnr": [], "ssim": [], "ssim_map": [], "mse_error": [], "ssim_error": []}
    for g, r in zip(gt, ren):
        g, r = g.clone(), r.clone()
        g[mask] = 0.0
        r[mask] = 0.0
        d = g - r
        res["psnr"].append(float(-10.0 * torch.log10((d.double() ** 2).sum() / d.numel())))
        means, S = [], []
        for c in range(3):
            X, Y = g[..., c].double(), r[..., c].double()
            ux, uy, uxx, uyy, uxy = r_filter(X), r_filter(Y), r_filter(X * X), r_filter(Y * Y), r_filter(X * Y)
            vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
            C1, C2 = 0.01 ** 2, 0.03 ** 2
            Sc = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
            means.append(Sc[5:-5, 5:-5].mean() if min(Sc.shape) > 10 else torch.tensor(float("nan"), dtype=torch.float64))
            S.append(Sc)
        S = torch.stack(S, -1)
        res["ssim"].append(float(((means[0] + means[1]) + means[2]) / 3.0))
        res["ssim_map"].append(S)
        e = torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).double() / np.sqrt(3.0)
        res["mse_error"].append(r_jet((e * 10.0).clamp(0, 1)))
        res["ssim_error"].append(r_jet(1.0 - ((S[..., 0] + S[..., 1]) + S[..., 2]) / 3.0))
    return {k: (torch.tensor(v, dtype=torch.float64) if k in ("psnr", "ssim") else torch.stack(v)) for k, v in res.items()}


def r_stability(frames):
    x = frames.double()
    s, sq = torch.zeros_like(x[0]), torch.zeros_like(x[0])
    for f in x:
        s, sq = s + f, sq + f * f
    m = s / x.shape[0]
    std = torch.sqrt((sq / x.shape[0] - m * m).clamp(min=0.0))
    return r_jet(10.0 * (((std[..., 0] + std[..., 1]) + std[..., 2]) / 3.0))


def _jet_step_stats(a, b):
    """Jet-coded maps: (max distance in table steps between the indices behind the two colours, fraction of pixels that differ).  A
    one-step change of the index moves a channel by up to 5 LSB."""
    code = lambda t: (t[..., 0].long() << 16) | (t[..., 1].long() << 8) | t[..., 2].long()
    lut = code(JET)
    a, b = code(torch.as_tensor(a)), code(torch.as_tensor(b))
    diff = a != b
    if not bool(diff.any()):
        return 0, 0.0
    idx = lambda c: (c[:, None] == lut[None, :]).float().argmax(1)     # first index of the colour in the table
    steps = (idx(a[diff]) - idx(b[diff])).abs()
    return int(steps.max()), float(diff.float().mean())


def _lsb_stats(a, b):
    """(max |a - b| in LSB, fraction of bytes that differ)."""
    d = (torch.as_tensor(a).int() - torch.as_tensor(b).int()).abs()
    return int(d.max()), float((d > 0).float().mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU tier
# ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_jet_table_is_matplotlib_jet():
    """The 256 x 3 table csrc/nrnerf_visualize.hip embeds == to8b(cm.jet(i)[:3]) restated from jet's segment data."""
    import re
    src = open(os.path.join(REPO, "nonrigid_nerf_amd", "csrc", "nrnerf_visualize.hip")).read()
    body = re.search(r"JET\[256 \* 3\] = \{(.*?)\};", src, re.S).group(1)
    table = torch.tensor([int(v) for v in body.replace("\n", " ").split(",") if v.strip()], dtype=torch.uint8).reshape(256, 3)
    assert torch.equal(table, JET)


def test_restatements_reproduce_the_fixture():
    z = _fixture()
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in z.items()}
    dm = r_disparity(t["disp_in"])
    for k in ("disp", "disp_jet", "disp_phong"):
        assert torch.equal(dm[k], t[k]), (k, _lsb_stats(dm[k], t[k]))
    assert torch.equal(r_correspondences(t["surface_pts"], z["min_point"], z["max_point"]), t["correspondences"])
    assert torch.equal(r_to8b(t["surface_rigidity"]), t["rigidity"])
    assert torch.equal(r_jet(t["surface_rigidity"]), t["rigidity_jet"])
    m = r_metrics(t["gt"], t["rgb_in"], t["gt"][0])
    assert int(z["n_masked"]) > 0
    assert torch.allclose(m["psnr"], t["psnr"], rtol=0, atol=1e-9)
    assert (m["psnr"] - t["psnr_numpy_f32"]).abs().max() < 1e-4            # the reference's float32 np.mean rounds at ~1e-6 relative
    assert torch.allclose(m["ssim"], t["ssim"], rtol=0, atol=1e-12)
    assert (m["ssim_map"][0] - t["ssim_map_0"].double()).abs().max() < 1e-6      # (frame 0's map, stored as float32)
    assert torch.equal(m["mse_error"], t["mse_error"])
    assert torch.equal(m["ssim_error"], t["ssim_error"])
    assert torch.equal(r_stability(t["fixed_rgb"]), t["stability"])


def test_abi_structs_match_ctypes(tmp_path):
    """No GPU needed: sizeof / offsetof of the ABI 9 structures as a C99 compiler sees them == the ctypes mirror."""
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nrnerf.h"\nint main(void) {\n'
                     'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(nrnerf_visualize_args), offsetof(nrnerf_visualize_args, min_point),\n'
                     '       offsetof(nrnerf_visualize_args, voxels), offsetof(nrnerf_visualize_args, rigidity),\n'
                     '       offsetof(nrnerf_visualize_args, rigidity_jet), offsetof(nrnerf_visualize_args, disp_max));\n'
                     'printf("%zu %zu %zu %zu %zu\\n", sizeof(nrnerf_metrics_args), offsetof(nrnerf_metrics_args, gt),\n'
                     '       offsetof(nrnerf_metrics_args, ssim_map), offsetof(nrnerf_metrics_args, workspace),\n'
                     '       offsetof(nrnerf_metrics_args, workspace_bytes));\n'
                     'printf("%d %d %d %d %d %d %d %d\\n", NRNERF_ABI_VERSION, NRNERF_VIS_DISP, NRNERF_VIS_DISP_JET, NRNERF_VIS_DISP_PHONG,\n'
                     '       NRNERF_VIS_CORRESPONDENCES, NRNERF_VIS_RIGIDITY, NRNERF_VIS_RIGIDITY_JET, NRNERF_VIS_NORM_STACK);\n'
                     'return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    VA, MA = _lib.VisualizeArgs, _lib.MetricsArgs
    want = [C.sizeof(VA), VA.min_point.offset, VA.voxels.offset, VA.rigidity.offset, VA.rigidity_jet.offset, VA.disp_max.offset,
            C.sizeof(MA), MA.gt.offset, MA.ssim_map.offset, MA.workspace.offset, MA.workspace_bytes.offset,
            _lib.ABI_VERSION, _lib.VIS_DISP, _lib.VIS_DISP_JET, _lib.VIS_DISP_PHONG, _lib.VIS_CORRESPONDENCES, _lib.VIS_RIGIDITY,
            _lib.VIS_RIGIDITY_JET, _lib.VIS_NORM_STACK]
    assert got == want


def _closed_form_frame(i, c2w, intrin, code):
    H, W = int(intrin["height"]), int(intrin["width"])
    px = torch.arange(H * W, dtype=torch.float32)
    rgb = torch.stack([px / (H * W), (px % 7) / 7.0, torch.full_like(px, 0.25 + 0.1 * i)], -1)
    return {"rgb_map": rgb, "disp_map": px + 1000.0 * i, "acc_map": torch.ones(H * W),
            "surface_pts": rgb + 1.0, "surface_rigidity": px * 0.0 + i, "median_index": (px % 3).to(torch.int32)}


def test_render_path_default_returns_unchanged():
    """Without the new keywords render_path returns exactly what it returned before (2 or 3 elements); asking for rigidity maps of a
    model without a ray bender is a ValueError before anything renders."""
    from nonrigid_nerf_amd.driver import render_path
    poses = [torch.eye(4)[:3] + 0.01 * f for f in range(3)]
    intr = [dict(height=3, width=5, focal_x=4.0, focal_y=4.0, center_x=2.5, center_y=1.5) for _ in range(3)]
    codes = torch.zeros(3, 4)
    kw = dict(near=0.1, far=1.0, network_fn=None)
    res = render_path(poses, intr, 1024, kw, codes, _frame_fn=_closed_form_frame)
    assert isinstance(res, tuple) and len(res) == 2 and res[0].shape == (3, 3, 5, 3) and res[1].shape == (3, 3, 5)
    res = render_path(poses, intr, 1024, kw, codes, _frame_fn=_closed_form_frame, surface_outputs=True)
    assert len(res) == 3 and set(res[2][0]) == {"surface_pts", "surface_rigidity", "median_index"}
    res = render_path(poses, intr, 1024, kw, codes, _frame_fn=_closed_form_frame, visualizations=(), metrics=False, stability=False)
    assert len(res) == 2

    class NoBender(torch.nn.Module):
        ray_bender = None
    with pytest.raises(ValueError, match="ray bender"):
        render_path(poses, intr, 1024, dict(near=0.1, far=1.0, network_fn=NoBender()), codes, visualizations=("rigidity",))
    with pytest.raises(ValueError, match="volume_extent"):
        render_path(poses, intr, 1024, kw, codes, _frame_fn=_closed_form_frame, visualizations=("correspondences",))
    with pytest.raises(ValueError, match="unknown visualizations"):
        render_path(poses, intr, 1024, kw, codes, _frame_fn=_closed_form_frame, visualizations=("depth",))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------------------
def _dev(x):
    return torch.as_tensor(np.asarray(x)).to(DEV).contiguous()


@pytest.mark.gpu
def test_maps_and_scores_against_the_fixture():
    z = _fixture()
    dm = V.disparity_maps(_dev(z["disp_in"]))
    for k in ("disp", "disp_jet"):
        assert np.array_equal(dm[k].cpu().numpy(), z[k]), k
    lsb, frac = _lsb_stats(dm["disp_phong"].cpu(), torch.from_numpy(z["disp_phong"]))
    assert lsb <= 1 and frac <= 1e-3, (lsb, frac)
    assert np.array_equal(V.correspondence_rgb(_dev(z["surface_pts"]), z["min_point"], z["max_point"]).cpu().numpy(), z["correspondences"])
    rm = V.rigidity_maps(_dev(z["surface_rigidity"]))
    assert np.array_equal(rm["rigidity"].cpu().numpy(), z["rigidity"])
    assert np.array_equal(rm["rigidity_jet"].cpu().numpy(), z["rigidity_jet"])
    scores, maps = V.image_metrics(_dev(z["gt"]), _dev(z["rgb_in"]), error_maps=True, ssim_map=True)
    for f in range(3):
        assert abs(scores[f]["psnr"] - z["psnr"][f]) <= 1e-6 and abs(scores[f]["ssim"] - z["ssim"][f]) <= 1e-6, (f, scores[f])
        assert scores[f]["lpips"] is None
    assert abs(scores["average_psnr"] - np.mean(z["psnr"])) <= 1e-6 and scores["average_lpips"] is None
    assert np.abs(maps["ssim_map"][0].cpu().numpy() - z["ssim_map_0"]).max() <= 1e-5
    for k in ("mse_error", "ssim_error"):
        steps, frac = _jet_step_stats(maps[k].cpu(), torch.from_numpy(z[k]))
        assert steps <= 1 and frac <= 1e-3, (k, steps, frac)
    st = V.BackgroundStability()
    for f in z["fixed_rgb"]:
        st.add(_dev(f))
    assert np.array_equal(st.finish().cpu().numpy(), z["stability"])


def _random_case(F, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    disp = 0.05 + torch.rand(F, H, W, generator=g)
    disp[:, : H // 3] *= 0.5                                   # a ridge, so that the normals vary
    gt = torch.rand(F, H, W, 3, generator=g)
    ren = (gt + 0.1 * torch.randn(F, H, W, 3, generator=g)).clamp(0, 1)
    gt[0, :, : max(1, W // 8)] = 0.0                           # a masked band in the first frame
    pts = torch.randn(F, H, W, 3, generator=g)
    rig = torch.rand(F, H, W, generator=g) * 1.2 - 0.1
    return disp, gt, ren, pts, rig


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(2, 3), (17, 31), (384, 512), (1080, 1920)])
def test_kernels_against_restatements(H, W):
    F = 2 if H * W < 1e6 else 1
    disp, gt, ren, pts, rig = _random_case(F, H, W, H * 7919 + W)
    dm = V.disparity_maps(disp.to(DEV))
    want = r_disparity(disp)
    for k in ("disp", "disp_jet"):
        assert torch.equal(dm[k].cpu(), want[k]), k
    lsb, frac = _lsb_stats(dm["disp_phong"].cpu(), want["disp_phong"])
    assert lsb <= 1 and frac <= 1e-3, (lsb, frac)
    mn, mx = (-2.0, -2.5, -3.0), (2.0, 2.5, 1.0)
    assert torch.equal(V.correspondence_rgb(pts.to(DEV), mn, mx).cpu(), r_correspondences(pts, mn, mx))
    rm = V.rigidity_maps(rig.to(DEV))
    assert torch.equal(rm["rigidity"].cpu(), r_to8b(rig)) and torch.equal(rm["rigidity_jet"].cpu(), r_jet(rig))
    got = V.metrics_on_device(gt.to(DEV), ren.to(DEV), mask_ref=gt[0].to(DEV), error_maps=True, ssim_map=True)
    ref = r_metrics(gt, ren, gt[0])
    assert torch.allclose(got["psnr"].cpu(), ref["psnr"], rtol=0, atol=1e-6)
    assert torch.allclose(got["ssim"].cpu(), ref["ssim"], rtol=0, atol=1e-6, equal_nan=True)
    assert (got["ssim_map"].cpu() - ref["ssim_map"]).abs().max() <= 1e-5
    for k in ("mse_error", "ssim_error"):
        steps, frac = _jet_step_stats(got[k].cpu(), ref[k])
        assert steps <= 1 and frac <= 1e-3, (k, steps, frac)
    st = V.BackgroundStability()
    st.add(ren.to(DEV))
    st.add(gt.to(DEV))
    assert torch.equal(st.finish().cpu(), r_stability(torch.cat([ren, gt])))


@pytest.mark.gpu
def test_scores_are_bit_reproducible_and_stack_normalisation():
    disp, gt, ren, _, _ = _random_case(3, 384, 512, 5)
    a = V.metrics_on_device(gt.to(DEV), ren.to(DEV), mask_ref=gt[0].to(DEV), ssim_map=True)
    b = V.metrics_on_device(gt.to(DEV), ren.to(DEV), mask_ref=gt[0].to(DEV), ssim_map=True)
    for k in ("psnr", "ssim", "mse", "ssim_map"):
        assert torch.equal(a[k], b[k]), k
    st = V.disparity_maps(disp.to(DEV), kinds="disp", normalize="stack")["disp"].cpu()
    assert torch.equal(st, r_to8b(disp / disp.max()))
    none = V.disparity_maps(disp.to(DEV), kinds=("jet",), normalize=None)["disp_jet"].cpu()
    assert torch.equal(none, r_jet(disp))


@pytest.mark.gpu
def test_render_path_visualizations_match_the_module():
    """render_path(..., visualizations="all", metrics=True, stability=True) on the fitted checkpoint in f32 mode: every map is byte-equal
    to nonrigid_nerf_amd.visualize applied to the render_path's own returned disp / rgb / surface outputs."""
    from nonrigid_nerf_amd import render as R
    from nonrigid_nerf_amd.checkpoint import load_checkpoint
    from nonrigid_nerf_amd.driver import render_path
    ck = load_checkpoint(os.path.join(GOLD, "fitted_latest.tar"), N_samples=64, N_importance=128, device=DEV)
    zs = np.load(os.path.join(GOLD, "example_sequence_96x72.npz"))
    near, far = float(zs["bds"].min()) * 0.9, float(zs["bds"].max())
    H, W, focal = int(zs["hwf"][0]), int(zs["hwf"][1]), float(zs["hwf"][2])
    intrin = dict(height=H, width=W, focal_x=focal, focal_y=focal, center_x=W / 2, center_y=H / 2)
    frames = [0, 5]
    poses = [torch.from_numpy(zs["poses"][f]) for f in frames]
    gt = zs["images"][frames].astype(np.float32) / np.float32(255)
    ext = ((-1.5, -1.5, -2.0), (1.5, 1.5, 0.5))
    R.set_precision("f32")
    try:
        kw = dict(ck.render_kwargs_test, near=near, far=far)
        rgbs, disps, det, ex = render_path(poses, [intrin] * 2, 1024 * 32, kw, ck.latents[frames], gt_imgs=gt, surface_outputs=True,
                                           visualizations="all", volume_extent=ext, metrics=True, stability=True)
        base = render_path(poses, [intrin] * 2, 1024 * 32, kw, ck.latents[frames])
    finally:
        R.set_precision("bf16")
    assert len(base) == 2
    dm = V.disparity_maps(_dev(disps))
    for k in ("disp", "disp_jet", "disp_phong"):
        assert np.array_equal(ex[k], dm[k].cpu().numpy()), k
    pts = np.stack([d["surface_pts"] for d in det])
    rig = np.stack([d["surface_rigidity"] for d in det])
    assert np.array_equal(ex["correspondences"], V.correspondence_rgb(_dev(pts), *ext).cpu().numpy())
    rm = V.rigidity_maps(_dev(rig))
    assert np.array_equal(ex["rigidity"], rm["rigidity"].cpu().numpy()) and np.array_equal(ex["rigidity_jet"], rm["rigidity_jet"].cpu().numpy())
    scores, maps = V.image_metrics(_dev(gt), _dev(rgbs), error_maps=True)
    for f in range(2):
        assert ex["scores"][f]["psnr"] == scores[f]["psnr"] and ex["scores"][f]["ssim"] == scores[f]["ssim"]
    assert ex["scores"]["average_psnr"] == scores["average_psnr"] and ex["scores"]["average_lpips"] is None
    for k in ("mse_error", "ssim_error"):
        assert np.array_equal(ex[k], maps[k].cpu().numpy()), k
    st = V.BackgroundStability()
    st.add(_dev(rgbs))
    assert np.array_equal(ex["stability"], st.finish().cpu().numpy())
    assert ex["disp_jet"].shape == (2, H, W, 3) and ex["disp"].dtype == np.uint8
