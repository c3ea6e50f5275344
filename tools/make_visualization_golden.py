"""Writes tests/golden/visualize/visualize_96x72.npz: inputs and expected outputs of free_viewpoint_rendering.py's (fvr) per-frame images and
scores, for tests/test_visualize.py.  Runs on the CPU (no GPU needed):

    NRNERF_REFERENCE=/path/to/nonrigid_nerf python tools/make_visualization_golden.py

Inputs: the fp32 oracle's render (oracle.nrnerf_oracle.render_path with detailed outputs + surface_from_details) of the fitted
checkpoint tests/golden/fitted_latest.tar at 96 x 72 -- frames 0, i_test and 30 at their own cameras, and a fixed-camera trio (the camera
of frame 0, the codes of frames 0, 15, 30).  The ground truth is example_sequence_96x72.npz's images / 255 (float32), which the tests
read from there; a 4-pixel black band is painted into the first frame's ground truth (rows 0-3), the undistortion border fvr masks out
(fvr:819-823).

Expected outputs: the disparity colour maps from the reference's own functions (imported from $NRNERF_REFERENCE/run_nerf_helpers.py:
to8b, visualize_disparity_with_jet_color_scheme, visualize_disparity_with_blinn_phong), the correspondence / rigidity maps, error maps
and background stability as fvr computes them (restated below with line citations: they are closures inside its main function), and
SSIM as skimage's structural_similarity computes it (restated with scipy.ndimage.gaussian_filter: skimage is not a dependency here).
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch
from scipy.ndimage import gaussian_filter

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden")
FRAMES = (0, None, 30)          # None: i_test
FIXED_CODES = (0, 15, 30)
MASK_ROWS = 4
MIN_POINT = np.array([-1.5, -1.5, -2.0])      # a volume around the scene (the fitted checkpoint's scripts_dict carries none)
MAX_POINT = np.array([1.5, 1.5, 0.5])


def _reference_helpers():
    ref = os.environ.get("NRNERF_REFERENCE")
    if not ref:
        sys.exit("set NRNERF_REFERENCE to a checkout of the reference (run_nerf_helpers.py is imported from there)")
    spec = importlib.util.spec_from_file_location("rnh", os.path.join(ref, "run_nerf_helpers.py"))
    rnh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rnh)
    return rnh


def ssim_skimage(im1, im2):
    """skimage.metrics.structural_similarity(im1, im2, data_range=1.0, multichannel=True, gaussian_weights=True, sigma=1.5,
    use_sample_covariance=False, full=True) on float64 copies: per channel, then the mean over channels."""
    sigma, truncate = 1.5, 3.5
    pad = (2 * int(truncate * sigma + 0.5) + 1 - 1) // 2
    means, S = [], []
    for c in range(im1.shape[-1]):
        X, Y = im1[..., c].astype(np.float64), im2[..., c].astype(np.float64)
        f = lambda a: gaussian_filter(a, sigma=sigma, truncate=truncate)          # mode='reflect'
        ux, uy, uxx, uyy, uxy = f(X), f(Y), f(X * X), f(Y * Y), f(X * Y)
        vx, vy, vxy = 1.0 * (uxx - ux * ux), 1.0 * (uyy - uy * uy), 1.0 * (uxy - ux * uy)
        C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
        A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
        Sc = (A1 * A2) / (B1 * B2)
        means.append(Sc[pad:-pad, pad:-pad].mean())
        S.append(Sc)
    return float(np.mean(means)), np.stack(S, -1)


def main():
    rnh = _reference_helpers()
    to8b = rnh.to8b
    from matplotlib import cm
    from nonrigid_nerf_amd.checkpoint import load_checkpoint
    from nonrigid_nerf_amd.synthetic import Scene, SceneConfig
    from oracle import nrnerf_oracle as O

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ck = load_checkpoint(os.path.join(GOLD, "fitted_latest.tar"), N_samples=64, N_importance=128)
    z = np.load(os.path.join(GOLD, "example_sequence_96x72.npz"))
    near, far = float(z["bds"].min()) * 0.9, float(z["bds"].max())
    H, W, focal = int(z["hwf"][0]), int(z["hwf"][1]), float(z["hwf"][2])
    intrin = dict(height=H, width=W, focal_x=focal, focal_y=focal, center_x=W / 2, center_y=H / 2)
    sd = lambda m: {k: v.detach().clone() for k, v in m.state_dict().items()}
    scene = Scene(SceneConfig(near=near, far=far), sd(ck.ray_bender), sd(ck.network_fn), sd(ck.network_fine))
    frames = [int(z["i_test"]) if f is None else f for f in FRAMES]

    def render(poses, codes):
        with torch.no_grad():
            rgb, disp, det = O.render_path([torch.from_numpy(p) for p in poses], [intrin] * len(poses), scene, codes, detailed_output=True)
        pts, rig = [], []
        for d in det:
            _, p, r = O.surface_from_details(d["fine_visibility_weights"].reshape(H * W, -1), d["fine_input_pts"].reshape(H * W, -1, 3),
                                             d["fine_rigidity_mask"].reshape(H * W, -1))
            pts.append(p.reshape(H, W, 3))
            rig.append(r.reshape(H, W))
        return rgb.numpy(), disp.numpy(), torch.stack(pts).numpy(), torch.stack(rig).numpy()

    rgb, disp, pts, rig = render(z["poses"][frames], ck.latents[frames].cpu())
    fixed_rgb = render(z["poses"][[0] * len(FIXED_CODES)], ck.latents[list(FIXED_CODES)].cpu())[0]
    gt = z["images"][frames].astype(np.float32) / np.float32(255)
    gt[0, :MASK_ROWS] = 0.0

    # (size: the trio's first frame is frame 0's render, bit for bit -- stored once; the SSIM map of the first frame only)
    assert np.array_equal(fixed_rgb[0], rgb[0])
    out = dict(frames=np.array(frames, np.int32), fixed_codes=np.array(FIXED_CODES, np.int32), mask_rows=np.int32(MASK_ROWS),
               disp_in=disp, rgb_in=rgb, surface_pts=pts, surface_rigidity=rig, fixed_rgb_tail=fixed_rgb[1:],
               min_point=MIN_POINT, max_point=MAX_POINT)
    # fvr:351-378, per frame (normalize=True)
    out["disp"] = np.stack([to8b(d / np.max(d)) for d in disp])
    out["disp_jet"] = np.stack([to8b(rnh.visualize_disparity_with_jet_color_scheme(d / np.max(d))) for d in disp])
    out["disp_phong"] = np.stack([to8b(rnh.visualize_disparity_with_blinn_phong(d / np.max(d))) for d in disp])
    # fvr:638-645 (min_point / max_point: float64 arrays, fvr:617-622)
    corr = (pts - MIN_POINT.reshape(1, 1, 3)) / (MAX_POINT.reshape(1, 1, 3) - MIN_POINT.reshape(1, 1, 3))
    corr *= 100
    corr = corr - corr.astype(int)
    out["correspondences"] = to8b(corr)                                          # fvr:702 convert_rgb_to_saveable
    # fvr:705-707, normalize=False
    out["rigidity"] = np.stack([to8b(r.copy()) for r in rig])
    out["rigidity_jet"] = np.stack([to8b(rnh.visualize_disparity_with_jet_color_scheme(r.copy())) for r in rig])
    # fvr:767-785: the reference's float32 np.std, and the float64 flow the library uses (sums of x and x^2 in double)
    lut = np.array([cm.jet(i)[:3] for i in range(256)])
    jet8 = lambda v: to8b(lut[(255.0 * np.clip(v, 0.0, 1.0)).astype("uint8").flatten()].reshape(v.shape + (3,)))
    stability_f32 = jet8(10 * np.mean(np.std(fixed_rgb, axis=0), axis=-1))
    x = fixed_rgb.astype(np.float64)
    s, sq = np.zeros_like(x[0]), np.zeros_like(x[0])
    for f in range(x.shape[0]):
        s, sq = s + x[f], sq + x[f] * x[f]
    m = s / x.shape[0]
    std = np.sqrt(np.maximum(sq / x.shape[0] - m * m, 0.0))
    out["stability"] = jet8(10.0 * (((std[..., 0] + std[..., 1]) + std[..., 2]) / 3.0))
    out["stability_pixels_off_numpy_f32"] = np.int32((out["stability"] != stability_f32).any(-1).sum())
    # fvr:813-860
    mask = np.sum(gt[0], axis=-1) == 0.0
    psnr, psnr32, ssim, smap, mse_err, ssim_err = [], [], [], [], [], []
    for g, r in zip(gt, rgb):
        g, r = g.copy(), r.copy()
        g[mask] = 0.0
        r[mask] = 0.0
        d = g - r
        psnr32.append(float(-10.0 * np.log10(np.mean(d ** 2))))                 # fvr:826-827 (float32)
        psnr.append(float(-10.0 * np.log10(np.sum(d.astype(np.float64) ** 2) / d.size)))
        s_mean, S = ssim_skimage(g, r)
        ssim.append(s_mean)
        smap.append(S.astype(np.float32))
        e = np.linalg.norm(d, axis=-1) / np.sqrt(1 + 1 + 1)
        e *= 10.0
        e = np.clip(e, 0.0, 1.0)
        mse_err.append(jet8(e))
        ssim_err.append(jet8(1.0 - np.mean(S, axis=-1)))
    out.update(psnr=np.array(psnr), psnr_numpy_f32=np.array(psnr32), ssim=np.array(ssim), ssim_map_0=smap[0],
               mse_error=np.stack(mse_err), ssim_error=np.stack(ssim_err), n_masked=np.int32(mask.sum()))
    path = os.path.join(GOLD, "visualize", "visualize_96x72.npz")    # (a folder of its own: every .npz at the top of tests/golden is a render case)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes); frames {frames}, masked pixels {int(mask.sum())}; psnr {psnr}, ssim {ssim}; "
          f"stability pixels differing from the float32 numpy flow: {int(out['stability_pixels_off_numpy_f32'])}")


if __name__ == "__main__":
    main()
