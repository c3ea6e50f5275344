"""The images and scores the reference's ``free_viewpoint_rendering.py`` (fvr) writes for every frame, on the device.

Every function takes CUDA tensors, batched over frames, and launches the HIP kernels of ``csrc/nrnerf_visualize.hip`` (C ABI 9,
``include/nrnerf.h``) on the current stream; the uint8 images come back as CUDA tensors, so a caller moves 1 or 3 bytes per pixel to
the host instead of running numpy there (about 130 ms per 512 x 384 frame, several times the render).

* ``disparity_maps``: ``disp``, ``disp_jet``, ``disp_phong`` (fvr:351-378; run_nerf_helpers.py (rnh):701-791);
* ``correspondence_rgb``: the canonical-space correspondence colours (fvr:638-645);
* ``rigidity_maps``: ``rigidity``, ``rigidity_jet`` (fvr:665-668);
* ``image_metrics``: PSNR / SSIM per frame with fvr's ``scores.json`` layout and the two error maps (fvr:787-876);
* ``BackgroundStability``: the fixed-camera standard-deviation map (fvr:767-785).

The uint8 maps are the reference's bytes: the kernels restate numpy's float32 / float64 operations in order.  The scores are computed
in double: PSNR from the float32 differences (numpy's ``np.mean`` of float32 squares rounds to float32, about 1e-6 dB at 30 dB), SSIM as
skimage's ``structural_similarity(data_range=1, gaussian_weights=True, sigma=1.5, use_sample_covariance=False)`` on float64 images.
LPIPS needs a network that is not part of this package: its entries are ``None``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

DISPARITY_KINDS = {"disp": ("disp", _lib.VIS_DISP), "jet": ("disp_jet", _lib.VIS_DISP_JET), "phong": ("disp_phong", _lib.VIS_DISP_PHONG)}
_NORMALIZE = {None: _lib.VIS_NORM_NONE, "frame": _lib.VIS_NORM_FRAME, "stack": _lib.VIS_NORM_STACK}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _frames(t, name, dims, dtype=torch.float32):
    """[F, *dims] contiguous on a CUDA device (a single frame [*dims] gets F = 1)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor")
    if t.dim() == len(dims):
        t = t.unsqueeze(0)
    if t.dim() != len(dims) + 1 or any(d is not None and t.shape[k + 1] != d for k, d in enumerate(dims)):
        raise ValueError(f"{name} must be [F, {', '.join('H W 3'.split()[:len(dims)])}] (got {tuple(t.shape)})")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    return t.contiguous()


def _visualize(flags, F, H, W, dev, disp=None, normalize=_lib.VIS_NORM_NONE, disp_max=None, pts=None, extent=None, voxels=100,
               rigidity=None):
    lib = _lib.load()
    a = _lib.VisualizeArgs()
    a.struct_size, a.flags, a.n_frames, a.height, a.width, a.normalize = C.sizeof(a), flags, F, H, W, normalize
    a.voxels = int(voxels)
    if extent is not None:
        for k in range(3):
            a.min_point[k], a.max_point[k] = float(extent[0][k]), float(extent[1][k])
    out = {}

    def new(key, flag, shape):
        if flags & flag:
            out[key] = torch.empty(shape, dtype=torch.uint8, device=dev)
            return _ptr(out[key])
        return None
    a.disp, a.disp_max, a.surface_pts, a.rigidity = _ptr(disp), _ptr(disp_max), _ptr(pts), _ptr(rigidity)
    a.disp_out = new("disp", _lib.VIS_DISP, (F, H, W))
    a.disp_jet = new("disp_jet", _lib.VIS_DISP_JET, (F, H, W, 3))
    a.disp_phong = new("disp_phong", _lib.VIS_DISP_PHONG, (F, H, W, 3))
    a.correspondences = new("correspondences", _lib.VIS_CORRESPONDENCES, (F, H, W, 3))
    a.rigidity_out = new("rigidity", _lib.VIS_RIGIDITY, (F, H, W))
    a.rigidity_jet = new("rigidity_jet", _lib.VIS_RIGIDITY_JET, (F, H, W, 3))
    with torch.cuda.device(dev):
        _lib.check(lib.nrnerf_visualize_frames(C.byref(a), _stream(dev)), "nrnerf_visualize_frames")
    return out


def disparity_maps(disp, kinds=("disp", "jet", "phong"), normalize="frame", disp_max=None):
    """uint8 maps of a disparity stack ``disp [F,H,W]`` (or ``[H,W]``) float32: ``{"disp" [F,H,W], "disp_jet" [F,H,W,3],
    "disp_phong" [F,H,W,3]}`` for the requested ``kinds`` (a subset of "disp", "jet", "phong").

    ``normalize``: "frame" = each frame divided by its own max (fvr's per-image ``convert_disparity_to_*``, fvr:351-378); "stack" = by the
    max over all frames (fvr:724-741, the videos); None = as it is.  ``disp_max`` (a CUDA float32 tensor [F]) overrides the divisor.
    The Blinn-Phong map needs H, W >= 2 (np.gradient)."""
    if isinstance(kinds, str):
        kinds = (kinds,)
    bad = [k for k in kinds if k not in DISPARITY_KINDS]
    if bad:
        raise ValueError(f"unknown disparity map kinds {bad} (one of {sorted(DISPARITY_KINDS)})")
    if normalize not in _NORMALIZE:
        raise ValueError("normalize must be 'frame', 'stack' or None")
    disp = _frames(disp, "disp", (None, None))
    F, H, W = disp.shape
    flags = 0
    for k in kinds:
        flags |= DISPARITY_KINDS[k][1]
    if flags & _lib.VIS_DISP_PHONG and (H < 2 or W < 2):
        raise ValueError("the Blinn-Phong map needs at least 2 x 2 pixels (np.gradient)")
    mode = _NORMALIZE[normalize]
    if disp_max is not None:
        disp_max = torch.as_tensor(disp_max, dtype=torch.float32, device=disp.device).reshape(-1).expand(F).contiguous()
        mode = _lib.VIS_NORM_GIVEN
    elif mode != _lib.VIS_NORM_NONE:
        disp_max = torch.empty(F, dtype=torch.float32, device=disp.device)
    return _visualize(flags, F, H, W, disp.device, disp=disp, normalize=mode, disp_max=disp_max)


def correspondence_rgb(surface_pts, min_point, max_point, voxels=100):
    """uint8 ``[F,H,W,3]`` correspondence colours of the surface points ``surface_pts [F,H,W,3]`` (or ``[H,W,3]``) float32
    (fvr:638-645): ``to8b(frac(voxels * (p - min_point) / (max_point - min_point)))`` in float64, frac = x - trunc(x)."""
    pts = _frames(surface_pts, "surface_pts", (None, None, 3))
    F, H, W, _ = pts.shape
    ext = (np.asarray(min_point, dtype=np.float64).reshape(3), np.asarray(max_point, dtype=np.float64).reshape(3))
    return _visualize(_lib.VIS_CORRESPONDENCES, F, H, W, pts.device, pts=pts, extent=ext, voxels=voxels)["correspondences"]


def rigidity_maps(rigidity, kinds=("rigidity", "rigidity_jet")):
    """uint8 ``{"rigidity" [F,H,W], "rigidity_jet" [F,H,W,3]}`` of ``rigidity [F,H,W]`` (or ``[H,W]``) float32, not normalised
    (fvr:665-668)."""
    if isinstance(kinds, str):
        kinds = (kinds,)
    names = {"rigidity": _lib.VIS_RIGIDITY, "rigidity_jet": _lib.VIS_RIGIDITY_JET}
    bad = [k for k in kinds if k not in names]
    if bad:
        raise ValueError(f"unknown rigidity map kinds {bad} (one of {sorted(names)})")
    rig = _frames(rigidity, "rigidity", (None, None))
    F, H, W = rig.shape
    flags = 0
    for k in kinds:
        flags |= names[k]
    return _visualize(flags, F, H, W, rig.device, rigidity=rig)


def metrics_on_device(gt, rendered, mask_ref=None, error_maps=False, ssim_map=False):
    """The launch behind ``image_metrics``: ``{"psnr" [F], "ssim" [F], "mse" [F]}`` float64 CUDA tensors, plus "mse_error" /
    "ssim_error" uint8 [F,H,W,3] with ``error_maps`` and "ssim_map" float64 [F,H,W,3] (skimage's full S) with ``ssim_map``.  Nothing
    is synchronised.  ``mask_ref`` [H,W,3]: pixels whose channel sum is 0 there are zeroed in both images (None: no mask)."""
    gt = _frames(gt, "gt", (None, None, 3))
    rendered = _frames(rendered, "rendered", (None, None, 3))
    if gt.shape != rendered.shape or gt.device != rendered.device:
        raise ValueError("gt and rendered must have one shape and device")
    F, H, W, _ = gt.shape
    dev = gt.device
    if mask_ref is not None:
        mask_ref = _frames(mask_ref, "mask_ref", (H, W, 3))[0]
    lib = _lib.load()
    ws = torch.empty(max(1, int(lib.nrnerf_visualize_workspace_bytes(F, H, W))), dtype=torch.uint8, device=dev)
    d64 = dict(dtype=torch.float64, device=dev)
    out = {"psnr": torch.empty(F, **d64), "ssim": torch.empty(F, **d64), "mse": torch.empty(F, **d64)}
    if error_maps:
        out["mse_error"] = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        out["ssim_error"] = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    if ssim_map:
        out["ssim_map"] = torch.empty((F, H, W, 3), **d64)
    a = _lib.MetricsArgs()
    a.struct_size, a.n_frames, a.height, a.width = C.sizeof(a), F, H, W
    a.gt, a.rendered, a.mask_ref = _ptr(gt), _ptr(rendered), _ptr(mask_ref)
    a.psnr, a.ssim, a.mse = _ptr(out["psnr"]), _ptr(out["ssim"]), _ptr(out["mse"])
    a.ssim_map, a.mse_error_map, a.ssim_error_map = _ptr(out.get("ssim_map")), _ptr(out.get("mse_error")), _ptr(out.get("ssim_error"))
    a.workspace, a.workspace_bytes = _ptr(ws), ws.numel()
    with torch.cuda.device(dev):
        _lib.check(lib.nrnerf_image_metrics(C.byref(a), _stream(dev)), "nrnerf_image_metrics")
    ws.record_stream(torch.cuda.current_stream(dev))
    return out


def scores_json(psnr, ssim, first=0):
    """fvr's ``scores.json`` dictionary (fvr:862-876) from per-frame PSNR / SSIM values: ``{i: {"psnr", "ssim", "lpips": None}, ...,
    "average_psnr", "average_ssim", "average_lpips": None}``, frames numbered from ``first``."""
    psnr, ssim = [float(v) for v in psnr], [float(v) for v in ssim]
    scores = {first + i: {"psnr": p, "ssim": s, "lpips": None} for i, (p, s) in enumerate(zip(psnr, ssim))}
    scores["average_psnr"] = float(np.mean(psnr)) if psnr else float("nan")
    scores["average_ssim"] = float(np.mean(ssim)) if ssim else float("nan")
    scores["average_lpips"] = None
    return scores


def image_metrics(gt, rendered, error_maps=False, ssim_map=False, mask_ref="first"):
    """PSNR and SSIM of each (gt, rendered) pair, ``[F,H,W,3]`` float32 CUDA tensors, in fvr's ``scores.json`` layout.

    ``mask_ref``: "first" (fvr:819-823: the pixels where the first ground-truth frame's channel sum is 0 are zeroed in both images),
    a [H,W,3] tensor, or None.  With ``error_maps`` (and / or ``ssim_map``) returns ``(scores, maps)``: "mse_error" / "ssim_error"
    uint8 [F,H,W,3] (fvr:847-860), "ssim_map" float64 [F,H,W,3]."""
    gt = _frames(gt, "gt", (None, None, 3))
    if isinstance(mask_ref, str):
        if mask_ref != "first":
            raise ValueError("mask_ref must be 'first', a tensor or None")
        mask_ref = gt[0]
    out = metrics_on_device(gt, rendered, mask_ref=mask_ref, error_maps=error_maps, ssim_map=ssim_map)
    scores = scores_json(out["psnr"].cpu().tolist(), out["ssim"].cpu().tolist())
    if not (error_maps or ssim_map):
        return scores
    return scores, {k: v for k, v in out.items() if k in ("mse_error", "ssim_error", "ssim_map")}


class BackgroundStability:
    """fvr:767-785 for a fixed camera: ``add(rgb)`` per frame (``[H,W,3]`` or ``[F,H,W,3]`` float32 CUDA), ``finish()`` -> uint8
    ``[H,W,3]`` = jet(clip(10 * mean_c std)), std the population standard deviation over the frames.  Sums in double on the device."""

    def __init__(self):
        self.sum = self.sum_sq = None
        self.count = 0

    def add(self, rgb):
        rgb = _frames(rgb, "rgb", (None, None, 3))
        if self.sum is None:
            self.sum = torch.zeros(rgb.shape[1:], dtype=torch.float64, device=rgb.device)
            self.sum_sq = torch.zeros_like(self.sum)
        if tuple(rgb.shape[1:]) != tuple(self.sum.shape) or rgb.device != self.sum.device:
            raise ValueError("every frame of a background-stability sequence must have one size and device")
        lib = _lib.load()
        dev = rgb.device
        with torch.cuda.device(dev):
            for f in range(rgb.shape[0]):
                _lib.check(lib.nrnerf_stability_accumulate(_ptr(rgb[f]), rgb[f].numel(), _ptr(self.sum), _ptr(self.sum_sq), _stream(dev)),
                           "nrnerf_stability_accumulate")
        self.count += rgb.shape[0]

    def finish(self):
        if self.count == 0:
            raise ValueError("BackgroundStability.finish() before any add()")
        H, W, _ = self.sum.shape
        dev = self.sum.device
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.nrnerf_stability_finish(_ptr(self.sum), _ptr(self.sum_sq), self.count, H * W, _ptr(out), _stream(dev)),
                       "nrnerf_stability_finish")
        return out


def volume_extent_of(checkpoint):
    """``(min_point, max_point)`` of a checkpoint's ``scripts_dict`` (fvr:617-622: ``min_nerf_volume_point`` / ``max_nerf_volume_point``,
    written by the reference's ``determine_nerf_volume_extent``), or None when the checkpoint does not carry them."""
    raw = getattr(checkpoint, "raw", checkpoint)
    sd = (raw or {}).get("scripts_dict") or {}
    if "min_nerf_volume_point" in sd and "max_nerf_volume_point" in sd:
        return (np.asarray(sd["min_nerf_volume_point"], dtype=np.float64).reshape(3),
                np.asarray(sd["max_nerf_volume_point"], dtype=np.float64).reshape(3))
    return None
