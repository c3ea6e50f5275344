"""The radiance field on a regular grid: density, colour and rigidity volumes of a fitted model.

``sample_grid`` evaluates the networks at the vertices of a box -- what NeRF-family users do with the reference's
``network_query_fn`` (train.py:633-649) to cut slices, extract iso-surfaces or build occupancy grids -- without an array of raw
network outputs for the whole grid ever existing: the grid is walked in slabs of whole x-rows through ``nrnerf_grid_points`` ->
``nrnerf_query`` -> ``nrnerf_field_from_raw``, all on the device.
"""
from __future__ import annotations

import copy
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from . import render as R

_canonical_views = weakref.WeakKeyDictionary()      # network -> its bender-free view (shares the parameters)


def grid_shape(resolution):
    """``resolution`` (an int, or ``(Gx, Gy, Gz)``) -> ``(Gx, Gy, Gz)``; each 1 .. MAX_SAMPLES (a grid row is one query row).  Pure."""
    if isinstance(resolution, (int, np.integer)):
        g = (int(resolution),) * 3
    else:
        g = tuple(int(v) for v in resolution)
        if len(g) != 3:
            raise ValueError(f"resolution must be an int or (Gx, Gy, Gz), got {resolution!r}")
    if any(v < 1 or v > _lib.MAX_SAMPLES for v in g):
        raise ValueError(f"every grid resolution must be in 1 .. {_lib.MAX_SAMPLES}, got {g}")
    return g


def grid_extent(min_point, max_point):
    """The box as two float32 triples; ``min <= max`` per axis.  Pure."""
    lo = np.asarray(min_point, dtype=np.float64).reshape(-1)
    hi = np.asarray(max_point, dtype=np.float64).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,):
        raise ValueError("min_point and max_point must have three coordinates each")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi < lo).any():
        raise ValueError(f"the grid box needs finite corners with min <= max, got {lo} .. {hi}")
    return lo.astype(np.float32), hi.astype(np.float32)


def plan_slabs(n_rows: int, rows_per_launch: int | None):
    """The launches of a grid of ``n_rows`` x-rows: ``[(first_row, rows), ...]``, whole rows, in order, covering every row once.
    ``rows_per_launch=None``: one slab.  Pure."""
    n_rows = int(n_rows)
    if n_rows < 0:
        raise ValueError("n_rows >= 0")
    per = n_rows if rows_per_launch is None else int(rows_per_launch)
    if rows_per_launch is not None and per < 1:
        raise ValueError("rows_per_launch >= 1")
    return [(r, min(per, n_rows - r)) for r in range(0, n_rows, max(per, 1))]


def default_rows_per_launch(gx: int) -> int:
    """Rows per slab when the caller does not say: about 2^20 samples (16 MiB of raw values, a few ms of kernel time)."""
    return max(1, (1 << 20) // max(int(gx), 1))


def grid_points(min_point, max_point, resolution, first_row=0, n_rows=None, device=None) -> torch.Tensor:
    """``nrnerf_grid_points``: rows ``[first_row, first_row + n_rows)`` of the grid as ``[n_rows, Gx, 4]`` (w = 0); row = iz * Gy + iy."""
    gx, gy, gz = grid_shape(resolution)
    lo, hi = grid_extent(min_point, max_point)
    n_rows = gy * gz - first_row if n_rows is None else int(n_rows)
    dev = torch.device(device if device is not None else "cuda")
    dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
    out = torch.empty((n_rows, gx, 4), dtype=torch.float32, device=dev)
    fp = C.POINTER(C.c_float)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nrnerf_grid_points(lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), gx, gy, gz, int(first_row), n_rows, out.data_ptr(),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "nrnerf_grid_points")
    return out


def field_from_raw(raw: torch.Tensor):
    """``nrnerf_field_from_raw``: ``raw [..., C >= 4]`` -> ``(sigma [...] float32 = relu(raw[..., 3]), rgb [..., 3] uint8 = to8b(sigmoid(raw[..., :3])))``."""
    raw = raw.to(torch.float32).contiguous()
    n, ch = raw.numel() // raw.shape[-1], int(raw.shape[-1])
    sigma = torch.empty(raw.shape[:-1], dtype=torch.float32, device=raw.device)
    rgb = torch.empty(tuple(raw.shape[:-1]) + (3,), dtype=torch.uint8, device=raw.device)
    with torch.cuda.device(raw.device):
        _lib.check(_lib.load().nrnerf_field_from_raw(raw.data_ptr(), ch, n, sigma.data_ptr(), rgb.data_ptr(),
                                                     C.c_void_p(torch.cuda.current_stream(raw.device).cuda_stream)), "nrnerf_field_from_raw")
    return sigma, rgb


def canonical_view(network):
    """``network`` without its ray bender: a shallow copy that shares every parameter (so the handle cache's staleness rules see the
    same tensors) and carries ``ray_bender = (None,)`` -- the canonical volume."""
    view = _canonical_views.get(network)
    if view is None:
        view = copy.copy(network)
        view.ray_bender = (None,)
        _canonical_views[network] = view
    return view


def sample_grid(render_kwargs, latent, min_point=None, max_point=None, resolution=64, *, fine=True, with_bending=True,
                rows_per_launch=None, viewdirs=None, precision=None, checkpoint=None):
    """Density, colour and rigidity of the field at the vertices of a regular grid over ``[min_point, max_point]``.

    ``render_kwargs``: the dictionary ``load_checkpoint`` / ``create_nerf`` returns (``network_fn``, ``network_fine``); ``fine`` picks
    ``network_fine`` when there is one.  ``latent``: the deformation code of ONE time step, ``[latent_size]`` or ``[1, latent_size]`` (ignored by
    a model that takes none).  ``resolution``: an int or ``(Gx, Gy, Gz)``, each <= ``MAX_SAMPLES``.  The extent defaults to
    ``visualize.volume_extent_of(checkpoint)``.  ``with_bending=False`` samples the CANONICAL volume: the same networks without the ray bender.

    Returns ``{"sigma": float32 [Gz, Gy, Gx] = relu(raw sigma), "rgb": uint8 [Gz, Gy, Gx, 3] = to8b(sigmoid(raw rgb)), "rigidity": float32
    [Gz, Gy, Gx]}`` (``rigidity`` only with a bender), on the device.  Vertex ``(ix, iy, iz)`` is ``min + i * (max - min) / (G - 1)`` per axis
    (``G == 1``: ``min``).  The grid is evaluated in slabs of ``rows_per_launch`` whole x-rows (default: about 2^20 samples); the result does not
    depend on the slab size.

    Colour of a view-dependent model: without a bender it is the colour seen along ``viewdirs`` (one unit direction ``[3]``, default +z
    ``(0, 0, 1)``), the same for every vertex; WITH a bender the reference takes a sample's direction from the finite difference of the bent
    points along its row (rnh:339-351), here the grid's x-rows -- the colour is that of a ray travelling along +x through the bent volume (so
    ``Gx >= 2`` is needed).  ``sigma`` and ``rigidity`` do not depend on the direction."""
    net = render_kwargs.get("network_fine") if fine and render_kwargs.get("network_fine") is not None else render_kwargs["network_fn"]
    if min_point is None or max_point is None:
        from .visualize import volume_extent_of
        ext = volume_extent_of(checkpoint) if checkpoint is not None else None
        if ext is None:
            raise ValueError("sample_grid needs min_point / max_point (or a checkpoint that carries its volume extent)")
        min_point, max_point = ext
    gx, gy, gz = grid_shape(resolution)
    lo, hi = grid_extent(min_point, max_point)
    if not with_bending:
        net = canonical_view(net)
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        if latent is not None and torch.is_tensor(latent) and latent.device.type == "cuda":
            dev = latent.device
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
    model = R.get_model(net, None, precision=precision, device=dev)
    dev = model.device
    n_rows = gy * gz
    slabs = plan_slabs(n_rows, default_rows_per_launch(gx) if rows_per_launch is None else rows_per_launch)
    lat = None
    if model.needs_latents:
        if latent is None:
            raise ValueError("this model needs a latent code")
        lat = torch.as_tensor(latent).to(device=dev, dtype=torch.float32).reshape(1, -1).contiguous()
    views = bool(getattr(net, "use_viewdirs", False))
    vd = None
    if views and not model.has_bender:
        vd = torch.as_tensor((0.0, 0.0, 1.0) if viewdirs is None else viewdirs, dtype=torch.float32).reshape(1, 3).to(dev)
    out = {"sigma": torch.empty((gz, gy, gx), dtype=torch.float32, device=dev),
           "rgb": torch.empty((gz, gy, gx, 3), dtype=torch.uint8, device=dev)}
    if model.has_bender:
        out["rigidity"] = torch.empty((gz, gy, gx), dtype=torch.float32, device=dev)
    sigma_rows, rgb_rows = out["sigma"].view(n_rows, gx), out["rgb"].view(n_rows, gx, 3)
    knobs = R._query_knobs(net)
    lib = _lib.load()
    fp = C.POINTER(C.c_float)
    ch = model.coarse_output_ch
    rows_max = max((n for _, n in slabs), default=0)
    pts = torch.empty((rows_max, gx, 4), dtype=torch.float32, device=dev)
    raw = torch.empty((rows_max, gx, ch), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for first, n in slabs:
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(lib.nrnerf_grid_points(lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), gx, gy, gz, first, n, pts.data_ptr(), stream),
                       "nrnerf_grid_points")
            dst = {"raw": raw[:n]}
            if model.has_bender:
                dst["rigidity_mask"] = out["rigidity"].view(n_rows, gx, 1)[first:first + n]
            try:
                model.query(pts[:n], None if lat is None else lat.expand(n, -1), None if vd is None else vd.expand(n, -1), 0, out=dst, **knobs)
            except _lib.NrnerfError as e:
                if e.status != _lib.ERR_UNSUPPORTED:
                    raise
                raise R.Unsupported(str(e)) from e
            _lib.check(lib.nrnerf_field_from_raw(raw.data_ptr(), ch, n * gx, sigma_rows[first:first + n].data_ptr(),
                                                 rgb_rows[first:first + n].data_ptr(), stream), "nrnerf_field_from_raw")
    return out
