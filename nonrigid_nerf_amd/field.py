"""The radiance field on a regular grid: density, colour and rigidity volumes of a fitted model.

``sample_grid`` evaluates the networks at the vertices of a box -- what NeRF-family users do with the reference's
``network_query_fn`` (train.py:633-649) to cut slices, extract iso-surfaces or build occupancy grids -- without an array of raw
network outputs for the whole grid ever existing: the grid is walked in slabs of whole x-rows through ``nrnerf_grid_points`` ->
``nrnerf_query`` -> ``nrnerf_field_from_raw``, all on the device.  ``bake`` keeps the raw logits of such a grid instead, and ``render_volume``
renders any time step from one canonical bake: the ray bender on the frame's samples, then a lookup-and-composite kernel, no network pass.
``bake_warp`` bakes the ray bender of a time step into a coarse offset grid as well, and ``render_baked`` renders a frame from the two bakes
alone: one kernel, no network, no model handle.
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


# --------------------------------------------------------------------------------------------
# iso-surface meshes of the field (nrnerf_isosurface_count / _emit: marching tetrahedra on the device)
# --------------------------------------------------------------------------------------------
def isosurface(volume: torch.Tensor, level, min_point, max_point, *, normals=True):
    """The iso-surface ``volume == level`` of a float32 volume ``[Gz, Gy, Gx]`` on the device (the layout of ``sample_grid``'s ``"sigma"``)
    over the box ``[min_point, max_point]``, by marching tetrahedra over the Kuhn triangulation of every cell.

    Returns ``{"vertices": float32 [V, 3], "faces": int32 [F, 3], "normals": float32 [V, 3]}`` (``normals`` only when asked for), on the
    device.  A grid vertex is inside iff ``value >= level`` (NaN is outside); every triangle's normal points from inside to outside -- for a
    density, towards lower density -- and ``normals`` is the unit ``-grad value`` at each vertex.  The mesh is closed away from the box faces,
    shares one vertex per grid edge, keeps zero-area triangles (a value equal to the level), and has the same bytes on every run; the exact
    definitions are in csrc/nrnerf_isosurface.h.  One host read -- the two totals, between the counting and the emitting pass -- is the only
    synchronisation.  Raises ``Unsupported`` for a mesh of 2^31 or more vertices or triangles, or a grid beyond 2^30 vertices."""
    if volume.device.type != "cuda":
        raise R.Unsupported("the volume is not on a ROCm device")
    if volume.dim() != 3:
        raise ValueError(f"volume must be [Gz, Gy, Gx], got {tuple(volume.shape)}")
    vol = volume.detach().to(torch.float32).contiguous()
    gz, gy, gx = (int(v) for v in vol.shape)
    if min(gx, gy, gz) < 1:
        raise ValueError("every grid resolution must be >= 1")
    lo, hi = grid_extent(min_point, max_point)
    dev = vol.device
    lib = _lib.load()
    a = _lib.IsosurfaceArgs()
    a.struct_size = C.sizeof(_lib.IsosurfaceArgs)
    a.value, a.gx, a.gy, a.gz, a.level = vol.data_ptr(), gx, gy, gz, float(level)
    a.min_point[:], a.max_point[:] = lo.tolist(), hi.tolist()
    need = int(lib.nrnerf_isosurface_workspace_bytes(gx, gy, gz))
    if need == 0 and min(gx, gy, gz) >= 2:
        raise R.Unsupported(f"a grid of {gx} x {gy} x {gz} vertices is beyond the {_lib.ISO_MAX_VERTICES} the iso-surface kernels index")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    a.workspace, a.workspace_bytes, a.totals = (ws.data_ptr() if need else None), need, totals.data_ptr()
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.nrnerf_isosurface_count(C.byref(a), stream), "nrnerf_isosurface_count")
        n_v, n_t = (int(v) for v in totals.tolist())                   # the one host read
        if n_v >= 1 << 31 or n_t >= 1 << 31:
            raise R.Unsupported(f"a mesh of {n_v} vertices and {n_t} triangles: faces are int32")
        out = {"vertices": torch.empty((n_v, 3), dtype=torch.float32, device=dev), "faces": torch.empty((n_t, 3), dtype=torch.int32, device=dev)}
        if normals:
            out["normals"] = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
        a.vertices, a.faces = (out["vertices"].data_ptr() or None), (out["faces"].data_ptr() or None)
        a.normals = (out["normals"].data_ptr() or None) if normals else None
        a.n_vertices, a.n_triangles = n_v, n_t
        _lib.check(lib.nrnerf_isosurface_emit(C.byref(a), stream), "nrnerf_isosurface_emit")
    return out


def density_along_rows(render_kwargs, latent, min_point, max_point, resolution, *, fine=True, precision=None, rows_per_launch=None):
    """The density grid of a model whose points NO point query takes (exact Jacobian view directions, a bender that is not a compiled shape:
    ``sample_grid`` raises ``Unsupported``), from the kernels that do take it -- the renderer's: every x-row of the grid is one ray from the
    row's first vertex along ``(max_x - min_x, 0, 0)`` with near 0, far 1 and ``Gx`` samples, one coarse pass, and ``sigma = relu(raw sigma)`` of
    its samples.  The samples are ``o + d * linspace(0, 1, Gx)`` in fp32: within a rounding of the grid's vertices in x, the same in y and z.
    Returns float32 ``[Gz, Gy, Gx]``; needs ``Gx >= 2``."""
    net = render_kwargs.get("network_fine") if fine and render_kwargs.get("network_fine") is not None else render_kwargs["network_fn"]
    gx, gy, gz = grid_shape(resolution)
    lo, hi = grid_extent(min_point, max_point)
    if gx < 2:
        raise R.Unsupported("a density grid along rays needs Gx >= 2")
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        dev = torch.device("cuda", torch.cuda.current_device())
    model = R.get_model(net, None, precision=precision, device=dev)
    dev = model.device
    n_rows = gy * gz
    lat = None
    if model.needs_latents:
        if latent is None:
            raise ValueError("this model needs a latent code")
        lat = torch.as_tensor(latent).to(device=dev, dtype=torch.float32).reshape(1, -1).contiguous()
    cols = [torch.tensor([float(hi[0]) - float(lo[0]), 0.0, 0.0, 0.0, 1.0], dtype=torch.float32, device=dev)]
    if getattr(net, "use_viewdirs", False):
        cols.append(torch.tensor([1.0, 0.0, 0.0], dtype=torch.float32, device=dev))
    tail = torch.cat(cols)
    knobs = R._query_knobs(net)
    sigma = torch.empty((gz, gy, gx), dtype=torch.float32, device=dev)
    rows = sigma.view(n_rows, gx)
    with torch.no_grad():
        for first, n in plan_slabs(n_rows, default_rows_per_launch(gx) if rows_per_launch is None else rows_per_launch):
            origins = grid_points(lo, hi, (1, gy, gz), first_row=first, n_rows=n, device=dev)[:, 0, :3]
            rays = torch.cat([origins, tail.expand(n, -1)], -1).contiguous()
            try:
                out = model.render(rays, None if lat is None else lat.expand(n, -1), gx, 0, retraw=True,
                                   rigidity_cutoff=knobs["rigidity_cutoff"], test_time_scaling=knobs["test_time_scaling"])
            except _lib.NrnerfError as e:
                if e.status != _lib.ERR_UNSUPPORTED:
                    raise
                raise R.Unsupported(str(e)) from e
            rows[first:first + n] = field_from_raw(out["raw"])[0]
    return sigma


def vertex_probe_step(min_point, max_point, resolution) -> float:
    """``h`` of ``extract_mesh``'s two-sample rows: one cell diagonal of the grid, rounded to float32.  Pure."""
    g = grid_shape(resolution)
    lo, hi = grid_extent(min_point, max_point)
    step = [(float(hi[c]) - float(lo[c])) / (g[c] - 1) if g[c] > 1 else 0.0 for c in range(3)]
    return float(np.float32(np.sqrt(sum(s * s for s in step))))


def query_vertices(network, vertices, normals, latent=None, *, probe_step=None, precision=None):
    """``query_points`` at mesh vertices under ``extract_mesh``'s view-direction rule -> ``(raw [V, C], details)``, each detail ``[V, .]``.
    No view-dependent head: a flat query.  A head without bender: ``viewdirs = -normal``, one vertex per row.  A head behind a bender: rows
    ``(v + probe_step * n, v)``, sample 1 -- its finite-difference direction (rnh:339-351) is that of a ray arriving along ``-normal``."""
    n_v = int(vertices.shape[0])
    views, has_bender = bool(getattr(network, "use_viewdirs", False)), R._bender_of(network) is not None
    lat = None if latent is None else torch.as_tensor(latent).to(device=vertices.device, dtype=torch.float32).reshape(1, -1).contiguous()
    rows_lat = None if lat is None else lat.expand(n_v, -1)
    with torch.no_grad():
        if not views:
            return R.query_points(vertices.contiguous(), network, lat, None, detailed_output=True, precision=precision)
        if has_bender:
            if probe_step is None:
                raise ValueError("a view-dependent head behind a ray bender needs probe_step")
            rows = torch.stack([vertices + float(probe_step) * normals, vertices], 1).contiguous()        # [V, 2, 3]
            raw, det = R.query_points(rows, network, rows_lat, None, detailed_output=True, precision=precision)
            return raw[:, 1].contiguous(), {k: v[:, 1] for k, v in det.items()}
        raw, det = R.query_points(vertices.reshape(n_v, 1, 3).contiguous(), network, rows_lat, (-normals).contiguous(), detailed_output=True,
                                  precision=precision)
        return raw[:, 0].contiguous(), {k: v[:, 0] for k, v in det.items()}


def extract_mesh(render_kwargs, latent, level, min_point=None, max_point=None, resolution=128, *, fine=True, with_bending=True, colors=True,
                 rigidity=True, precision=None, checkpoint=None, rows_per_launch=None):
    """The density iso-surface ``sigma == level`` of one time step (``latent``) -- or of the canonical volume, ``with_bending=False`` -- as a
    mesh with per-vertex attributes: ``sample_grid`` -> ``isosurface`` on ``"sigma"`` -> ``query_points`` at the mesh vertices, all on the device.

    Returns ``{"vertices", "faces", "normals"}`` as ``isosurface`` does, plus ``"rgb"`` uint8 ``[V, 3]`` (``colors``: ``field_from_raw`` of the
    query at the vertices) and ``"rigidity"`` float32 ``[V]`` (``rigidity``, only with a bender: the query's ``rigidity_mask``).  Vertices are in
    the space the grid was sampled in: the observed space of that time step, or canonical space.  ``render_kwargs``, ``latent``, ``fine``, the
    box (default: the checkpoint's volume extent), ``resolution``, ``precision`` and ``rows_per_launch`` are ``sample_grid``'s.

    Colour of a view-dependent model: that of a ray ARRIVING along ``-normal`` (``query_vertices``).  What ``query_points`` cannot take --
    exact (Jacobian) view directions, a bender that is not a compiled shape -- raises ``Unsupported``, unless ``colors=False, rigidity=False``
    ask for the geometry alone: the density grid then comes from the renderer's kernels, ``density_along_rows``."""
    net = render_kwargs.get("network_fine") if fine and render_kwargs.get("network_fine") is not None else render_kwargs["network_fn"]
    if min_point is None or max_point is None:
        from .visualize import volume_extent_of
        ext = volume_extent_of(checkpoint) if checkpoint is not None else None
        if ext is None:
            raise ValueError("extract_mesh needs min_point / max_point (or a checkpoint that carries its volume extent)")
        min_point, max_point = ext
    g = grid_shape(resolution)
    lo, hi = grid_extent(min_point, max_point)
    query_net = net if with_bending else canonical_view(net)
    has_bender = R._bender_of(query_net) is not None
    attributes = bool(colors) or (bool(rigidity) and has_bender)
    try:
        sigma = sample_grid({"network_fn": net}, latent, lo, hi, g, fine=False, with_bending=with_bending, rows_per_launch=rows_per_launch,
                            precision=precision)["sigma"]
    except R.Unsupported:
        if attributes:
            raise
        sigma = density_along_rows({"network_fn": query_net}, latent, lo, hi, g, fine=False, precision=precision, rows_per_launch=rows_per_launch)
    mesh = isosurface(sigma, level, lo, hi, normals=True)
    if not attributes:
        return mesh
    n_v, dev = int(mesh["vertices"].shape[0]), mesh["vertices"].device
    if n_v == 0:
        raw, det = torch.zeros((0, 4), device=dev), {"rigidity_mask": torch.zeros((0, 1), device=dev)}
    else:
        raw, det = query_vertices(query_net, mesh["vertices"], mesh["normals"], latent, probe_step=vertex_probe_step(lo, hi, g), precision=precision)
    if colors:
        mesh["rgb"] = field_from_raw(raw)[1] if n_v else torch.empty((0, 3), dtype=torch.uint8, device=dev)
    if rigidity and has_bender:
        mesh["rigidity"] = det["rigidity_mask"].reshape(n_v).contiguous()
    return mesh


# --------------------------------------------------------------------------------------------
# the bender walked backwards (nrnerf_bender_inverse): canonical points -> the observed space of a time step
# --------------------------------------------------------------------------------------------
def unbend_points(network, canonical_points, latent, *, initial=None, tol=1e-6, relaxation=1.0, max_iters=64, flags=None):
    """The observed points ``x`` of a time step whose bent image is ``canonical_points``: ``bend(x, latent) = c``, solved per point by the
    damped fixed-point iteration ``x <- x - relaxation (bend(x) - c)`` inside one kernel (``Model.bender_inverse``).

    ``canonical_points``: ``[N, S, 3]`` with ``latent [N, latent_size]`` (a code per row), or a flat ``[M, 3]`` with ONE code (``[latent_size]`` or
    ``[1, latent_size]``; laid out as rows by ``plan_flat_rows``, as ``query_points`` does).  ``initial``: a first guess of the same shape
    (default: the canonical points).  A point is finished when ``max_c |bend(x)_c - c_c| <= tol`` or after ``max_iters`` (1 .. 1024)
    evaluations; ``0 < relaxation <= 1`` -- the map is not a contraction everywhere, less so under ``test_time_scaling > 1``, and a smaller
    factor then converges where 1 oscillates.  The knobs (``rigidity_test_time_cutoff``, ``test_time_scaling``) are read from the bender as
    ``query_points`` reads them: they are part of the map.

    Returns ``{"points", "residual", "iterations", "converged"}``: ``[N, S, 3]`` / ``[N, S]`` (flat: ``[M, 3]`` / ``[M]``); ``residual`` is that
    OF the returned point -- ``query_points(points, detailed_output=True)["input_pts"]`` on the fp32 handle differs from ``canonical_points`` by
    exactly it -- ``iterations`` (int32) the evaluations made, ``converged = residual <= tol``.  Always the FP32 handle of the network, whatever
    precision is selected for rendering: a 16-bit bender rounds the point itself.  A network without bender returns the points themselves
    (``iterations`` 0, all converged).  Raises ``Unsupported`` for a bender shape without a compiled kernel, and under autograd."""
    pts = canonical_points
    if pts.device.type != "cuda":
        raise R.Unsupported("points are not on a ROCm device")
    lat_t = latent if torch.is_tensor(latent) else None
    if R._trains(network, None, pts, lat_t) or (initial is not None and torch.is_grad_enabled() and initial.requires_grad):
        raise R.Unsupported("autograd is enabled (the inverse has no gradient)")
    flat = pts.dim() == 2
    if pts.dim() not in (2, 3) or pts.shape[-1] != 3:
        raise ValueError(f"canonical_points must be [N, S, 3] or [M, 3], got {tuple(pts.shape)}")
    if initial is not None and tuple(initial.shape) != tuple(pts.shape):
        raise ValueError(f"initial must have the shape of canonical_points {tuple(pts.shape)}, got {tuple(initial.shape)}")
    dev = pts.device
    if R._bender_of(network) is None:
        p = pts.detach().to(torch.float32).clone()
        return {"points": p, "residual": torch.zeros(p.shape[:-1], dtype=torch.float32, device=dev),
                "iterations": torch.zeros(p.shape[:-1], dtype=torch.int32, device=dev),
                "converged": torch.ones(p.shape[:-1], dtype=torch.bool, device=dev)}
    if latent is None:
        raise ValueError("a ray bender needs a latent code")
    lat = torch.as_tensor(latent).detach().to(device=dev, dtype=torch.float32)
    pts = pts.detach()
    init = None if initial is None else initial.detach()
    if flat:
        M = int(pts.shape[0])
        n_rows, row, n_pad = R.plan_flat_rows(M)
        if lat.dim() == 1:
            lat = lat[None]
        if lat.dim() != 2 or lat.shape[0] != 1:
            raise ValueError("flat points take one latent code [1, latent_size]")
        lat = lat.contiguous().expand(n_rows, -1)

        def rows(t):
            if n_pad:
                t = torch.cat([t, t[-1:].expand(n_pad, -1)], 0)
            return t.reshape(n_rows, row, 3)
        pts = rows(pts)
        init = None if init is None else rows(init)
    model = R.get_model(network, None, precision="f32", device=dev)
    knobs = R._query_knobs(network)
    try:
        x, res, its = model.bender_inverse(pts, lat, init, tol=tol, relaxation=relaxation, max_iters=max_iters,
                                           rigidity_cutoff=knobs["rigidity_cutoff"], test_time_scaling=knobs["test_time_scaling"], flags=flags)
    except _lib.NrnerfError as e:
        if e.status != _lib.ERR_UNSUPPORTED:
            raise
        raise R.Unsupported(str(e)) from e
    if flat:
        x, res, its = x.reshape(-1, 3)[:M], res.reshape(-1)[:M], its.reshape(-1)[:M]
    return {"points": x, "residual": res, "iterations": its, "converged": res <= float(np.float32(tol))}


def vertex_normals(vertices, faces):
    """Area-weighted unit vertex normals of a triangle mesh, with torch ops on the tensors' device: the sum over a vertex's triangles of
    ``(v1 - v0) x (v2 - v0)`` (twice the area times the face normal), normalised.  Orientation follows the faces' winding -- for ``isosurface``'s
    faces, from inside to outside.  A vertex of no triangle, or of zero-area ones only, gets the zero vector.  ``[V, 3]`` float32."""
    v = vertices.to(torch.float32)
    f = faces.to(torch.int64)
    acc = torch.zeros_like(v)
    if f.numel():
        v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        fn = torch.cross(v1 - v0, v2 - v0, dim=-1)
        acc.index_put_((f.t().reshape(-1),), fn.repeat(3, 1), accumulate=True)
    length = acc.norm(dim=-1, keepdim=True)
    return torch.where(length > 0, acc / length.clamp_min(1e-30), torch.zeros_like(acc))


def animate_mesh(canonical_mesh, render_kwargs, latents, *, fine=True, warm_start=True, **solver):
    """A canonical mesh carried into every time step: ONE connectivity, the vertices moved by the inverse of the ray bender.

    ``canonical_mesh``: what ``extract_mesh(..., with_bending=False)`` returns.  ``latents``: the codes of the frames, ``[T, latent_size]`` (or a
    sequence of codes).  ``solver``: ``tol`` / ``relaxation`` / ``max_iters`` / ``flags`` of ``unbend_points``.  With ``warm_start`` frame t's
    solution is frame t + 1's first guess (neighbouring time steps deform alike: most vertices then finish in one or two evaluations).

    Returns one mesh per code, ``{"vertices", "normals", "converged", "residual", "faces"[, "rgb"][, "rigidity"]}``: ``faces`` / ``rgb`` /
    ``rigidity`` are the canonical mesh's own tensors, shared by every frame, and ``normals = vertex_normals`` of the moved vertices -- every
    frame has the same vertex count and connectivity, and ``write_ply`` takes a frame as it is."""
    net = render_kwargs.get("network_fine") if fine and render_kwargs.get("network_fine") is not None else render_kwargs["network_fn"]
    verts = canonical_mesh["vertices"].detach().to(torch.float32).contiguous()
    faces = canonical_mesh["faces"]
    codes = [latents[t] for t in range(len(latents))]
    shared = {key: canonical_mesh[key] for key in ("rgb", "rigidity") if canonical_mesh.get(key) is not None}
    out, guess = [], None
    with torch.no_grad():
        for code in codes:
            if verts.shape[0] == 0:
                sol = {"points": verts.clone(), "residual": verts.new_zeros((0,)), "converged": torch.ones((0,), dtype=torch.bool, device=verts.device)}
            else:
                sol = unbend_points(net, verts, torch.as_tensor(code).reshape(1, -1), initial=guess, **solver)
            if warm_start:
                guess = sol["points"]
            out.append({"vertices": sol["points"], "normals": vertex_normals(sol["points"], faces), "converged": sol["converged"],
                        "residual": sol["residual"], "faces": faces, **shared})
    return out


def track_points(render_kwargs, points, latent_from, latents_to, *, fine=True, **solver):
    """Points seen in one time step found again in others: ``points [M, 3]`` of the observed space of ``latent_from`` are bent to canonical
    space (``query_points(..., detailed_output=True)``'s ``input_pts`` on the fp32 handle) and from there carried into each code of
    ``latents_to`` by one ``unbend_points`` call (``solver``: its ``tol`` / ``relaxation`` / ``max_iters`` / ``flags``).

    Returns ``{"canonical": [M, 3], "tracks": [{"points", "residual", "iterations", "converged"}, ...]}``, one entry per target code."""
    net = render_kwargs.get("network_fine") if fine and render_kwargs.get("network_fine") is not None else render_kwargs["network_fn"]
    if points.dim() != 2 or points.shape[-1] != 3:
        raise ValueError(f"points must be [M, 3], got {tuple(points.shape)}")
    with torch.no_grad():
        pts = points.detach().to(torch.float32).contiguous()
        if R._bender_of(net) is None:
            canonical = pts.clone()
        else:
            # rows of 64 (the bent point of a sample does not depend on its row; a view-dependent head behind a bender refuses flat input)
            M = int(pts.shape[0])
            n_rows, row, n_pad = R.plan_flat_rows(M)
            rows = torch.cat([pts, pts[-1:].expand(n_pad, -1)], 0) if n_pad else pts
            lat = torch.as_tensor(latent_from).to(device=pts.device, dtype=torch.float32).reshape(1, -1).contiguous()
            if M == 0:
                canonical = pts.clone()
            else:
                det = R.query_points(rows.reshape(n_rows, row, 3), net, lat.expand(n_rows, -1), None, detailed_output=True, precision="f32")[1]
                canonical = det["input_pts"].reshape(-1, 3)[:M].contiguous()
        tracks = [unbend_points(net, canonical, torch.as_tensor(latents_to[t]).reshape(1, -1), **solver) for t in range(len(latents_to))]
    return {"canonical": canonical, "tracks": tracks}


def write_ply(path, mesh) -> None:
    """``mesh`` (what ``isosurface`` / ``extract_mesh`` return; tensors or arrays) as a binary little-endian PLY: vertex properties ``x y z``
    ``[nx ny nz]`` ``[red green blue]`` ``[rigidity]`` -- the bracketed ones when the mesh carries ``"normals"`` / ``"rgb"`` / ``"rigidity"`` --
    and faces as ``uchar int vertex_indices``.  numpy only; the one place the mesh comes to the host."""
    def host(v, dtype):
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        return np.ascontiguousarray(v, dtype=dtype)

    verts = host(mesh["vertices"], "<f4").reshape(-1, 3)
    faces = host(mesh["faces"], "<i4").reshape(-1, 3)
    n_v = verts.shape[0]
    fields, cols, header = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")], [verts[:, 0], verts[:, 1], verts[:, 2]], ["float x", "float y", "float z"]
    if mesh.get("normals") is not None:
        nrm = host(mesh["normals"], "<f4").reshape(n_v, 3)
        for c, name in enumerate(("nx", "ny", "nz")):
            fields.append((name, "<f4")); cols.append(nrm[:, c]); header.append(f"float {name}")
    if mesh.get("rgb") is not None:
        rgb = host(mesh["rgb"], "u1").reshape(n_v, 3)
        for c, name in enumerate(("red", "green", "blue")):
            fields.append((name, "u1")); cols.append(rgb[:, c]); header.append(f"uchar {name}")
    if mesh.get("rigidity") is not None:
        fields.append(("rigidity", "<f4")); cols.append(host(mesh["rigidity"], "<f4").reshape(n_v)); header.append("float rigidity")
    vrec = np.empty(n_v, dtype=np.dtype(fields))            # packed: no padding between the properties
    for (name, _), col in zip(fields, cols):
        vrec[name] = col
    frec = np.empty(faces.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    frec["n"], frec["v"] = 3, faces
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n_v}"] + [f"property {h}" for h in header] + \
            [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


# --------------------------------------------------------------------------------------------
# baked volumes of the field (nrnerf_volume_render / nrnerf_bend_points): bake once, render every frame by lookup
# --------------------------------------------------------------------------------------------
_VOLUME_DTYPES = {torch.float32: _lib.VOLUME_F32, torch.float16: _lib.VOLUME_F16}


def volume_grid_shape(resolution):
    """``grid_shape`` for a volume that is interpolated: every axis needs two vertices, and the grid at most 2^30 of them.  Pure."""
    g = grid_shape(resolution)
    if min(g) < 2:
        raise ValueError(f"a baked volume needs at least 2 vertices per axis, got {g}")
    if g[0] * g[1] * g[2] > _lib.VOLUME_MAX_VERTICES:
        raise ValueError(f"a baked volume has at most {_lib.VOLUME_MAX_VERTICES} vertices, got {g}")
    return g


def _lebedev_26():
    """The 26-point Lebedev rule on the sphere, exact to degree 7: ``(directions [26, 3], weights [26])`` in float64, the weights summing to 1
    (the integral over the sphere is ``4 pi sum_d w_d f(d)``).  Six axis directions (1/21), twelve edge directions (4/105), eight corner
    directions (9/280), in this fixed order: the order ``bake`` accumulates in."""
    axes = [(s if c == 0 else 0.0, s if c == 1 else 0.0, s if c == 2 else 0.0) for c in range(3) for s in (1.0, -1.0)]
    edges = [tuple(0.0 if c == skip else (s0 if c == (skip + 1) % 3 else s1) for c in range(3))
             for skip in (2, 0, 1) for s0 in (1.0, -1.0) for s1 in (1.0, -1.0)]
    corners = [(sx, sy, sz) for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
    d = np.asarray(axes + edges + corners, dtype=np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    w = np.asarray([1.0 / 21.0] * 6 + [4.0 / 105.0] * 12 + [9.0 / 280.0] * 8, dtype=np.float64)
    return d, w


SH_DIRECTIONS, SH_WEIGHTS = _lebedev_26()
_SH_C0, _SH_C1, _SH_C2, _SH_C20, _SH_C22 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396


def sh_channels(degree: int) -> int:
    """Channels per vertex of the ``"sh"`` array of a bake of ``degree`` 1 or 2: 12 (9 coefficients and 3 zeros) or 24.  Pure."""
    if degree not in (1, 2):
        raise ValueError(f"an sh array has degree 1 or 2, got {degree!r}")
    return 12 * degree


def sh_basis(dirs, degree):
    """The real spherical harmonics ``Y_0 .. Y_{K-1}``, ``K = (degree + 1)^2``, at directions ``dirs [..., 3]`` (float32 or float64 tensor; the
    result has its dtype): ``[..., K]`` in the order and with the operation order of include/nrnerf.h ("view-dependent bakes").  Pure."""
    degree = int(degree)
    if not 0 <= degree <= _lib.SH_MAX_DEGREE:
        raise ValueError(f"sh_degree is 0 .. {_lib.SH_MAX_DEGREE}, got {degree}")
    d = torch.as_tensor(dirs)
    if d.dtype not in (torch.float32, torch.float64) or d.shape[-1] != 3:
        raise ValueError(f"dirs must be float32 or float64 [..., 3], got {d.dtype} {tuple(d.shape)}")
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = [torch.full_like(x, _SH_C0)]
    if degree >= 1:
        out += [_SH_C1 * -y, _SH_C1 * z, _SH_C1 * -x]
    if degree >= 2:
        xx, yy, zz = x * x, y * y, z * z
        out += [_SH_C2 * (x * y), -_SH_C2 * (y * z), _SH_C20 * ((2.0 * zz - xx) - yy), -_SH_C2 * (x * z), _SH_C22 * (xx - yy)]
    return torch.stack(out, -1)


def bake(render_kwargs, latent=None, min_point=None, max_point=None, resolution=128, *, fine=True, with_bending=False, dtype=torch.float32,
         rows_per_launch=None, precision=None, checkpoint=None, sh_degree=None):
    """The field's raw outputs on a regular grid, kept as LOGITS: ``{"raw": [Gz, Gy, Gx, 4] (r, g, b, sigma before the sigmoid / relu),
    "min_point", "max_point"}`` -- what ``render_volume`` interpolates.  ``sample_grid``'s slab loop (``nrnerf_grid_points`` -> ``nrnerf_query``)
    writing the first four raw channels instead of going through ``nrnerf_field_from_raw``; the result does not depend on ``rows_per_launch``.

    ``with_bending=False`` (the default) bakes the CANONICAL volume, which does not depend on time: one bake serves every time step, the ray
    bender is applied to the samples at render time.  ``with_bending=True`` bakes the observed space of ONE time step (``latent``); the
    time-conditioned baseline always bakes per code.  ``dtype``: ``torch.float32`` or ``torch.float16`` (the float32 bake rounded once; 8 bytes
    per vertex).  ``resolution``: an int or ``(Gx, Gy, Gz)``, each 2 .. ``MAX_SAMPLES``.  The extent defaults to the checkpoint's volume extent.
    A view-dependent head raises ``Unsupported``: its colour is not a function of position -- unless ``sh_degree`` says how to keep the
    dependence.

    ``sh_degree = L`` in 0 .. 2 (a view-dependent head only; ``ValueError`` on any other): the colour logits are projected onto the real
    spherical harmonics of degree <= L with the 26-point Lebedev rule (``SH_DIRECTIONS``, ``SH_WEIGHTS``; exact to degree 7, so the nine
    functions are orthonormal under it) -- one pass of the slab loop per direction, every vertex queried with that direction.  The record:
    ``"raw"`` = (the MEAN colour logits over the directions, the sigma logit of the first direction), a valid volume for every call that takes
    one (it renders the direction-averaged colour); ``"sh" [Gz, Gy, Gx, 12 L]`` (``L >= 1``) = the coefficients of basis function ``k = 1 ..
    (L + 1)^2 - 1`` of colour ``c`` at channel ``3 (k - 1) + c`` (``L = 1``: channels 9 .. 11 are zero), in ``dtype``; ``"sh_degree": L``.
    ``raw_c = sum_d w_d f_c(d)`` and ``sh_{k,c} = sum_d (4 pi w_d Y_k(d)) f_c(d)``, accumulated in float32 in the order of the direction table,
    rounded to ``dtype`` once.  ``render_volume`` / ``render_baked`` evaluate the sum at each sample's direction (``sh_volume_render``).  Behind a
    ray bender the head's direction comes from its row neighbours (rnh:339-351), which a grid vertex does not have: ``with_bending=True``
    stays ``Unsupported`` there -- bake the canonical volume and render it through a warp."""
    if dtype not in _VOLUME_DTYPES:
        raise ValueError(f"a baked volume is float32 or float16, got {dtype}")
    net = render_kwargs.get("network_fine") if fine and render_kwargs.get("network_fine") is not None else render_kwargs["network_fn"]
    views = bool(getattr(net, "use_viewdirs", False))
    if sh_degree is not None:
        if isinstance(sh_degree, bool) or not isinstance(sh_degree, (int, np.integer)) or not 0 <= int(sh_degree) <= _lib.SH_MAX_DEGREE:
            raise ValueError(f"sh_degree is None or 0 .. {_lib.SH_MAX_DEGREE}, got {sh_degree!r}")
        if not views:
            raise ValueError("sh_degree is for a view-dependent head: this one's colour is a function of position, bake it without")
        sh_degree = int(sh_degree)
        if with_bending and R._bender_of(net) is not None:
            raise R.Unsupported("a view-dependent head behind a ray bender takes its direction from a sample's row neighbours, which a grid "
                                "vertex does not have: bake the canonical volume (with_bending=False)")
    elif views:
        raise R.Unsupported("a view-dependent head cannot be baked: its colour is not a function of position (sh_degree keeps the dependence)")
    if min_point is None or max_point is None:
        from .visualize import volume_extent_of
        ext = volume_extent_of(checkpoint) if checkpoint is not None else None
        if ext is None:
            raise ValueError("bake needs min_point / max_point (or a checkpoint that carries its volume extent)")
        min_point, max_point = ext
    gx, gy, gz = volume_grid_shape(resolution)
    lo, hi = grid_extent(min_point, max_point)
    if not (hi > lo).all():
        raise ValueError(f"a baked volume needs min < max on every axis, got {lo} .. {hi}")
    if not with_bending:
        net = canonical_view(net)
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        dev = latent.device if torch.is_tensor(latent) and latent.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    model = R.get_model(net, None, precision=precision, device=dev)
    dev = model.device
    lat = None
    if model.needs_latents:
        if latent is None:
            raise ValueError("this model needs a latent code")
        lat = torch.as_tensor(latent).to(device=dev, dtype=torch.float32).reshape(1, -1).contiguous()
    n_rows = gy * gz
    slabs = plan_slabs(n_rows, default_rows_per_launch(gx) if rows_per_launch is None else rows_per_launch)
    vol = torch.empty((gz, gy, gx, 4), dtype=dtype, device=dev)
    vol_rows = vol.view(n_rows, gx, 4)
    knobs = R._query_knobs(net)
    lib = _lib.load()
    fp = C.POINTER(C.c_float)
    ch = model.coarse_output_ch
    rows_max = max(n for _, n in slabs)
    pts = torch.empty((rows_max, gx, 4), dtype=torch.float32, device=dev)
    raw = torch.empty((rows_max, gx, ch), dtype=torch.float32, device=dev)
    sh = sh_rows = None
    if sh_degree is not None:
        if model.has_bender:
            raise R.Unsupported("a view-dependent head behind a ray bender cannot be baked per time step: bake the canonical volume")
        basis = sh_basis(torch.from_numpy(SH_DIRECTIONS), sh_degree)                                           # float64 [26, K]
        dirs = torch.from_numpy(SH_DIRECTIONS).to(device=dev, dtype=torch.float32).contiguous()
        weights = torch.from_numpy(SH_WEIGHTS).to(device=dev, dtype=torch.float32)
        coef = (4.0 * np.pi * torch.from_numpy(SH_WEIGHTS)[:, None] * basis[:, 1:]).to(device=dev, dtype=torch.float32)     # [26, K - 1]
        n_coef = int(coef.shape[1])
        acc_raw = torch.empty((rows_max, gx, 4), dtype=torch.float32, device=dev)
        if sh_degree >= 1:
            sh = torch.empty((gz, gy, gx, sh_channels(sh_degree)), dtype=dtype, device=dev)
            sh_rows = sh.view(n_rows, gx, sh_channels(sh_degree))
            acc_sh = torch.empty((rows_max, gx, sh_channels(sh_degree) // 3, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), torch.no_grad():
        for first, n in slabs:
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(lib.nrnerf_grid_points(lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), gx, gy, gz, first, n, pts.data_ptr(), stream),
                       "nrnerf_grid_points")
            if sh_degree is None:
                try:
                    model.query(pts[:n], None if lat is None else lat.expand(n, -1), None, 0, out={"raw": raw[:n]}, **knobs)
                except _lib.NrnerfError as e:
                    if e.status != _lib.ERR_UNSUPPORTED:
                        raise
                    raise R.Unsupported(str(e)) from e
                vol_rows[first:first + n].copy_(raw[:n, :, :4])
                continue
            # one query per direction, the same direction for every vertex of the slab; per vertex the sums run in the table's order
            acc_raw[:n].zero_()
            if sh_rows is not None:
                acc_sh[:n].zero_()
            for d in range(len(SH_WEIGHTS)):
                try:
                    model.query(pts[:n], None if lat is None else lat.expand(n, -1), dirs[d:d + 1].expand(n, -1), 0, out={"raw": raw[:n]}, **knobs)
                except _lib.NrnerfError as e:
                    if e.status != _lib.ERR_UNSUPPORTED:
                        raise
                    raise R.Unsupported(str(e)) from e
                if d == 0:
                    acc_raw[:n, :, 3].copy_(raw[:n, :, 3])
                acc_raw[:n, :, :3].add_(raw[:n, :, :3] * weights[d])
                if sh_rows is not None:
                    acc_sh[:n, :, :n_coef].add_(raw[:n, :, None, :3] * coef[d][:, None])
            vol_rows[first:first + n].copy_(acc_raw[:n])
            if sh_rows is not None:
                sh_rows[first:first + n].copy_(acc_sh[:n].view(n, gx, -1))
    if sh_degree is None:
        return {"raw": vol, "min_point": lo, "max_point": hi}
    record = {"raw": vol, "sh_degree": sh_degree, "min_point": lo, "max_point": hi}
    if sh is not None:
        record["sh"] = sh
    return record


def _grid_parts(record, key, noun):
    """``record[key]`` (what ``bake`` / ``bake_warp`` return) -> ``(grid [Gz, Gy, Gx, 4] contiguous on the device, lo, hi, (Gx, Gy, Gz))``."""
    grid = record[key]
    if not torch.is_tensor(grid) or grid.device.type != "cuda":
        raise R.Unsupported(f"the {noun} is not on a ROCm device")
    if grid.dim() != 4 or grid.shape[-1] != 4 or grid.dtype not in _VOLUME_DTYPES:
        raise ValueError(f"a {noun} is float32 or float16 [Gz, Gy, Gx, 4], got {grid.dtype} {tuple(grid.shape)}")
    gz, gy, gx = (int(v) for v in grid.shape[:3])
    if min(gx, gy, gz) < 2 or gx * gy * gz > _lib.VOLUME_MAX_VERTICES:
        raise ValueError(f"a {noun} has 2 or more vertices per axis and at most {_lib.VOLUME_MAX_VERTICES} in all, got {(gx, gy, gz)}")
    lo, hi = grid_extent(record["min_point"], record["max_point"])
    if not (hi > lo).all():
        raise ValueError(f"a {noun} needs min < max on every axis, got {lo} .. {hi}")
    return grid.detach().contiguous(), lo, hi, (gx, gy, gz)


def _render_front(a, dev, rays, N_samples, z_vals, lindisp, white_bkgd):
    """The front the two baked-render wrappers share: checks and converts ``rays`` and ``z_vals`` and fills the fields the argument structs
    ``a`` have in common.  Returns ``(N, S, keep)``; ``keep`` holds the converted tensors, to stay alive over the call."""
    f32 = dict(dtype=torch.float32, device=dev)
    if rays.dim() != 2 or rays.shape[1] < 8:
        raise ValueError(f"rays must be [N, >= 8], got {tuple(rays.shape)}")
    rays = rays.detach().to(**f32).contiguous()
    N, S = int(rays.shape[0]), int(N_samples)
    if not 1 <= S <= _lib.MAX_SAMPLES:
        raise ValueError(f"1 <= N_samples <= {_lib.MAX_SAMPLES}, got {S}")
    a.struct_size = C.sizeof(a)
    a.n_rays, a.n_samples = N, S
    a.rays, a.ray_stride = rays.data_ptr() or None, int(rays.shape[1])
    a.lindisp, a.white_bkgd = int(bool(lindisp)), int(bool(white_bkgd))
    if z_vals is not None:
        if tuple(z_vals.shape) != (N, S):
            raise ValueError(f"z_vals must be {(N, S)}, got {tuple(z_vals.shape)}")
        z_vals = z_vals.detach().to(**f32).contiguous()
        a.z = z_vals.data_ptr() or None
    return N, S, (rays, z_vals)


def _render_outputs(a, dev, N, S, composite, weights, alpha, surface):
    """The back the two wrappers share: the maps, weights, alpha and surface outputs, allocated and named in ``a``.  Returns ``(out, new)``:
    the dict of results and the allocator ``new(key, *shape)`` that adds to it."""
    out = {}

    def new(key, *shape, dtype=torch.float32):
        out[key] = torch.empty(shape, dtype=dtype, device=dev)
        return out[key].data_ptr() or None

    if composite:
        a.rgb, a.disp, a.acc = new("rgb_map", N, 3), new("disp_map", N), new("acc_map", N)
        if weights:
            a.weights = new("weights", N, S)
        if alpha:
            a.alpha = new("alpha", N, S)
        if surface:
            a.surface_pts, a.surface_rigidity = new("surface_pts", N, 3), new("surface_rigidity", N)
            a.median_index = new("median_index", N, dtype=torch.int32)
    elif weights or alpha or surface:
        raise ValueError("weights, alpha and the surface outputs come from compositing")
    return out, new


def volume_render(volume, rays, *, N_samples, z_vals=None, points4=None, lindisp=False, white_bkgd=False, removal_threshold=None,
                  composite=True, retraw=False, weights=False, alpha=False, surface=False):
    """``nrnerf_volume_render`` on tensors: the volume's logits at the ``N_samples`` samples of every ray -- ``points4 [N, S, 4]`` (xyz, rigidity),
    or ``o + d z`` -- and their compositing.  ``rays [N, >= 8]``; ``z_vals [N, S]`` or the coarse spacing between the rays' near and far.
    Returns ``rgb_map / disp_map / acc_map`` (+ ``raw``, ``weights``, ``alpha``, ``surface_pts``, ``surface_rigidity``, ``median_index`` as asked
    for); ``composite=False`` runs the lookup alone and returns ``raw``.  The sampling rule: include/nrnerf.h."""
    vol, lo, hi, g = _grid_parts(volume, "raw", "volume")
    dev = vol.device
    a = _lib.VolumeRenderArgs()
    N, S, keep = _render_front(a, dev, rays, N_samples, z_vals, lindisp, white_bkgd)
    if points4 is not None:
        if tuple(points4.shape) != (N, S, 4):
            raise ValueError(f"points4 must be {(N, S, 4)}, got {tuple(points4.shape)}")
        points4 = points4.detach().to(dtype=torch.float32, device=dev).contiguous()
        a.points4 = points4.data_ptr() or None
    elif removal_threshold is not None or surface:
        raise ValueError("a removal threshold and the surface outputs need points4")
    a.volume, a.volume_dtype = vol.data_ptr(), _VOLUME_DTYPES[vol.dtype]
    a.g[:] = g
    a.min_point[:], a.max_point[:] = lo.tolist(), hi.tolist()
    if removal_threshold is not None:
        a.has_removal_threshold, a.removal_threshold = 1, float(removal_threshold)
    out, new = _render_outputs(a, dev, N, S, composite, weights, alpha, surface)
    if retraw or not composite:
        a.raw = new("raw", N, S, 4)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nrnerf_volume_render(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "nrnerf_volume_render")
    return out


def sample_rays(rays, N_samples, lindisp=False):
    """``nrnerf_sample_depths_points`` without jitter: ``(z [N, S], points [N, S, 3])`` of the coarse spacing, ``S >= 2``."""
    N, S = int(rays.shape[0]), int(N_samples)
    dev = rays.device
    z = torch.empty((N, S), dtype=torch.float32, device=dev)
    pts = torch.empty((N, S, 3), dtype=torch.float32, device=dev)
    if N:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().nrnerf_sample_depths_points(rays.data_ptr(), int(rays.shape[1]), None, N, S, int(bool(lindisp)), z.data_ptr(),
                                                               pts.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                       "nrnerf_sample_depths_points")
    return z, pts


def render_volume(volume, rays, *, network=None, latents=None, N_samples=192, z_vals=None, lindisp=False, white_bkgd=False, surface=False,
                  retraw=False, removal_threshold=None, precision=None, occupancy=None, N_importance=0, importance_u=None, fused=None):
    """A baked volume rendered along ``rays [N, >= 8]``: ``rgb_map / disp_map / acc_map`` (+ ``raw`` under ``retraw``; ``surface_pts``,
    ``surface_rigidity``, ``median_index`` under ``surface``), no trunk pass.

    ``network`` with a ray bender and a CANONICAL bake: the samples (``N_samples`` of the coarse spacing, ``lindisp`` honoured, or ``z_vals
    [N, S]``) are bent with ``latents`` (``[N, latent_size]``, or one code ``[latent_size]`` / ``[1, latent_size]`` for all rays) by
    ``nrnerf_bend_points`` -- the modules' knobs (``rigidity_test_time_cutoff``, ``test_time_scaling``, and the removal threshold unless
    ``removal_threshold`` is given) as ``query_points`` reads them -- and looked up at the bent points: any time step, motion exaggeration and
    background stabilisation included, from one bake.  Without ``network`` (or without a bender): straight rays, no bender launch -- a bake of
    one time step's observed space, or a static scene.  Refuses autograd inputs (``Unsupported``): a preview has no gradient.
    A volume record with ``"sh"`` (``bake(sh_degree=1 or 2)`` of a view-dependent head) goes through ``sh_volume_render`` instead: the colour
    of a sample is evaluated at its direction -- the difference of consecutive bent points behind a bender, the ray's direction without.
    ``occupancy``: the volume's mask (``build_occupancy``) -- samples in empty blocks request nothing, through ``culled_volume_render``; ``None``
    takes the calls above.
    ``N_importance > 0`` (without ``network``: the real bender between the two passes is ``Unsupported``): hierarchical sampling on straight
    rays, ``render_baked``'s -- ``importance_u``, ``fused`` and the additional results ``rgb0 / disp0 / acc0``, ``z_std``, ``z_vals`` as there."""
    if rays.device.type != "cuda":
        raise R.Unsupported("rays are not on a ROCm device")
    if int(N_importance) > 0:
        if network is not None:
            raise R.Unsupported("hierarchical sampling of a baked volume behind a network's ray bender (bake the bender: bake_warp, render_baked)")
        return _render_volume_hierarchical(volume, rays, int(N_samples), int(N_importance), z_vals, importance_u, lindisp, white_bkgd, surface,
                                           retraw, occupancy, fused)
    lat_t = latents if torch.is_tensor(latents) else None
    if torch.is_grad_enabled() and (rays.requires_grad or (lat_t is not None and lat_t.requires_grad) or volume["raw"].requires_grad
                                    or (z_vals is not None and z_vals.requires_grad)):
        raise R.Unsupported("autograd is enabled (rendering a baked volume has no gradient: render_baked_train has)")
    dev = rays.device
    rays = rays.detach().to(dtype=torch.float32).contiguous()
    N, S = int(rays.shape[0]), int(z_vals.shape[1] if z_vals is not None else N_samples)
    bender = R._bender_of(network) if network is not None else None
    with torch.no_grad():
        if z_vals is not None:
            z = z_vals.detach().to(device=dev, dtype=torch.float32).contiguous()
            pts = None
        elif S >= 2:
            z, pts = sample_rays(rays, S, lindisp)
        else:       # one sample: the near bound
            z, pts = (1.0 / (1.0 / rays[:, 6:7])).contiguous() if lindisp else rays[:, 6:7].contiguous(), None
        points4 = None
        if bender is not None or surface:
            if pts is None:
                pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]        # a product and a sum, each rounded, as the kernels'
        if bender is not None:
            if latents is None:
                raise ValueError("a ray bender needs latents")
            lat = torch.as_tensor(latents).detach().to(device=dev, dtype=torch.float32)
            if lat.dim() == 1:
                lat = lat[None]
            if lat.dim() != 2 or lat.shape[0] not in (1, N):
                raise ValueError(f"latents must be [N, latent_size] or one code, got {tuple(lat.shape)}")
            if lat.shape[0] == 1:
                lat = lat.contiguous().expand(N, -1)
            knobs = R._query_knobs(network)
            if removal_threshold is None:
                removal_threshold = knobs["removal_threshold"]
            model = R.get_model(network, None, precision=precision, device=dev)
            try:
                points4 = model.bend_points(pts, lat, rigidity_cutoff=knobs["rigidity_cutoff"], test_time_scaling=knobs["test_time_scaling"])
            except _lib.NrnerfError as e:
                if e.status != _lib.ERR_UNSUPPORTED:
                    raise
                raise R.Unsupported(str(e)) from e
        elif surface and not _has_sh(volume):
            points4 = torch.cat([pts, torch.zeros_like(pts[..., :1])], -1)
        if points4 is None:
            removal_threshold = None
        if _has_sh(volume):         # a view-dependent bake: bent points give the directions by differences, straight rays their own
            return sh_volume_render(volume, rays, N_samples=S, z_vals=z, points4=points4, lindisp=lindisp, white_bkgd=white_bkgd,
                                    removal_threshold=removal_threshold, retraw=retraw, surface=surface, occupancy=occupancy)
        if occupancy is not None:
            return culled_volume_render(volume, rays, occupancy=occupancy, use_sh=False, N_samples=S, z_vals=z, points4=points4,
                                        lindisp=lindisp, white_bkgd=white_bkgd, removal_threshold=removal_threshold, retraw=retraw,
                                        surface=surface)
        return volume_render(volume, rays, N_samples=S, z_vals=z, points4=points4, lindisp=lindisp, white_bkgd=white_bkgd,
                             removal_threshold=removal_threshold, retraw=retraw, surface=surface)


def _render_volume_hierarchical(volume, rays, N_samples, I, z_vals, importance_u, lindisp, white_bkgd, surface, retraw, occupancy, fused):
    """``render_volume(N_importance > 0)``: straight rays, the coarse depths ``render_volume`` takes (``z_vals``, or ``sample_rays``')."""
    if torch.is_grad_enabled() and (rays.requires_grad or volume["raw"].requires_grad or (z_vals is not None and z_vals.requires_grad)
                                    or (importance_u is not None and importance_u.requires_grad)):
        raise R.Unsupported("autograd is enabled (rendering a baked volume has no gradient: render_baked_train has)")
    dev = rays.device
    rays = rays.detach().to(dtype=torch.float32).contiguous()
    S = int(z_vals.shape[1] if z_vals is not None else N_samples)
    if S < 3:
        raise ValueError(f"hierarchical sampling needs N_samples >= 3, got {S}")
    with torch.no_grad():
        z = z_vals.detach().to(device=dev, dtype=torch.float32).contiguous() if z_vals is not None else sample_rays(rays, S, lindisp)[0]
        if _use_fused(fused, S, I, not _has_sh(volume) and occupancy is None):
            return hierarchical_volume_render(volume, None, rays, N_samples=S, N_importance=I, z_vals=z, importance_u=importance_u,
                                              lindisp=lindisp, white_bkgd=white_bkgd, retraw=retraw, surface=surface)

        def render(N_samples, z_vals, retraw=False, surface=False):
            points4 = None
            if surface and not _has_sh(volume):
                pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z_vals[..., None]   # a product and a sum, each rounded, as the kernels'
                points4 = torch.cat([pts, torch.zeros_like(pts[..., :1])], -1)
            kw = dict(N_samples=N_samples, z_vals=z_vals, points4=points4, lindisp=lindisp, white_bkgd=white_bkgd, retraw=retraw, surface=surface)
            if _has_sh(volume):
                return sh_volume_render(volume, rays, occupancy=occupancy, **kw)
            if occupancy is not None:
                return culled_volume_render(volume, rays, occupancy=occupancy, use_sh=False, **kw)
            return volume_render(volume, rays, **kw)
        return _render_hierarchical_composed(render, rays, S, I, z, importance_u, lindisp, white_bkgd, retraw=retraw, surface=surface)


def render_volume_frames(volume, render_poses, intrinsics, near, far, *, network=None, latents=None, **kwargs):
    """``render_volume`` for every camera of ``render_poses`` (``driver.generate_rays`` per frame): ``(rgbs uint8 [F, H, W, 3], disps float32
    [F, H, W])`` on the device, ``rgbs`` by the reference's truncating ``to8b`` (run_nerf_helpers.py:19).  ``latents``: one code per frame
    ``[F, latent_size]``, or one code for all frames; ``kwargs``: ``render_volume``'s (``occupancy=`` among them: one mask serves every frame)."""
    from .driver import generate_rays
    dev = volume["raw"].device
    H, W = int(intrinsics["height"]), int(intrinsics["width"])
    n_frames = len(render_poses)
    rgbs = torch.empty((n_frames, H, W, 3), dtype=torch.uint8, device=dev)
    disps = torch.empty((n_frames, H, W), dtype=torch.float32, device=dev)
    lat = None if latents is None else torch.as_tensor(latents).detach().to(device=dev, dtype=torch.float32)
    if lat is not None and lat.dim() == 1:
        lat = lat[None]
    if lat is not None and lat.shape[0] not in (1, n_frames):
        raise ValueError(f"latents must be one code or one per frame ({n_frames}), got {tuple(lat.shape)}")
    for i in range(n_frames):
        rays = generate_rays(render_poses[i], intrinsics, near, far, False, dev)
        code = None if lat is None else lat[i if lat.shape[0] > 1 else 0][None]
        out = render_volume(volume, rays, network=network, latents=code, **kwargs)
        rgbs[i] = (255 * out["rgb_map"].clamp(0, 1)).to(torch.uint8).view(H, W, 3)          # to8b: clip, scale, truncate
        disps[i] = out["disp_map"].view(H, W)
    return rgbs, disps


# --------------------------------------------------------------------------------------------
# baked warps (nrnerf_warped_volume_render): the ray bender of a time step as a coarse offset grid; a frame is one kernel
# --------------------------------------------------------------------------------------------
def bake_warp(render_kwargs_or_network, latent, min_point=None, max_point=None, resolution=32, *, fine=True, dtype=torch.float32,
              rows_per_launch=None, precision=None, checkpoint=None):
    """The ray bender of ONE time step (``latent``) on a regular grid: ``{"warp": [Gz, Gy, Gx, 4] = (unmasked offset x, y, z, rigidity mask),
    "min_point", "max_point"}`` -- what ``render_baked`` interpolates next to a canonical ``bake``.  ``bake``'s slab loop (``nrnerf_grid_points``
    -> ``nrnerf_query``) keeping the query's ``unmasked_offsets`` and ``rigidity_mask`` at the vertices; the result does not depend on
    ``rows_per_launch``.  ALL THREE test-time knobs are off in the bake whatever the modules carry (the modules are not touched):
    ``rigidity_test_time_cutoff``, ``test_time_scaling`` and the removal threshold are applied at render time.  The layout's mask of a bender
    without rigidity network is 1; this library packs no such bender.  ``render_kwargs_or_network``: the dictionary ``load_checkpoint`` /
    ``create_nerf`` returns (``fine`` picks ``network_fine`` when there is one) or a network module.  ``dtype``: ``torch.float32`` or
    ``torch.float16`` (the float32 bake rounded once).  ``resolution``: an int or ``(Gx, Gy, Gz)``, each 2 .. ``MAX_SAMPLES``.  The extent
    defaults to the checkpoint's volume extent.  No ray bender (the time-conditioned baseline included) raises ``Unsupported``."""
    if dtype not in _VOLUME_DTYPES:
        raise ValueError(f"a baked warp is float32 or float16, got {dtype}")
    if isinstance(render_kwargs_or_network, dict):
        kw = render_kwargs_or_network
        net = kw.get("network_fine") if fine and kw.get("network_fine") is not None else kw["network_fn"]
    else:
        net = render_kwargs_or_network
    if R._bender_of(net) is None:
        raise R.Unsupported("a warp is baked from a ray bender: this network has none")
    if min_point is None or max_point is None:
        from .visualize import volume_extent_of
        ext = volume_extent_of(checkpoint) if checkpoint is not None else None
        if ext is None:
            raise ValueError("bake_warp needs min_point / max_point (or a checkpoint that carries its volume extent)")
        min_point, max_point = ext
    gx, gy, gz = volume_grid_shape(resolution)
    lo, hi = grid_extent(min_point, max_point)
    if not (hi > lo).all():
        raise ValueError(f"a baked warp needs min < max on every axis, got {lo} .. {hi}")
    if latent is None:
        raise ValueError("a ray bender needs a latent code")
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        dev = latent.device if torch.is_tensor(latent) and latent.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    model = R.get_model(net, None, precision=precision, device=dev)
    if not model.has_bender:
        raise R.Unsupported("a warp is baked from a ray bender: this handle has none")
    dev = model.device
    lat = torch.as_tensor(latent).detach().to(device=dev, dtype=torch.float32).reshape(1, -1).contiguous()
    n_rows = gy * gz
    slabs = plan_slabs(n_rows, default_rows_per_launch(gx) if rows_per_launch is None else rows_per_launch)
    warp = torch.empty((gz, gy, gx, 4), dtype=dtype, device=dev)
    warp_rows = warp.view(n_rows, gx, 4)
    lib = _lib.load()
    fp = C.POINTER(C.c_float)
    rows_max = max(n for _, n in slabs)
    pts = torch.empty((rows_max, gx, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), torch.no_grad():
        for first, n in slabs:
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(lib.nrnerf_grid_points(lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), gx, gy, gz, first, n, pts.data_ptr(), stream),
                       "nrnerf_grid_points")
            try:
                _, det = model.query(pts[:n], lat.expand(n, -1), None, 0, detailed_output=True)        # (no knob is passed: all off)
            except _lib.NrnerfError as e:
                if e.status != _lib.ERR_UNSUPPORTED:
                    raise
                raise R.Unsupported(str(e)) from e
            warp_rows[first:first + n, :, :3].copy_(det["unmasked_offsets"])
            warp_rows[first:first + n, :, 3:].copy_(det["rigidity_mask"])
    return {"warp": warp, "min_point": lo, "max_point": hi}


def bake_warps(render_kwargs_or_network, latents, min_point=None, max_point=None, resolution=32, **kwargs):
    """``bake_warp`` for every code of ``latents [F, latent_size]``: ``{"warp": [F, Gz, Gy, Gx, 4], "min_point", "max_point"}``, one box for
    all frames -- with a canonical ``bake`` the whole sequence, a handful of tensors ``torch.save`` can write."""
    lat = torch.as_tensor(latents)
    if lat.dim() != 2 or lat.shape[0] < 1:
        raise ValueError(f"latents must be [F >= 1, latent_size], got {tuple(lat.shape)}")
    frames = [bake_warp(render_kwargs_or_network, lat[i], min_point, max_point, resolution, **kwargs) for i in range(lat.shape[0])]
    return {"warp": torch.stack([f["warp"] for f in frames], 0), "min_point": frames[0]["min_point"], "max_point": frames[0]["max_point"]}


def warped_volume_render(volume, warp, rays, *, N_samples, z_vals=None, lindisp=False, white_bkgd=False, rigidity_cutoff=None,
                         test_time_scaling=None, removal_threshold=None, composite=True, retraw=False, weights=False, alpha=False,
                         surface=False, return_points=False, occupancy=None):
    """``nrnerf_warped_volume_render`` on tensors: the ``N_samples`` samples ``o + d z`` of every ray bent by ``warp`` (the knobs applied here),
    the canonical ``volume``'s logits at the bent points, and their compositing -- one kernel.  ``rays [N, >= 8]``; ``z_vals [N, S]`` or the
    coarse spacing between the rays' near and far.  Returns ``rgb_map / disp_map / acc_map`` (+ ``raw``, ``weights``, ``alpha``,
    ``surface_pts``, ``surface_rigidity``, ``median_index``, ``points4 [N, S, 4]`` = (bent xyz, rigidity after the cutoff) as asked for);
    ``composite=False`` runs the lookup alone and returns ``raw`` and / or ``points4``.  The value rule: include/nrnerf.h.
    ``occupancy``: the volume's mask (``build_occupancy``) -- the same call through ``culled_volume_render``, which requests nothing for a
    sample in an empty block; ``None`` is this call."""
    if occupancy is not None:
        return culled_volume_render(volume, rays, occupancy=occupancy, use_sh=False, warp=warp, N_samples=N_samples, z_vals=z_vals,
                                    lindisp=lindisp, white_bkgd=white_bkgd, rigidity_cutoff=rigidity_cutoff,
                                    test_time_scaling=test_time_scaling, removal_threshold=removal_threshold, composite=composite,
                                    retraw=retraw, weights=weights, alpha=alpha, surface=surface, return_points=return_points)
    vol, lo, hi, g = _grid_parts(volume, "raw", "volume")
    grid, wlo, whi, wg = _grid_parts(warp, "warp", "warp")
    dev = vol.device
    if grid.device != dev:
        raise ValueError(f"the volume is on {dev}, the warp on {grid.device}")
    a = _lib.WarpedVolumeRenderArgs()
    N, S, keep = _render_front(a, dev, rays, N_samples, z_vals, lindisp, white_bkgd)
    a.volume, a.volume_dtype = vol.data_ptr(), _VOLUME_DTYPES[vol.dtype]
    a.g[:] = g
    a.min_point[:], a.max_point[:] = lo.tolist(), hi.tolist()
    a.warp, a.warp_dtype = grid.data_ptr(), _VOLUME_DTYPES[grid.dtype]
    a.warp_g[:] = wg
    a.warp_min_point[:], a.warp_max_point[:] = wlo.tolist(), whi.tolist()
    if rigidity_cutoff is not None:
        a.has_rigidity_cutoff, a.rigidity_cutoff = 1, float(rigidity_cutoff)
    if test_time_scaling is not None:
        a.has_test_time_scaling, a.test_time_scaling = 1, float(test_time_scaling)
    if removal_threshold is not None:
        a.has_removal_threshold, a.removal_threshold = 1, float(removal_threshold)
    out, new = _render_outputs(a, dev, N, S, composite, weights, alpha, surface)
    if retraw or (not composite and not return_points):
        a.raw = new("raw", N, S, 4)
    if return_points:
        a.points4 = new("points4", N, S, 4)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nrnerf_warped_volume_render(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "nrnerf_warped_volume_render")
    return out


def _has_sh(volume) -> bool:
    """Whether a volume record carries spherical-harmonic coefficients (a view-dependent bake of degree >= 1)."""
    return isinstance(volume, dict) and volume.get("sh") is not None


def _sh_parts(volume, vol):
    """``volume["sh"]`` checked against the record's ``"raw"`` (``vol``, as ``_grid_parts`` returned it): ``(sh contiguous, degree)``."""
    sh = volume["sh"]
    if not torch.is_tensor(sh) or sh.device != vol.device:
        raise R.Unsupported("the sh array is not on the volume's device")
    degree = volume.get("sh_degree", int(sh.shape[-1]) // 12 if sh.dim() == 4 else None)
    if degree not in (1, 2):
        raise ValueError(f"an sh array has sh_degree 1 or 2, got {degree!r}")
    want = tuple(vol.shape[:3]) + (sh_channels(int(degree)),)
    if tuple(sh.shape) != want or sh.dtype != vol.dtype:
        raise ValueError(f"the sh array of this volume is {vol.dtype} {want}, got {sh.dtype} {tuple(sh.shape)}")
    return sh.detach().contiguous(), int(degree)


def sh_volume_render(volume, rays, *, N_samples, warp=None, points4=None, z_vals=None, lindisp=False, white_bkgd=False, rigidity_cutoff=None,
                     test_time_scaling=None, removal_threshold=None, composite=True, retraw=False, weights=False, alpha=False,
                     surface=False, return_points=False, ray_directions=None, occupancy=None):
    """``nrnerf_sh_volume_render`` on tensors: ``warped_volume_render`` for a volume record with ``"sh"`` (``bake(sh_degree=1 or 2)``) -- per
    sample the colour logits are ``raw`` plus the spherical harmonics at the sample's direction times the coefficients at the bent point.
    The bent points are ``warp``'s (a ``bake_warp`` record; the knobs applied here), the ready-made ``points4 [N, S, 4]`` (not with a warp),
    or the straight samples.  ``ray_directions``: ``True`` takes every sample's direction from its ray, ``False`` from the difference of
    consecutive bent points (needs 2 samples or more); ``None`` picks differences whenever a warp or ``points4`` is given, as the reference
    does for a head behind a bender.  Outputs and the other arguments: ``warped_volume_render``'s.  The value rule: include/nrnerf.h."""
    if occupancy is not None:
        return culled_volume_render(volume, rays, occupancy=occupancy, use_sh=True, warp=warp, points4=points4, N_samples=N_samples,
                                    z_vals=z_vals, lindisp=lindisp, white_bkgd=white_bkgd, rigidity_cutoff=rigidity_cutoff,
                                    test_time_scaling=test_time_scaling, removal_threshold=removal_threshold, composite=composite,
                                    retraw=retraw, weights=weights, alpha=alpha, surface=surface, return_points=return_points,
                                    ray_directions=ray_directions)
    vol, lo, hi, g = _grid_parts(volume, "raw", "volume")
    sh, degree = _sh_parts(volume, vol)
    dev = vol.device
    if warp is not None and points4 is not None:
        raise ValueError("a warp bends the samples itself: points4 cannot be given with it")
    a = _lib.ShVolumeRenderArgs()
    N, S, keep = _render_front(a, dev, rays, N_samples, z_vals, lindisp, white_bkgd)
    a.volume, a.volume_dtype = vol.data_ptr(), _VOLUME_DTYPES[vol.dtype]
    a.g[:] = g
    a.min_point[:], a.max_point[:] = lo.tolist(), hi.tolist()
    a.sh, a.sh_degree = sh.data_ptr(), degree
    if warp is not None:
        grid, wlo, whi, wg = _grid_parts(warp, "warp", "warp")
        if grid.device != dev:
            raise ValueError(f"the volume is on {dev}, the warp on {grid.device}")
        a.warp, a.warp_dtype = grid.data_ptr(), _VOLUME_DTYPES[grid.dtype]
        a.warp_g[:] = wg
        a.warp_min_point[:], a.warp_max_point[:] = wlo.tolist(), whi.tolist()
    elif rigidity_cutoff is not None or test_time_scaling is not None:
        raise ValueError("the rigidity cutoff and the scaling act on a warp")
    if points4 is not None:
        if tuple(points4.shape) != (N, S, 4):
            raise ValueError(f"points4 must be {(N, S, 4)}, got {tuple(points4.shape)}")
        points4 = points4.detach().to(dtype=torch.float32, device=dev).contiguous()
        a.points4_in = points4.data_ptr() or None
    if ray_directions is None:
        ray_directions = warp is None and points4 is None
    if not ray_directions and S < 2:
        raise ValueError("a direction from the difference of bent points needs 2 samples or more")
    a.direction_mode = _lib.SH_DIRECTION_RAY if ray_directions else _lib.SH_DIRECTION_DIFFERENCES
    if rigidity_cutoff is not None:
        a.has_rigidity_cutoff, a.rigidity_cutoff = 1, float(rigidity_cutoff)
    if test_time_scaling is not None:
        a.has_test_time_scaling, a.test_time_scaling = 1, float(test_time_scaling)
    if removal_threshold is not None:
        a.has_removal_threshold, a.removal_threshold = 1, float(removal_threshold)
    out, new = _render_outputs(a, dev, N, S, composite, weights, alpha, surface)
    if retraw or (not composite and not return_points):
        a.raw = new("raw", N, S, 4)
    if return_points:
        a.points4 = new("points4", N, S, 4)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nrnerf_sh_volume_render(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "nrnerf_sh_volume_render")
    return out


# --------------------------------------------------------------------------------------------
# occupancy masks (nrnerf_occupancy_build / nrnerf_culled_volume_render): a baked render that skips empty space
# --------------------------------------------------------------------------------------------
def build_occupancy(volume, *, block=8, threshold=0.0):
    """The occupancy mask of a baked volume: ``{"bits": int32 [words], "block", "grid": (Gz, Gy, Gx), "threshold"}`` -- one bit per block of
    ``block`` (2, 4, 8 or 16) cells per axis, set iff some corner of some cell of the block has a sigma logit that is not ``<= threshold`` or
    a ``raw`` channel that is not finite (the rule: include/nrnerf.h, "occupancy masks").  ``volume``: a ``bake`` record, with or without
    ``"sh"``, or a bare grid ``[Gz, Gy, Gx, 4]`` on the device; an ``"sh"`` array must be finite (``ValueError``).
    ``threshold=0`` is exact: every map ``render_baked(..., occupancy=mask)`` returns keeps the bits of the unmasked render.  ``threshold >
    0`` also drops blocks of thin density: lossy.  A negative threshold is a ``ValueError``.
    A mask is a SNAPSHOT: after ``refine_bake`` (or anything else) changes the volume, build it again -- a stale mask is not detected."""
    block = int(block)
    if block not in (2, 4, 8, 16):
        raise ValueError(f"an occupancy block is 2, 4, 8 or 16 cells per axis, got {block}")
    threshold = float(threshold)
    if not threshold >= 0.0:
        raise ValueError(f"an occupancy threshold is >= 0 (0: exact), got {threshold}")
    record = volume if isinstance(volume, dict) else {"raw": volume, "min_point": (0.0, 0.0, 0.0), "max_point": (1.0, 1.0, 1.0)}
    vol, _, _, g = _grid_parts(record, "raw", "volume")
    if _has_sh(record):
        sh, _ = _sh_parts(record, vol)
        if not bool(torch.isfinite(sh).all()):
            raise ValueError("the sh array holds a value that is not finite: no mask can vouch for a render of it")
    k = block.bit_length() - 1
    dev = vol.device
    bits = torch.empty((_lib.occupancy_words(g, k),), dtype=torch.int32, device=dev)
    a = _lib.OccupancyBuildArgs()
    a.struct_size = C.sizeof(a)
    a.volume, a.volume_dtype = vol.data_ptr(), _VOLUME_DTYPES[vol.dtype]
    a.g[:] = g
    a.log2_block, a.threshold = k, threshold
    a.words, a.n_words = bits.data_ptr(), int(bits.numel())
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nrnerf_occupancy_build(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "nrnerf_occupancy_build")
    return {"bits": bits, "block": block, "grid": (g[2], g[1], g[0]), "threshold": threshold}


def _occupancy_parts(occupancy, vol, g):
    """A ``build_occupancy`` record checked against the volume it is used with: ``(bits contiguous, log2 of the block)``."""
    block = int(occupancy["block"])
    if block not in (2, 4, 8, 16):
        raise ValueError(f"an occupancy block is 2, 4, 8 or 16 cells per axis, got {block}")
    if tuple(int(v) for v in occupancy["grid"]) != (g[2], g[1], g[0]):
        raise ValueError(f"the occupancy mask was built for a grid {tuple(occupancy['grid'])}, the volume is {(g[2], g[1], g[0])}")
    bits = occupancy["bits"]
    k = block.bit_length() - 1
    if not torch.is_tensor(bits) or bits.device != vol.device:
        raise R.Unsupported("the occupancy mask is not on the volume's device")
    if bits.dtype != torch.int32 or bits.dim() != 1 or int(bits.numel()) != _lib.occupancy_words(g, k):
        raise ValueError(f"the occupancy mask of this volume is int32 [{_lib.occupancy_words(g, k)}], got {bits.dtype} {tuple(bits.shape)}")
    return bits.contiguous(), k


def culled_volume_render(volume, rays, *, occupancy, N_samples, use_sh=None, warp=None, points4=None, z_vals=None, lindisp=False,
                         white_bkgd=False, rigidity_cutoff=None, test_time_scaling=None, removal_threshold=None, composite=True, retraw=False,
                         weights=False, alpha=False, surface=False, return_points=False, ray_directions=None):
    """``nrnerf_culled_volume_render`` on tensors: ``sh_volume_render`` -- or, for a record without ``"sh"`` (and with ``use_sh=False``),
    ``warped_volume_render`` / ``volume_render`` -- with the volume's ``occupancy`` mask (``build_occupancy``): a sample whose bent point falls
    in an empty block is an empty sample and requests nothing.  The bent points are ``warp``'s, the ready-made ``points4``, or the straight
    samples.  Arguments and outputs: ``sh_volume_render``'s.  The mask must have been built from this volume as it is now (a snapshot: rebuild
    it after ``refine_bake``); only its grid shape is checked (``ValueError``)."""
    vol, lo, hi, g = _grid_parts(volume, "raw", "volume")
    if use_sh is None:
        use_sh = _has_sh(volume)
    sh, degree = _sh_parts(volume, vol) if use_sh else (None, 0)
    bits, k = _occupancy_parts(occupancy, vol, g)
    dev = vol.device
    if warp is not None and points4 is not None:
        raise ValueError("a warp bends the samples itself: points4 cannot be given with it")
    a = _lib.CulledVolumeRenderArgs()
    N, S, keep = _render_front(a, dev, rays, N_samples, z_vals, lindisp, white_bkgd)
    a.volume, a.volume_dtype = vol.data_ptr(), _VOLUME_DTYPES[vol.dtype]
    a.g[:] = g
    a.min_point[:], a.max_point[:] = lo.tolist(), hi.tolist()
    if sh is not None:
        a.sh = sh.data_ptr()
    a.sh_degree = degree
    a.occupancy, a.occupancy_log2_block, a.occupancy_words = bits.data_ptr(), k, int(bits.numel())
    if warp is not None:
        grid, wlo, whi, wg = _grid_parts(warp, "warp", "warp")
        if grid.device != dev:
            raise ValueError(f"the volume is on {dev}, the warp on {grid.device}")
        a.warp, a.warp_dtype = grid.data_ptr(), _VOLUME_DTYPES[grid.dtype]
        a.warp_g[:] = wg
        a.warp_min_point[:], a.warp_max_point[:] = wlo.tolist(), whi.tolist()
    elif rigidity_cutoff is not None or test_time_scaling is not None:
        raise ValueError("the rigidity cutoff and the scaling act on a warp")
    if points4 is not None:
        if tuple(points4.shape) != (N, S, 4):
            raise ValueError(f"points4 must be {(N, S, 4)}, got {tuple(points4.shape)}")
        points4 = points4.detach().to(dtype=torch.float32, device=dev).contiguous()
        a.points4_in = points4.data_ptr() or None
    if ray_directions is None:
        ray_directions = warp is None and points4 is None
    if degree and not ray_directions and S < 2:
        raise ValueError("a direction from the difference of bent points needs 2 samples or more")
    a.direction_mode = _lib.SH_DIRECTION_RAY if ray_directions else _lib.SH_DIRECTION_DIFFERENCES
    if rigidity_cutoff is not None:
        a.has_rigidity_cutoff, a.rigidity_cutoff = 1, float(rigidity_cutoff)
    if test_time_scaling is not None:
        a.has_test_time_scaling, a.test_time_scaling = 1, float(test_time_scaling)
    if removal_threshold is not None:
        a.has_removal_threshold, a.removal_threshold = 1, float(removal_threshold)
    out, new = _render_outputs(a, dev, N, S, composite, weights, alpha, surface)
    if retraw or (not composite and not return_points):
        a.raw = new("raw", N, S, 4)
    if return_points:
        a.points4 = new("points4", N, S, 4)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nrnerf_culled_volume_render(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "nrnerf_culled_volume_render")
    return out


# --------------------------------------------------------------------------------------------
# hierarchical sampling of a baked scene (nrnerf_hierarchical_volume_render): the coarse pass, sample_pdf and the fine
# pass in one kernel, or composed of the calls above for the records and sizes that have no fused kernel
# --------------------------------------------------------------------------------------------
def hierarchical_fused_shape(N_samples, N_importance) -> bool:
    """Whether the fused kernel takes ``N_samples`` + ``N_importance`` (csrc/nrnerf_hier_volume.h: 3 .. 256 coarse, at most 512 merged)."""
    S, I = int(N_samples), int(N_importance)
    return 3 <= S <= _lib.HIER_MAX_COARSE and I >= 1 and S + I <= _lib.HIER_MAX_MERGED


def _importance_u(importance_u, N, I, dev):
    if importance_u is None:
        return None
    if tuple(importance_u.shape) != (N, I):
        raise ValueError(f"importance_u must be {(N, I)}, got {tuple(importance_u.shape)}")
    return importance_u.detach().to(device=dev, dtype=torch.float32).contiguous()


def hierarchical_volume_render(volume, warp, rays, *, N_samples, N_importance, z_vals=None, importance_u=None, lindisp=False, white_bkgd=False,
                               rigidity_cutoff=None, test_time_scaling=None, removal_threshold=None, coarse=True, retraw=False, weights=False,
                               alpha=False, surface=False, return_points=False):
    """``nrnerf_hierarchical_volume_render`` on tensors: ``N_samples`` coarse samples (``z_vals [N, S]`` or the coarse spacing), ``N_importance``
    more drawn from the coarse weights (``importance_u [N, I]`` or ``linspace(0, 1, I)``), and the fine pass at the merged depths -- one
    kernel, the bits of ``warped_volume_render`` -> ``nrnerf_composite_forward`` -> ``warped_volume_render``.  ``warp``: a ``bake_warp`` record,
    or ``None`` for straight rays.  Returns the fine pass' ``rgb_map / disp_map / acc_map``, ``z_std [N]``, ``z_vals [N, S + I]``, the coarse
    pass' ``rgb0 / disp0 / acc0`` (unless ``coarse=False``) and, as asked for, the fine pass' ``raw``, ``weights``, ``alpha``, ``surface_pts``,
    ``surface_rigidity``, ``median_index``, ``points4``.  Shapes beyond ``hierarchical_fused_shape`` raise ``NrnerfError`` (UNSUPPORTED):
    ``render_baked`` composes those.  The value rule: include/nrnerf.h."""
    vol, lo, hi, g = _grid_parts(volume, "raw", "volume")
    dev = vol.device
    a = _lib.HierarchicalVolumeRenderArgs()
    N, S, keep = _render_front(a, dev, rays, N_samples, z_vals, lindisp, white_bkgd)
    I = int(N_importance)
    if I < 1 or S < 3:
        raise ValueError(f"hierarchical sampling needs N_samples >= 3 and N_importance >= 1, got {S} + {I}")
    a.n_importance = I
    u = _importance_u(importance_u, N, I, dev)
    if u is not None:
        a.u = u.data_ptr() or None
    a.volume, a.volume_dtype = vol.data_ptr(), _VOLUME_DTYPES[vol.dtype]
    a.g[:] = g
    a.min_point[:], a.max_point[:] = lo.tolist(), hi.tolist()
    if warp is not None:
        grid, wlo, whi, wg = _grid_parts(warp, "warp", "warp")
        if grid.device != dev:
            raise ValueError(f"the volume is on {dev}, the warp on {grid.device}")
        a.warp, a.warp_dtype = grid.data_ptr(), _VOLUME_DTYPES[grid.dtype]
        a.warp_g[:] = wg
        a.warp_min_point[:], a.warp_max_point[:] = wlo.tolist(), whi.tolist()
    if rigidity_cutoff is not None:
        a.has_rigidity_cutoff, a.rigidity_cutoff = 1, float(rigidity_cutoff)
    if test_time_scaling is not None:
        a.has_test_time_scaling, a.test_time_scaling = 1, float(test_time_scaling)
    if removal_threshold is not None:
        a.has_removal_threshold, a.removal_threshold = 1, float(removal_threshold)
    out, new = _render_outputs(a, dev, N, S + I, True, weights, alpha, surface)
    if coarse:
        a.rgb0, a.disp0, a.acc0 = new("rgb0", N, 3), new("disp0", N), new("acc0", N)
    a.z_std, a.z_vals = new("z_std", N), new("z_vals", N, S + I)
    if retraw:
        a.raw = new("raw", N, S + I, 4)
    if return_points:
        a.points4 = new("points4", N, S + I, 4)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nrnerf_hierarchical_volume_render(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "nrnerf_hierarchical_volume_render")
    return out


def importance_depths(raw, rays, *, N_importance, z_vals=None, importance_u=None, lindisp=False, white_bkgd=False):
    """``nrnerf_composite_forward`` with ``n_importance > 0`` on the logits ``raw [N, S, 4]`` of a coarse pass, without autograd: ``(z_merged
    [N, S + I], z_std [N])`` -- the coarse depths (``z_vals`` or the coarse spacing) merged with ``N_importance`` depths drawn from the pass'
    weights (sample_pdf, run_nerf_helpers.py:651-698; the merge, train.py:910-920)."""
    dev = raw.device
    f32 = dict(dtype=torch.float32, device=dev)
    raw = raw.detach().to(**f32).contiguous()
    rays = rays.detach().to(**f32).contiguous()
    N, S, I = int(raw.shape[0]), int(raw.shape[1]), int(N_importance)
    if I < 1 or S < 3 or S + I > _lib.MAX_SAMPLES:
        raise ValueError(f"hierarchical sampling needs N_samples >= 3, N_importance >= 1 and at most {_lib.MAX_SAMPLES} samples in all, got {S} + {I}")
    a = _lib.CompositeArgs()
    a.struct_size = C.sizeof(_lib.CompositeArgs)
    a.n_rays, a.n_samples, a.n_importance = N, S, I
    a.rays, a.ray_stride, a.raw4 = rays.data_ptr() or None, int(rays.shape[1]), raw.data_ptr() or None
    a.lindisp, a.white_bkgd = int(bool(lindisp)), int(bool(white_bkgd))
    if z_vals is not None:
        if tuple(z_vals.shape) != (N, S):
            raise ValueError(f"z_vals must be {(N, S)}, got {tuple(z_vals.shape)}")
        z_vals = z_vals.detach().to(**f32).contiguous()
        a.z = z_vals.data_ptr() or None
    u = _importance_u(importance_u, N, I, dev)
    if u is not None:
        a.u = u.data_ptr() or None
    maps = torch.empty((N, 5), **f32)            # the pass' rgb, disp, acc: the call requires them, the coarse render has returned them already
    z_merged, z_std = torch.empty((N, S + I), **f32), torch.empty((N,), **f32)
    a.rgb, a.disp, a.acc = maps.data_ptr() or None, (maps.data_ptr() + 12 * N) or None, (maps.data_ptr() + 16 * N) or None
    a.z_std, a.z_merged = z_std.data_ptr() or None, z_merged.data_ptr() or None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nrnerf_composite_forward(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                   "nrnerf_composite_forward")
    return z_merged, z_std


def _render_hierarchical_composed(render, rays, S, I, z, importance_u, lindisp, white_bkgd, **fine):
    """The composed route of a hierarchical render, over ANY ``render(N_samples=, z_vals=, retraw=, **outputs)`` of this module that returns
    ``raw`` under ``retraw``: the render at ``S``, ``importance_depths`` on its logits, the render at ``S + I`` at the merged depths."""
    if I < 1 or S < 3 or S + I > _lib.MAX_SAMPLES:
        raise ValueError(f"hierarchical sampling needs N_samples >= 3, N_importance >= 1 and at most {_lib.MAX_SAMPLES} samples in all, got {S} + {I}")
    first = render(N_samples=S, z_vals=z, retraw=True)
    z_merged, z_std = importance_depths(first["raw"], rays, N_importance=I, z_vals=z, importance_u=importance_u, lindisp=lindisp,
                                        white_bkgd=white_bkgd)
    out = render(N_samples=S + I, z_vals=z_merged, **fine)
    out.update(rgb0=first["rgb_map"], disp0=first["disp_map"], acc0=first["acc_map"], z_std=z_std, z_vals=z_merged)
    return out


HIER_FUSED_DEFAULT_MERGED = 128     # fused=None takes the fused kernel up to this many merged samples: where it measured faster


def _use_fused(fused, S, I, plain):
    """``fused=True`` insists on the fused kernel (``Unsupported`` where there is none: an ``"sh"`` record, a mask, a shape it does not take);
    ``None`` takes it where it is the faster route -- up to 128 merged samples, two per lane: beyond that its coarse pass runs at the fine
    pass' occupancy and the composed route wins (64 + 128: by 4 %; 64 + 192 and up: 1.4 - 1.8 x) -- and composes otherwise."""
    can = plain and hierarchical_fused_shape(S, I)
    if fused and not can:
        raise R.Unsupported(f"no fused hierarchical kernel for this render ({S} + {I} samples, {'plain' if plain else 'sh / occupancy'} record)")
    return (can and S + I <= HIER_FUSED_DEFAULT_MERGED) if fused is None else bool(fused)


def render_baked(volume, warp, rays, *, N_samples=192, z_vals=None, lindisp=False, white_bkgd=False, rigidity_cutoff=None,
                 test_time_scaling=None, removal_threshold=None, surface=False, retraw=False, return_points=False, occupancy=None,
                 N_importance=0, importance_u=None, fused=None):
    """A baked scene rendered along ``rays [N, >= 8]`` with no network, no model handle and no latent code: ``volume`` is the canonical ``bake``,
    ``warp`` the ``bake_warp`` of the time step.  ``rgb_map / disp_map / acc_map`` (+ ``raw`` under ``retraw``; ``surface_pts``,
    ``surface_rigidity``, ``median_index`` under ``surface``; ``points4`` under ``return_points``).  The samples are ``N_samples`` of the coarse
    spacing (``lindisp`` honoured) or ``z_vals [N, S]``.  ``rigidity_cutoff`` (background stabilisation), ``test_time_scaling`` (motion
    exaggeration) and ``removal_threshold`` are the bender's test-time knobs, applied per sample at render time; ``None`` is off.  Refuses
    autograd inputs (``Unsupported``): a preview has no gradient.  A volume record with ``"sh"`` (a view-dependent bake) goes through
    ``sh_volume_render``: the colour of a sample is evaluated at the difference of the ray's consecutive bent points.
    ``occupancy``: the volume's mask (``build_occupancy(volume)``): samples whose bent point falls in an empty block request nothing.  At the
    mask's ``threshold=0`` every map keeps its bits; ``raw`` is zero at the skipped samples.  ``None`` takes the unmasked kernels.
    ``N_importance > 0``: hierarchical sampling, as the network path does it -- the ``N_samples`` are the coarse pass, ``N_importance`` more are
    drawn from its weights (``importance_u [N, I]``, or ``linspace(0, 1, I)``) and the maps are the fine pass' over the merged depths; also
    returned: ``rgb0 / disp0 / acc0`` (the coarse maps), ``z_std [N]`` and ``z_vals [N, S + I]``; ``raw`` and ``points4`` are the fine pass'.
    ``fused=True`` takes the one-kernel route (``hierarchical_volume_render``), which exists for a record without ``"sh"``, no mask,
    ``N_samples <= 256`` and ``N_samples + N_importance <= 512`` (``Unsupported`` otherwise); ``False`` composes the calls above (up to 1024
    samples in all); ``None`` takes the faster of the two: the kernel up to 128 samples in all, the composition beyond.  Both routes return
    the same bits."""
    if not torch.is_tensor(rays) or rays.device.type != "cuda":
        raise R.Unsupported("rays are not on a ROCm device")
    if torch.is_grad_enabled() and (rays.requires_grad or volume["raw"].requires_grad or warp["warp"].requires_grad
                                    or (z_vals is not None and z_vals.requires_grad)
                                    or (importance_u is not None and importance_u.requires_grad)):
        raise R.Unsupported("autograd is enabled (rendering a baked scene has no gradient: render_baked_train has)")
    S = int(z_vals.shape[1] if z_vals is not None else N_samples)
    with torch.no_grad():
        z = None if z_vals is None else z_vals.detach().to(device=rays.device, dtype=torch.float32).contiguous()
        if int(N_importance) > 0:
            I = int(N_importance)
            knobs = dict(lindisp=lindisp, white_bkgd=white_bkgd, rigidity_cutoff=rigidity_cutoff, test_time_scaling=test_time_scaling,
                         removal_threshold=removal_threshold)
            if _use_fused(fused, S, I, not _has_sh(volume) and occupancy is None):
                return hierarchical_volume_render(volume, warp, rays, N_samples=S, N_importance=I, z_vals=z, importance_u=importance_u,
                                                  retraw=retraw, surface=surface, return_points=return_points, **knobs)
            one = sh_volume_render if _has_sh(volume) else warped_volume_render

            def render(**kw):
                return one(volume, rays, warp=warp, occupancy=occupancy, **knobs, **kw) if one is sh_volume_render else \
                    one(volume, warp, rays, occupancy=occupancy, **knobs, **kw)
            return _render_hierarchical_composed(render, rays, S, I, z, importance_u, lindisp, white_bkgd, retraw=retraw, surface=surface,
                                                 return_points=return_points)
        if _has_sh(volume):         # a view-dependent bake: the same kernel with a colour per direction (differences of the bent points)
            return sh_volume_render(volume, rays, warp=warp, N_samples=S, z_vals=z, lindisp=lindisp, white_bkgd=white_bkgd,
                                    rigidity_cutoff=rigidity_cutoff, test_time_scaling=test_time_scaling, removal_threshold=removal_threshold,
                                    retraw=retraw, surface=surface, return_points=return_points, occupancy=occupancy)
        return warped_volume_render(volume, warp, rays, N_samples=S, z_vals=z, lindisp=lindisp, white_bkgd=white_bkgd,
                                    rigidity_cutoff=rigidity_cutoff, test_time_scaling=test_time_scaling, removal_threshold=removal_threshold,
                                    retraw=retraw, surface=surface, return_points=return_points, occupancy=occupancy)


def render_baked_frames(volume, warps, render_poses, intrinsics, near, far, **kwargs):
    """``render_baked`` for every camera of ``render_poses`` (``driver.generate_rays`` per frame): ``(rgbs uint8 [F, H, W, 3], disps float32
    [F, H, W])`` on the device, ``rgbs`` by the reference's truncating ``to8b`` (run_nerf_helpers.py:19).  ``warps``: what ``bake_warps``
    returns (``[F, Gz, Gy, Gx, 4]``, one grid per frame; ``[1, ...]`` or what ``bake_warp`` returns: one grid for all frames); ``kwargs``:
    ``render_baked``'s (``occupancy=`` among them: the mask is the canonical volume's, one serves every frame; ``N_importance=`` and
    ``importance_u=``: hierarchical sampling, the same uniforms for every frame)."""
    from .driver import generate_rays
    dev = volume["raw"].device
    H, W = int(intrinsics["height"]), int(intrinsics["width"])
    n_frames = len(render_poses)
    grids = warps["warp"]
    if not torch.is_tensor(grids) or grids.dim() not in (4, 5):
        raise ValueError("warps must hold one grid [Gz, Gy, Gx, 4] or a stack [F, Gz, Gy, Gx, 4]")
    if grids.dim() == 4:
        grids = grids[None]
    if grids.shape[0] not in (1, n_frames):
        raise ValueError(f"warps must hold one grid or one per frame ({n_frames}), got {int(grids.shape[0])}")
    rgbs = torch.empty((n_frames, H, W, 3), dtype=torch.uint8, device=dev)
    disps = torch.empty((n_frames, H, W), dtype=torch.float32, device=dev)
    for i in range(n_frames):
        rays = generate_rays(render_poses[i], intrinsics, near, far, False, dev)
        out = render_baked(volume, dict(warps, warp=grids[i if grids.shape[0] > 1 else 0]), rays, **kwargs)
        rgbs[i] = (255 * out["rgb_map"].clamp(0, 1)).to(torch.uint8).view(H, W, 3)          # to8b: clip, scale, truncate
        disps[i] = out["disp_map"].view(H, W)
    return rgbs, disps


# --------------------------------------------------------------------------------------------
# the baked scene under autograd (nrnerf_grid_lookup_backward): refine a baked volume and baked warps on images
# --------------------------------------------------------------------------------------------
def _grid_record_fields(a, lo, hi, g):
    a.g[:] = g
    a.min_point[:], a.max_point[:] = lo.tolist(), hi.tolist()


class _GridLookup(torch.autograd.Function):
    """``[M, 4]`` values of ``grid [Gz, Gy, Gx, 4]`` at ``points4 [M, 4]`` (xyz first).  Forward: the lookup kernel of ``nrnerf_volume_render``
    (no maps, the points as ``[M, 1, 4]`` rows); backward: ``nrnerf_grid_lookup_backward``."""

    @staticmethod
    def forward(ctx, grid, points4, lo, hi):
        g = tuple(int(v) for v in (grid.shape[2], grid.shape[1], grid.shape[0]))
        dev = grid.device
        grid, points4 = grid.detach(), points4.detach()
        M = int(points4.shape[0])
        out = torch.empty((M, 4), dtype=torch.float32, device=dev)
        if M:
            a = _lib.VolumeRenderArgs()
            a.struct_size = C.sizeof(a)
            a.n_rays, a.n_samples = M, 1
            a.rays, a.ray_stride = points4.data_ptr(), 8          # (device memory the lookup on points4 never reads: the entry point wants a pointer)
            a.points4 = points4.data_ptr()
            a.volume, a.volume_dtype = grid.data_ptr(), _VOLUME_DTYPES[grid.dtype]
            _grid_record_fields(a, lo, hi, g)
            a.raw = out.data_ptr()
            with torch.cuda.device(dev):
                _lib.check(_lib.load().nrnerf_volume_render(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "nrnerf_volume_render")
        ctx.save_for_backward(grid, points4)
        ctx.lo, ctx.hi, ctx.g = lo, hi, g
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_value):
        grid, points4 = ctx.saved_tensors
        want_grid, want_points = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_value is None or not (want_grid or want_points):
            return None, None, None, None
        dev = grid.device
        M = int(points4.shape[0])
        g_value = g_value.to(dtype=torch.float32).contiguous()
        d_grid = torch.zeros(grid.shape, dtype=torch.float32, device=dev) if want_grid else None
        d_points = torch.zeros((M, 4), dtype=torch.float32, device=dev) if want_points else None
        d_xyz = torch.empty((M, 3), dtype=torch.float32, device=dev) if want_points else None
        if M:
            a = _lib.GridLookupBackwardArgs()
            a.struct_size = C.sizeof(a)
            a.grid, a.grid_dtype = grid.data_ptr(), _VOLUME_DTYPES[grid.dtype]
            _grid_record_fields(a, ctx.lo, ctx.hi, ctx.g)
            a.n_points, a.points, a.point_stride, a.g_value = M, points4.data_ptr(), 4, g_value.data_ptr()
            if want_grid:
                a.d_grid = d_grid.data_ptr()
            if want_points:
                a.d_points = d_xyz.data_ptr()
            with torch.cuda.device(dev):
                _lib.check(_lib.load().nrnerf_grid_lookup_backward(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                           "nrnerf_grid_lookup_backward")
            if want_points:
                d_points[:, :3] = d_xyz
        return (d_grid.to(grid.dtype) if want_grid else None), d_points, None, None


def grid_lookup(grid, min_point, max_point, points):
    """The value of a vertex-centred grid ``[Gz, Gy, Gx, 4]`` (float32 or float16, on the device) at ``points [..., 3]`` (or ``[..., 4]``, xyz
    first): ``[..., 4]`` float32 by THE VALUE AT A POINT of include/nrnerf.h -- the bits of ``volume_render(composite=False)`` -- and
    differentiable with respect to ``grid`` and ``points`` (``nrnerf_grid_lookup_backward``).  A point outside the box, or NaN, has value 0 and
    no gradient; on a cell face the gradient is the one of the cell the lookup picks (the upper cell, the last one on the top face).  The
    gradient of ``grid`` is summed in float32 with atomic adds -- its last bits can differ between runs -- and cast to the grid's dtype once.
    A volume record with ``"sh"`` in place of ``grid`` raises ``Unsupported``: ``sh_lookup`` is the lookup of such a record under autograd."""
    if _has_sh(grid):
        raise R.Unsupported("a volume record with spherical-harmonic coefficients: its gradients are sh_lookup's, not grid_lookup's")
    if not torch.is_tensor(grid) or grid.device.type != "cuda":
        raise R.Unsupported("the grid is not on a ROCm device")
    _, lo, hi, _ = _grid_parts({"grid": grid, "min_point": min_point, "max_point": max_point}, "grid", "grid")
    if not torch.is_tensor(points) or points.dim() < 1 or points.shape[-1] not in (3, 4):
        raise ValueError(f"points must be [..., 3] or [..., 4], got {tuple(points.shape) if torch.is_tensor(points) else type(points)}")
    lead = tuple(points.shape[:-1])
    p = points.to(device=grid.device, dtype=torch.float32).reshape(-1, points.shape[-1])
    if p.shape[-1] == 3:
        p = torch.cat([p, torch.zeros_like(p[:, :1])], -1)
    if int(p.shape[0]) >= 1 << 31:
        raise ValueError("at most 2^31 - 1 points per call")
    return _GridLookup.apply(grid.contiguous(), p.contiguous(), lo, hi).reshape(lead + (4,))


def render_baked_train(volume, warp, rays, *, N_samples, z_vals=None, lindisp=False, white_bkgd=False, rigidity_cutoff=None,
                       test_time_scaling=None, removal_threshold=None):
    """``render_baked``'s value rule under autograd, with respect to ``volume["raw"]`` and / or ``warp["warp"]`` (whichever requires a gradient):
    ``{"rgb_map", "disp_map", "acc_map", "weights"}``, the forward bits of ``render_baked``.  Composed of tested parts: the depths
    (``sample_rays``, or ``z_vals [N, S]``), ``p = o + d z``, ``grid_lookup`` of the warp, the cutoff (a decision: no gradient passes through
    it), ``p + m u`` (times the scaling), ``grid_lookup`` of the volume, the removal factor, then the compositing kernels of the training step
    (``training._Composite``).  ``warp=None``: straight rays (the knobs have nothing to act on and must be ``None``).  Rays and depths carry no
    gradient."""
    from .training import _Composite
    if _has_sh(volume):
        raise R.Unsupported("a view-dependent bake has no gradient here: render_sh_train differentiates its coefficients")
    if not torch.is_tensor(rays) or rays.device.type != "cuda":
        raise R.Unsupported("rays are not on a ROCm device")
    _, lo, hi, _ = _grid_parts(volume, "raw", "volume")
    dev = volume["raw"].device
    if warp is not None:
        _, wlo, whi, _ = _grid_parts(warp, "warp", "warp")
        if warp["warp"].device != dev:
            raise ValueError(f"the volume is on {dev}, the warp on {warp['warp'].device}")
    elif rigidity_cutoff is not None or test_time_scaling is not None or removal_threshold is not None:
        raise ValueError("the bender's knobs need a warp")
    if rays.dim() != 2 or rays.shape[1] < 8:
        raise ValueError(f"rays must be [N, >= 8], got {tuple(rays.shape)}")
    f32 = dict(dtype=torch.float32, device=dev)
    rays = rays.detach().to(**f32).contiguous()
    N, S = int(rays.shape[0]), int(z_vals.shape[1] if z_vals is not None else N_samples)
    if not 1 <= S <= _lib.MAX_SAMPLES:
        raise ValueError(f"1 <= N_samples <= {_lib.MAX_SAMPLES}, got {S}")
    with torch.no_grad():
        pts = None
        if z_vals is not None:
            if tuple(z_vals.shape) != (N, S):
                raise ValueError(f"z_vals must be {(N, S)}, got {tuple(z_vals.shape)}")
            z = z_vals.detach().to(**f32).contiguous()
        elif S >= 2:
            z, pts = sample_rays(rays, S, lindisp)
        else:       # one sample: the near bound
            z = (1.0 / (1.0 / rays[:, 6:7])).contiguous() if lindisp else rays[:, 6:7].contiguous()
        if pts is None:
            pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]                # a product and a sum, each rounded, as the kernels'
    if warp is not None:
        um = grid_lookup(warp["warp"], wlo, whi, pts)
        u, m = um[..., :3], um[..., 3]
        if rigidity_cutoff is not None:
            m = torch.where(m.detach() <= torch.tensor(float(rigidity_cutoff), **f32), torch.zeros_like(m), m)      # rnh:563-564
        off = m[..., None] * u                                                                                        # rnh:567
        if test_time_scaling is not None:
            off = off * torch.tensor(float(test_time_scaling), **f32)                                                 # rnh:568-569
        bent = pts + off
    else:
        bent = pts
    raw = grid_lookup(volume["raw"], lo, hi, bent)
    if removal_threshold is not None:
        kill = m.detach() >= torch.tensor(float(removal_threshold), **f32)                                            # rnh:308-311
        raw = torch.cat([raw[..., :3], torch.where(kill, raw[..., 3] * 0.0, raw[..., 3])[..., None]], -1)
    rgb, disp, acc, weights = _Composite.apply(raw, rays, z, None, bool(white_bkgd), 0, None)[:4]
    return {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "weights": weights}


def refine_bake(volume, warps, frames, *, steps, lr, batch_rays=None, params=("volume",), optimizer="adam", seed=0, **render):
    """Refines a baked scene on images: ``steps`` iterations of Adam (``optimizer="sgd"``: plain gradient descent) at rate ``lr`` on the mean
    squared error of ``render_baked_train``'s ``rgb_map`` against target colours.  ``frames``: a sequence of ``(rays [R, >= 8], target rgb
    [R, 3], warp index)``; step ``k`` takes frame ``k mod len(frames)`` and of it ``batch_rays`` rays drawn without replacement by a generator
    seeded with ``seed`` (``None``: all of its rays, in order).  ``warps``: what ``bake_warps`` / ``bake_warp`` returns (``[F, Gz, Gy, Gx, 4]`` or
    one grid, which every index then means), or ``None`` for straight rays.  ``params``: ``"volume"`` and / or ``"warp"``, what is refined; the
    refined grids are kept in float32 during the loop and come back in their records' dtype.  ``render``: ``render_baked_train``'s keywords
    (``N_samples``, ``lindisp``, ``white_bkgd``, the knobs).  Returns ``(volume record, warps record or None, [loss per step])``; the inputs are
    not modified.  No scheduler, no checkpointing.  A volume record with ``"sh"`` (a view-dependent bake) raises ``Unsupported``:
    ``refine_sh_bake`` refines such a record."""
    if _has_sh(volume):
        raise R.Unsupported("a view-dependent bake cannot be refined by refine_bake (gradients of its coefficients: refine_sh_bake)")
    return _refine_loop(volume, warps, frames, steps, lr, batch_rays, tuple(params), ("volume", "warp"), optimizer, seed, render_baked_train,
                        render, "refine_bake")


def _refine_loop(volume, warps, frames, steps, lr, batch_rays, params, allowed, optimizer, seed, render_fn, render, who):
    """The loop ``refine_bake`` and ``refine_sh_bake`` share: float32 copies of the grids named by ``params`` as leaves, per step one frame (and
    of it one batch of rays), the mean squared error of ``render_fn``'s ``rgb_map``, one optimiser step.  ``(volume record, warps record or
    None, [loss per step])``."""
    if not params or any(k not in allowed for k in params):
        raise ValueError(f"params names {' and / or '.join(repr(k) for k in allowed)}, got {params}")
    if "warp" in params and warps is None:
        raise ValueError("there is no warp to refine")
    if optimizer not in ("adam", "sgd"):
        raise ValueError(f"optimizer is 'adam' or 'sgd', got {optimizer!r}")
    if len(frames) < 1:
        raise ValueError(f"{who} needs at least one frame")
    dev = volume["raw"].device
    vol = volume["raw"].detach().to(torch.float32).clone().requires_grad_("volume" in params)
    sh = None
    if "sh" in allowed:
        sh = volume["sh"].detach().to(torch.float32).clone().requires_grad_("sh" in params)
    grids = None
    if warps is not None:
        grids = warps["warp"]
        if not torch.is_tensor(grids) or grids.dim() not in (4, 5):
            raise ValueError("warps must hold one grid [Gz, Gy, Gx, 4] or a stack [F, Gz, Gy, Gx, 4]")
        grids = grids.detach().to(torch.float32).clone().requires_grad_("warp" in params)
    leaves = [t for t in (vol, sh, grids) if t is not None and t.requires_grad]
    opt = torch.optim.Adam(leaves, lr=lr) if optimizer == "adam" else torch.optim.SGD(leaves, lr=lr)
    gen = torch.Generator().manual_seed(int(seed))
    losses = []
    for k in range(int(steps)):
        rays, target, index = frames[k % len(frames)]
        rays, target = rays.to(device=dev, dtype=torch.float32), target.to(device=dev, dtype=torch.float32)
        if batch_rays is not None and int(batch_rays) < int(rays.shape[0]):
            pick = torch.randperm(int(rays.shape[0]), generator=gen)[:int(batch_rays)].to(dev)
            rays, target = rays[pick], target[pick]
        w = None
        if grids is not None:
            w = dict(warps, warp=grids if grids.dim() == 4 else grids[int(index) if grids.shape[0] > 1 else 0])
        out = render_fn(dict(volume, raw=vol) if sh is None else dict(volume, raw=vol, sh=sh), w, rays, **render)
        loss = ((out["rgb_map"] - target) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    history = torch.stack(losses).cpu().tolist() if losses else []
    new_volume = dict(volume, raw=vol.detach().to(volume["raw"].dtype))
    if sh is not None:
        new_volume["sh"] = sh.detach().to(volume["sh"].dtype)
    new_warps = None if warps is None else dict(warps, warp=grids.detach().to(warps["warp"].dtype))
    return new_volume, new_warps, history


# --------------------------------------------------------------------------------------------
# view-dependent bakes under autograd (nrnerf_sh_lookup_backward): refine the coefficients of an SH volume on images
# --------------------------------------------------------------------------------------------
class _ShLookup(torch.autograd.Function):
    """``[N, S, 4]`` logits of a view-dependent record at ``points4 [N, S, 4]`` (xyz first).  Forward: the lookup kernel of
    ``nrnerf_sh_volume_render`` (``points4_in``, no maps, ``raw`` out); backward: ``nrnerf_grid_lookup_backward`` on ``raw`` plus
    ``nrnerf_sh_lookup_backward`` on ``sh``, the two ``d_points`` added.  ``rays`` given: the RAY rule, None: DIFFERENCES."""

    @staticmethod
    def forward(ctx, raw, sh, points4, rays, lo, hi, degree):
        raw, sh, points4 = raw.detach(), sh.detach(), points4.detach()
        N, S = int(points4.shape[0]), int(points4.shape[1])
        dev = raw.device
        record = {"raw": raw, "sh": sh, "sh_degree": degree, "min_point": lo, "max_point": hi}
        front = rays if rays is not None else torch.zeros((N, 8), dtype=torch.float32, device=dev)       # (read in RAY mode only)
        if N:
            out = sh_volume_render(record, front, N_samples=S, points4=points4, composite=False, retraw=True, ray_directions=rays is not None)["raw"]
        else:
            out = torch.empty((0, S, 4), dtype=torch.float32, device=dev)
        ctx.save_for_backward(raw, sh, points4, front)
        ctx.lo, ctx.hi, ctx.degree, ctx.ray_dirs = lo, hi, degree, rays is not None
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_raw):
        raw, sh, points4, rays = ctx.saved_tensors
        want_raw, want_sh, want_points = ctx.needs_input_grad[:3]
        if g_raw is None or not (want_raw or want_sh or want_points):
            return (None,) * 7
        dev = raw.device
        N, S = int(points4.shape[0]), int(points4.shape[1])
        g = tuple(int(v) for v in (raw.shape[2], raw.shape[1], raw.shape[0]))
        g_raw = g_raw.to(dtype=torch.float32).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        d_raw = torch.zeros(raw.shape, **f32) if want_raw else None
        d_sh = torch.zeros(sh.shape, **f32) if want_sh else None
        d_points = torch.zeros((N, S, 4), **f32) if want_points else None
        if N:
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            xyz_raw = torch.empty((N, S, 3), **f32) if want_points else None
            xyz_sh = torch.empty((N, S, 3), **f32) if want_points else None
            d_dirs = torch.empty((N, S, 3), **f32) if want_points and not ctx.ray_dirs else None          # the workspace of the chain
            with torch.cuda.device(dev):
                if want_raw or want_points:
                    a = _lib.GridLookupBackwardArgs()
                    a.struct_size = C.sizeof(a)
                    a.grid, a.grid_dtype = raw.data_ptr(), _VOLUME_DTYPES[raw.dtype]
                    _grid_record_fields(a, ctx.lo, ctx.hi, g)
                    a.n_points, a.points, a.point_stride, a.g_value = N * S, points4.data_ptr(), 4, g_raw.data_ptr()
                    a.d_grid = d_raw.data_ptr() if want_raw else None
                    a.d_points = xyz_raw.data_ptr() if want_points else None
                    _lib.check(_lib.load().nrnerf_grid_lookup_backward(C.byref(a), stream), "nrnerf_grid_lookup_backward")
                if want_sh or want_points:
                    b = _lib.ShLookupBackwardArgs()
                    b.struct_size = C.sizeof(b)
                    b.n_rays, b.n_samples = N, S
                    b.rays, b.ray_stride = rays.data_ptr(), int(rays.shape[1])
                    b.points4 = points4.data_ptr()
                    b.direction_mode = _lib.SH_DIRECTION_RAY if ctx.ray_dirs else _lib.SH_DIRECTION_DIFFERENCES
                    b.sh, b.sh_dtype, b.sh_degree = sh.data_ptr(), _VOLUME_DTYPES[sh.dtype], ctx.degree
                    _grid_record_fields(b, ctx.lo, ctx.hi, g)
                    b.g_raw = g_raw.data_ptr()
                    b.d_sh = d_sh.data_ptr() if want_sh else None
                    b.d_points = xyz_sh.data_ptr() if want_points else None
                    b.d_dirs = d_dirs.data_ptr() if d_dirs is not None else None
                    _lib.check(_lib.load().nrnerf_sh_lookup_backward(C.byref(b), stream), "nrnerf_sh_lookup_backward")
            if want_points:
                d_points[..., :3] = xyz_raw + xyz_sh
        return ((d_raw.to(raw.dtype) if want_raw else None), (d_sh.to(sh.dtype) if want_sh else None), d_points, None, None, None, None)


def sh_lookup(volume_record, points, rays=None):
    """The logits of a view-dependent volume record (``bake(sh_degree=1 or 2)``: ``"raw"`` and ``"sh"``) at the bent points ``points [N, S, 3]`` (or
    ``[N, S, 4]``, xyz first) of ``N`` rays: ``[N, S, 4]`` float32 -- the colour logits after the spherical-harmonic sum, and sigma -- the bits of
    ``sh_volume_render(points4=..., composite=False, retraw=True)``, and differentiable with respect to ``volume_record["raw"]``,
    ``volume_record["sh"]`` and ``points`` (``nrnerf_grid_lookup_backward`` plus ``nrnerf_sh_lookup_backward``).  ``rays [N, >= 8]`` given: every
    sample's direction is its ray's (RAY; nothing flows from the direction into the points); ``None``: the difference of consecutive points
    (DIFFERENCES, ``S >= 2``; the chain back to the points is part of the gradient).  Rays carry no gradient.  The gradients of ``raw`` and
    ``sh`` are summed in float32 with atomic adds -- their last bits can differ between runs -- and cast to the record's dtype once."""
    if not _has_sh(volume_record):
        raise R.Unsupported("sh_lookup takes a volume record with spherical-harmonic coefficients (\"sh\"): grid_lookup serves a plain grid")
    vol, lo, hi, _ = _grid_parts(volume_record, "raw", "volume")
    _, degree = _sh_parts(volume_record, vol)
    dev = vol.device
    if not torch.is_tensor(points) or points.dim() != 3 or points.shape[-1] not in (3, 4):
        raise ValueError(f"points must be [N, S, 3] or [N, S, 4], got {tuple(points.shape) if torch.is_tensor(points) else type(points)}")
    N, S = int(points.shape[0]), int(points.shape[1])
    if not 1 <= S <= _lib.MAX_SAMPLES:
        raise ValueError(f"1 <= S <= {_lib.MAX_SAMPLES}, got {S}")
    if rays is None and S < 2:
        raise ValueError("a direction from the difference of bent points needs 2 samples or more")
    if rays is not None:
        if not torch.is_tensor(rays) or rays.dim() != 2 or rays.shape[0] != N or rays.shape[1] < 8:
            raise ValueError(f"rays must be [{N}, >= 8], got {tuple(rays.shape) if torch.is_tensor(rays) else type(rays)}")
        rays = rays.detach().to(device=dev, dtype=torch.float32).contiguous()
    p = points.to(device=dev, dtype=torch.float32)
    if p.shape[-1] == 3:
        p = torch.cat([p, torch.zeros_like(p[..., :1])], -1)
    return _ShLookup.apply(volume_record["raw"].contiguous(), volume_record["sh"].contiguous(), p.contiguous(), rays, lo, hi, degree)


def render_sh_train(volume, warp, rays, *, N_samples, z_vals=None, lindisp=False, white_bkgd=False, rigidity_cutoff=None,
                    test_time_scaling=None, removal_threshold=None):
    """``render_baked``'s value rule for a view-dependent record under autograd, with respect to ``volume["raw"]``, ``volume["sh"]`` and / or
    ``warp["warp"]`` (whichever requires a gradient): ``{"rgb_map", "disp_map", "acc_map", "weights"}``, the forward bits of ``render_baked``.
    ``render_baked_train``'s composition with ``sh_lookup`` in place of the volume's ``grid_lookup``: behind a warp a sample's direction is the
    difference of the ray's consecutive bent points (DIFFERENCES, 2 samples or more), without one (``warp=None``; the knobs must be ``None``)
    the ray's own direction (RAY) -- the rule ``sh_volume_render`` follows.  Rays and depths carry no gradient."""
    from .training import _Composite
    if not _has_sh(volume):
        raise R.Unsupported("render_sh_train takes a volume record with \"sh\": render_baked_train serves a plain bake")
    if not torch.is_tensor(rays) or rays.device.type != "cuda":
        raise R.Unsupported("rays are not on a ROCm device")
    _grid_parts(volume, "raw", "volume")
    dev = volume["raw"].device
    if warp is not None:
        _, wlo, whi, _ = _grid_parts(warp, "warp", "warp")
        if warp["warp"].device != dev:
            raise ValueError(f"the volume is on {dev}, the warp on {warp['warp'].device}")
    elif rigidity_cutoff is not None or test_time_scaling is not None or removal_threshold is not None:
        raise ValueError("the bender's knobs need a warp")
    if rays.dim() != 2 or rays.shape[1] < 8:
        raise ValueError(f"rays must be [N, >= 8], got {tuple(rays.shape)}")
    f32 = dict(dtype=torch.float32, device=dev)
    rays = rays.detach().to(**f32).contiguous()
    N, S = int(rays.shape[0]), int(z_vals.shape[1] if z_vals is not None else N_samples)
    if not 1 <= S <= _lib.MAX_SAMPLES:
        raise ValueError(f"1 <= N_samples <= {_lib.MAX_SAMPLES}, got {S}")
    if warp is not None and S < 2:
        raise ValueError("a direction from the difference of bent points needs 2 samples or more")
    with torch.no_grad():
        pts = None
        if z_vals is not None:
            if tuple(z_vals.shape) != (N, S):
                raise ValueError(f"z_vals must be {(N, S)}, got {tuple(z_vals.shape)}")
            z = z_vals.detach().to(**f32).contiguous()
        elif S >= 2:
            z, pts = sample_rays(rays, S, lindisp)
        else:       # one sample: the near bound
            z = (1.0 / (1.0 / rays[:, 6:7])).contiguous() if lindisp else rays[:, 6:7].contiguous()
        if pts is None:
            pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]                # a product and a sum, each rounded, as the kernels'
    if warp is not None:
        um = grid_lookup(warp["warp"], wlo, whi, pts)
        u, m = um[..., :3], um[..., 3]
        if rigidity_cutoff is not None:
            m = torch.where(m.detach() <= torch.tensor(float(rigidity_cutoff), **f32), torch.zeros_like(m), m)      # rnh:563-564
        off = m[..., None] * u                                                                                        # rnh:567
        if test_time_scaling is not None:
            off = off * torch.tensor(float(test_time_scaling), **f32)                                                 # rnh:568-569
        raw = sh_lookup(volume, pts + off)
    else:
        raw = sh_lookup(volume, pts, rays)
    if removal_threshold is not None:
        kill = m.detach() >= torch.tensor(float(removal_threshold), **f32)                                            # rnh:308-311
        raw = torch.cat([raw[..., :3], torch.where(kill, raw[..., 3] * 0.0, raw[..., 3])[..., None]], -1)
    rgb, disp, acc, weights = _Composite.apply(raw, rays, z, None, bool(white_bkgd), 0, None)[:4]
    return {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "weights": weights}


def refine_sh_bake(volume, warps, frames, *, steps, lr, batch_rays=None, params=("volume", "sh"), optimizer="adam", seed=0, **render):
    """``refine_bake`` for a view-dependent bake: ``steps`` iterations of Adam (``optimizer="sgd"``: plain gradient descent) at rate ``lr`` on the
    mean squared error of ``render_sh_train``'s ``rgb_map`` against target colours.  ``frames``, ``warps``, ``batch_rays``, ``seed`` and ``render``:
    ``refine_bake``'s.  ``params``: a subset of ``"volume"`` (the record's ``"raw"``), ``"sh"`` (its coefficients) and ``"warp"``; the refined
    grids are kept in float32 during the loop and come back in their records' dtype.  Returns ``(volume record, warps record or None, [loss
    per step])``; the inputs are not modified."""
    if not _has_sh(volume):
        raise R.Unsupported("refine_sh_bake takes a volume record with \"sh\": refine_bake serves a plain bake")
    _sh_parts(volume, _grid_parts(volume, "raw", "volume")[0])
    return _refine_loop(volume, warps, frames, steps, lr, batch_rays, tuple(params), ("volume", "sh", "warp"), optimizer, seed, render_sh_train,
                        render, "refine_sh_bake")
