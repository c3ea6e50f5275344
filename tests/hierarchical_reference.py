"""The float64 model of a hierarchical baked render on straight rays -- tests/volume_reference.py for the two passes, the oracle's sample_pdf
and torch.sort between them -- and the synthetic thin-shell scene of tests/test_hierarchical.py: a Gaussian density shell baked analytically."""
import torch

from oracle import nrnerf_oracle as O
from tests import volume_reference as V

SHELL_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
SHELL_GRID = 48
# width: the Gaussian's sigma, chosen on the CPU with the float64 model below (tests/test_hierarchical.py, case 6): a Gaussian resolved by the
# uniform samples is integrated almost exactly by them (the Riemann sum of a smooth bump on an even grid), one much thinner than the coarse
# spacing is missed by the coarse pass too.  Between the two -- the rays' span 10.5, so 64 even samples lie 4 widths apart, 32 coarse ones 8 --
# the coarse pass sees the shell's tails and the fine pass resolves it.  Optical depth of one crossing: density * width * sqrt(2 pi) = 4
SHELL_RADIUS, SHELL_WIDTH, SHELL_DENSITY = 0.6, 0.04, 40.0
SHELL_NEAR, SHELL_FAR = 1.5, 12.0


def shell_volume(grid=SHELL_GRID, radius=SHELL_RADIUS, width=SHELL_WIDTH, density=SHELL_DENSITY):
    """``[G, G, G, 4]`` float32: sigma = density * exp(-(|p| - radius)^2 / (2 width^2)) at the vertices, colour logits that vary over the shell."""
    ax = torch.linspace(SHELL_BOX[0][0], SHELL_BOX[1][0], grid, dtype=torch.float64)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(xx * xx + yy * yy + zz * zz)
    vol = torch.stack([2.0 * torch.sin(3.0 * xx), 2.0 * torch.cos(3.0 * yy), 2.0 * zz, density * torch.exp(-(r - radius) ** 2 / (2 * width ** 2))], -1)
    return vol.to(torch.float32)


def shell_rays(side=16):
    """``side^2`` rays along +z through the box, slightly tilted, from a grid of origins in front of the shell: every ray crosses it twice, near
    its normal; near and far lie well outside the box, as a scene's bounds do."""
    ax = torch.linspace(-0.3, 0.3, side, dtype=torch.float64)
    oy, ox = torch.meshgrid(ax, ax, indexing="ij")
    n = side * side
    o = torch.stack([ox.reshape(n), oy.reshape(n), torch.full((n,), -3.0, dtype=torch.float64)], -1)
    d = torch.tensor([0.02, -0.015, 1.0], dtype=torch.float64).expand(n, 3)
    return torch.cat([o, d, torch.full((n, 1), SHELL_NEAR, dtype=torch.float64), torch.full((n, 1), SHELL_FAR, dtype=torch.float64)], -1).to(torch.float32)


def hierarchical_reference(vol, min_point, max_point, rays, n_samples, n_importance, dtype=torch.float64):
    """Coarse pass at the coarse spacing, sample_pdf (det) on weights[1:-1] at the mid-points, sort, fine pass: ``(fine, coarse, z_vals)``."""
    z = V.coarse_depths(rays, n_samples, False, dtype)
    coarse = V.render_reference(vol, min_point, max_point, rays, z, dtype=dtype)
    mids = 0.5 * (z[:, 1:] + z[:, :-1])
    new = O.sample_pdf_det(mids, coarse["weights"][:, 1:-1], n_importance)
    z_vals = torch.sort(torch.cat([z, new], -1), -1).values
    return V.render_reference(vol, min_point, max_point, rays, z_vals, dtype=dtype), coarse, z_vals


def mean_abs_errors(out, truth):
    """(mean |acc_map - truth|, mean |rgb_map - truth|) in float64."""
    return (float((out["acc_map"].double().cpu() - truth["acc_map"].double().cpu()).abs().mean()),
            float((out["rgb_map"].double().cpu() - truth["rgb_map"].double().cpu()).abs().mean()))
