"""Sampling grids shared by the grid_sample oracle pins (test_oracle_grid_sample.py) and the
GPU tests (test_gpu_grid_sample.py), and the assertions both make on their inputs.

A float64 reference is the truth for a float32 kernel only where both precisions put a
sample into the same cell, so a test grid is either exactly on the pixel lattice in both
precisions (`lattice_grid`) or provably away from it (`assert_off_lattice`)."""
import torch


def unnormalize(coord, size, align):
    """ATen's grid_sampler_unnormalize, in float64."""
    coord = coord.double()
    if align:
        return (coord + 1) / 2 * (size - 1)
    return ((coord + 1) * size - 1) / 2


def normalize(ix, size, align):
    """Inverse of unnormalize (float64): the grid value that samples pixel coordinate ix."""
    ix = ix.double()
    if align:
        return 2 * ix / (size - 1) - 1
    return (2 * ix + 1) / size - 1


def lattice_axis(size, align, dtype):
    """Grid values that sample the `size` pixel centres of an axis.  Exact in float32 and
    float64 when size - 1 (align_corners=True) or size (False) is a power of two, or 1."""
    if align:
        return torch.linspace(-1.0, 1.0, size, dtype=dtype)
    return ((2 * torch.arange(size, dtype=dtype) + 1) / size - 1).to(dtype)


def lattice_grid(N, sizes, align, dtype):
    """Identity grid [N, *sizes, len(sizes)] on the pixel centres of an input of spatial
    `sizes` ((H, W) or (D, H, W)); the last dim is (x, y[, z]) as grid_sample wants it."""
    axes = [lattice_axis(s, align, dtype) for s in sizes]
    mesh = torch.meshgrid(*axes, indexing="ij")
    g = torch.stack(mesh[::-1], dim=-1)
    return g.unsqueeze(0).expand(N, *g.shape).contiguous()


def _coords(grid, sizes, align):
    """Unnormalised float64 coordinates, one tensor per grid component (x: last size)."""
    return [unnormalize(grid[..., k], sizes[len(sizes) - 1 - k], align) for k in range(len(sizes))]


def assert_on_lattice(grid, sizes, align):
    """Every coordinate of `grid` is an exact integer -- in float64, and in the arithmetic of
    grid's own dtype, which is what a kernel of that dtype evaluates."""
    for k, ix in enumerate(_coords(grid, sizes, align)):
        assert torch.equal(ix, ix.round()), f"component {k} is off the lattice in float64"
        size = sizes[len(sizes) - 1 - k]
        c = grid[..., k]
        own = (c + 1) / 2 * (size - 1) if align else ((c + 1) * size - 1) / 2
        assert torch.equal(own.double(), ix), f"component {k} is off the lattice in {grid.dtype}"


def lattice_distance(grid, sizes, align):
    """Smallest distance of any unnormalised float64 coordinate from an integer.  0 and
    size - 1, where border padding clips, are integers, so they are covered."""
    return min(float((ix - ix.round()).abs().min()) for ix in _coords(grid, sizes, align))


def assert_off_lattice(grid, sizes, align, margin=1e-3):
    d = lattice_distance(grid, sizes, align)
    assert d >= margin, f"a sample lies {d:.2e} from the pixel lattice (margin {margin:.0e})"
