"""CPU pinning of the grid_sample oracles the GPU tests trust (oracle/grid_sample_ref.py).

* grad2 (2-D) is the gradient of L = <g2_inp, grad_input> + <g2_grid, grad_grid> of ATen's
  own first backward (aten::grid_sampler_2d_backward): float64 central differences along
  random directions, in the four (padding, align_corners) modes.  The 3-D twin is
  tests/test_grid_sample3d_host.py.
* On a sample that sits exactly on a pixel, grad2 / grad3 take the cell to its right (floor),
  as ATen and the kernels do: with zeros padding the result at the lattice equals the result
  a hair to the right of it, to O(hair).
* With border padding the first and last row / column sit on the clip boundary, where ATen's
  clip_coordinates_set_grad zeroes the gradient: grad_grid is exactly 0 there.
* The 3-D double backward takes no NULL g2_* (include/bpk.h): checked without a device.
"""
import ctypes

import pytest
import torch

from grid_sample_cases import assert_off_lattice, assert_on_lattice, lattice_grid
from oracle import grid_sample_ref as gs

D64 = torch.float64
MODES = [(pm, ac) for pm in (0, 1) for ac in (True, False)]


def _L(gout, inp, grid, g2i, g2g, pm, ac):
    gi, gg = gs.bwd(gout, inp, grid, pm, ac)
    return (g2i * gi).sum() + (g2g * gg).sum()


@pytest.mark.parametrize("pm,ac", MODES)
def test_grad2_oracle_is_the_derivative_of_the_first_backward(pm, ac):
    g = torch.Generator().manual_seed(3)
    N, C, H, W, Ho, Wo = 2, 3, 5, 6, 4, 3
    inp = torch.randn(N, C, H, W, generator=g, dtype=D64)
    grid = torch.rand(N, Ho, Wo, 2, generator=g, dtype=D64) * 2.2 - 1.1
    # L is only piecewise smooth in the grid: no probe (eps x |direction| x size / 2 < 1e-4
    # pixel) may cross a cell or clip boundary
    assert_off_lattice(grid, (H, W), ac, margin=1e-3)
    gout = torch.randn(N, C, Ho, Wo, generator=g, dtype=D64)
    g2i = torch.randn(inp.shape, generator=g, dtype=D64)
    g2g = torch.randn(grid.shape, generator=g, dtype=D64)
    ggo, gin, ggrid = gs.grad2(g2i, g2g, gout, inp, grid, pm, ac)
    eps = 1e-6
    for k, (arg, grad) in enumerate(((gout, ggo), (inp, gin), (grid, ggrid))):
        for _ in range(3):
            dirn = torch.randn(arg.shape, generator=g, dtype=D64)
            args = [gout, inp, grid]
            args[k] = arg + eps * dirn
            lp = _L(*args, g2i, g2g, pm, ac)
            args[k] = arg - eps * dirn
            lm = _L(*args, g2i, g2g, pm, ac)
            fd = (lp - lm) / (2 * eps)
            an = (grad * dirn).sum()
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (k, float(fd), float(an))


# ------------------------------------------------------------------ exact-lattice grids
# delta: a shift of every grid coordinate to the right, far inside the cell (at most
# 33 / 2 x 1e-9 pixel).  grad2 / grad3 are polynomials in the in-cell offsets with
# coefficients bounded by |g2| |gout| |input| products (here < 1e3 summed over C and the
# corners) times size / 2, so the shift moves them by < 1e-4 of their scale; the wrong cell
# moves them by O(1).
_DELTA = 1e-9
_LATTICE_TOL = 1e-4

_SIZES_2D = [(True, (2, 2)), (True, (3, 3)), (True, (5, 9)), (True, (33, 17)), (True, (1, 3)),
             (False, (1, 1)), (False, (2, 2)), (False, (4, 16)), (False, (8, 8)), (False, (1, 4))]


def _close_to_shifted(at, shifted):
    for name, a, b in zip(("grad_grad_out", "grad_input", "grad_grid"), at, shifted):
        scale = max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max()) / scale
        assert err <= _LATTICE_TOL, f"{name}: on-lattice result is {err:.2e} from its right limit"


@pytest.mark.parametrize("ac,hw", _SIZES_2D)
def test_grad2_oracle_takes_the_right_cell_on_the_lattice(ac, hw):
    g = torch.Generator().manual_seed(11)
    N, C = 2, 3
    grid = lattice_grid(N, hw, ac, D64)
    assert_on_lattice(grid, hw, ac)
    inp = torch.randn(N, C, *hw, generator=g, dtype=D64)
    gout = torch.randn(N, C, *hw, generator=g, dtype=D64)
    g2i = torch.randn(inp.shape, generator=g, dtype=D64)
    g2g = torch.randn(grid.shape, generator=g, dtype=D64)
    at = gs.grad2(g2i, g2g, gout, inp, grid, 0, ac)
    _close_to_shifted(at, gs.grad2(g2i, g2g, gout, inp, grid + _DELTA, 0, ac))
    # and the first backward of ATen itself follows the same convention
    for a, b in zip(gs.bwd(gout, inp, grid, 0, ac), gs.bwd(gout, inp, grid + _DELTA, 0, ac)):
        assert float((a - b).abs().max()) <= _LATTICE_TOL * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("ac,dhw", [(True, (5, 5, 9)), (True, (2, 3, 1)), (False, (4, 2, 8)),
                                    (False, (1, 1, 2))])
def test_grad3_oracle_takes_the_right_cell_on_the_lattice(ac, dhw):
    g = torch.Generator().manual_seed(12)
    N, C = 1, 2
    grid = lattice_grid(N, dhw, ac, D64)
    assert_on_lattice(grid, dhw, ac)
    inp = torch.randn(N, C, *dhw, generator=g, dtype=D64)
    gout = torch.randn(N, C, *dhw, generator=g, dtype=D64)
    g2i = torch.randn(inp.shape, generator=g, dtype=D64)
    g2g = torch.randn(grid.shape, generator=g, dtype=D64)
    at = gs.grad3(g2i, g2g, gout, inp, grid, 0, ac)
    _close_to_shifted(at, gs.grad3(g2i, g2g, gout, inp, grid + _DELTA, 0, ac))
    for a, b in zip(gs.bwd3(gout, inp, grid, 0, ac), gs.bwd3(gout, inp, grid + _DELTA, 0, ac)):
        assert float((a - b).abs().max()) <= _LATTICE_TOL * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("ac,hw", _SIZES_2D)
def test_border_clip_zeroes_grad_grid_on_the_edge_pixels_2d(ac, hw):
    g = torch.Generator().manual_seed(13)
    N, C = 2, 3
    grid = lattice_grid(N, hw, ac, D64)
    inp = torch.randn(N, C, *hw, generator=g, dtype=D64)
    gout = torch.randn(N, C, *hw, generator=g, dtype=D64)
    g2i = torch.randn(inp.shape, generator=g, dtype=D64)
    g2g = torch.randn(grid.shape, generator=g, dtype=D64)
    for gg in (gs.bwd(gout, inp, grid, 1, ac)[1], gs.grad2(g2i, g2g, gout, inp, grid, 1, ac)[2]):
        assert (gg[:, :, [0, -1], 0] == 0).all(), "x gradient on the first / last column"
        assert (gg[:, [0, -1], :, 1] == 0).all(), "y gradient on the first / last row"
        if min(hw) >= 3:  # the clip is on the edge only: interior gradients are alive
            assert (gg[:, 1:-1, 1:-1] != 0).all()


@pytest.mark.parametrize("ac,dhw", [(True, (5, 5, 9)), (False, (4, 2, 8))])
def test_border_clip_zeroes_grad_grid_on_the_edge_voxels_3d(ac, dhw):
    g = torch.Generator().manual_seed(14)
    N, C = 1, 2
    grid = lattice_grid(N, dhw, ac, D64)
    inp = torch.randn(N, C, *dhw, generator=g, dtype=D64)
    gout = torch.randn(N, C, *dhw, generator=g, dtype=D64)
    g2i = torch.randn(inp.shape, generator=g, dtype=D64)
    g2g = torch.randn(grid.shape, generator=g, dtype=D64)
    for gg in (gs.bwd3(gout, inp, grid, 1, ac)[1],
               gs.grad3(g2i, g2g, gout, inp, grid, 1, ac)[2]):
        assert (gg[:, :, :, [0, -1], 0] == 0).all()
        assert (gg[:, :, [0, -1], :, 1] == 0).all()
        assert (gg[:, [0, -1], :, :, 2] == 0).all()


# ------------------------------------------------------------------ 3-D NULL contract
@pytest.mark.parametrize("suffix", ["f32", "f64"])
def test_grid_sample3d_grad2_refuses_null_incoming_gradients_without_a_device(suffix):
    """The 3-D double backward reads g2_input and g2_grid unconditionally, so NULL is an
    argument error -- reported before the N = 0 early return, i.e. with nothing launched: a
    library without the guard answers 0 here and fails this test on the host."""
    from op import _lib
    dll = _lib.lib.load()
    fn = getattr(dll, f"bpk_grid_sample3d_grad2_{suffix}")
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # never touched: N = 0
    shape = (0, 1, 2, 2, 2, 1, 1, 1, 0, 1, None)
    for g2i, g2g in ((None, None), (None, p), (p, None)):
        rc = fn(g2i, g2g, p, p, p, p, p, p, *shape)
        assert rc == 1
        assert b"g2_input and g2_grid required" in dll.bpk_last_error()
    assert fn(p, p, p, p, p, p, p, p, *shape) == 0


@pytest.mark.parametrize("suffix", ["f32", "f64"])
def test_grid_sample2d_grad2_takes_the_null_pointers_of_empty_outputs(suffix):
    """An empty tensor has no storage, so its data pointer is NULL: with N = 0 every output
    of the 2-D double backward is empty and the call is a no-op, not an argument error.  A
    missing output that has elements is still refused."""
    from op import _lib
    dll = _lib.lib.load()
    fn = getattr(dll, f"bpk_grid_sample2d_grad2_{suffix}")
    assert fn(None, None, None, None, None, None, None, None, 0, 3, 4, 5, 2, 2, 1, 1, None) == 0
    assert fn(None, None, None, None, None, None, None, None, 2, 3, 4, 5, 0, 2, 1, 1, None) == 1
    assert b"all outputs required" in dll.bpk_last_error()  # grad_input has 2 x 3 x 4 x 5
