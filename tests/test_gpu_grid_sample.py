"""GPU: the grid_sample kernels (csrc/grid_sample.hip, csrc/grid_sample3d.hip) where the PINN
uses them -- the channel-sliced launches (C >= 16), the float32 double backward, samples
that sit exactly on a pixel or on the border clip, far out-of-range samples, the grid-stride
loops, NULL incoming gradients and empty tensors.

Truth is a float64 CPU reference fed the kernel's own inputs: ATen for the forward and the
first backward, oracle/grid_sample_ref.grad2 / grad3 (pinned in test_oracle_grid_sample.py
and test_grid_sample3d_host.py) for the double backward.

Tolerances.  float64 kernels: rtol = atol = 1e-10 against that truth (1e-12 where stated).
float32 kernels, per output tensor and relative to max |truth|:
    err(kernel) <= max(1e-5, 2 x err(the same reference run in float32)).
float64 truth says nothing about a float32 kernel at a sample whose cell differs between
the precisions, so every grid here is either exactly on the pixel lattice in both precisions
or at least 1e-3 pixel away from it; that is asserted on the inputs before any launch.
"""
import numpy as np
import pytest
import torch

from conftest import record_err
from grid_sample_cases import (assert_off_lattice, assert_on_lattice, lattice_grid, normalize)
from oracle import grid_sample_ref as gs

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
MODES = [(pm, ac) for pm in (0, 1) for ac in (True, False)]
NAMES2 = ("fwd", "bwd.grad_input", "bwd.grad_grid", "grad2.grad_grad_out", "grad2.grad_input",
          "grad2.grad_grid")


# ------------------------------------------------------------------ comparison helpers
def _gate32(what, got, ref64, ref32):
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    if scale == 0.0:
        assert not got.any(), f"{what}: truth is all zero, the kernel's output is not"
        return
    err = float((got.double() - ref64).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    tol = max(1e-5, 2 * e32)
    record_err(what, err, tol)
    print(f"{what}: err {err:.3e}  float32 reference {e32:.3e}  tol {tol:.3e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e} (float32 reference {e32:.3e})"


def _close64(what, got, ref64, tol):
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    err = float((got - ref64).abs().max()) / max(scale, 1e-300) if ref64.numel() else 0.0
    record_err(what, err, tol)
    print(f"{what}: err {err:.3e}  tol {tol:.0e}")
    np.testing.assert_allclose(got.numpy(), ref64.numpy(), rtol=tol, atol=tol, err_msg=what)


def _cast(t, dtype):
    return {k: v.to(dtype) for k, v in t.items()}


def _ref2(t, pm, ac):
    """(fwd, bwd.grad_input, bwd.grad_grid, grad2.*) of the CPU references in t's dtype."""
    out = gs.fwd(t["inp"], t["grid"], pm, ac)
    gi, gg = gs.bwd(t["gout"], t["inp"], t["grid"], pm, ac)
    return (out, gi, gg) + tuple(gs.grad2(t["g2i"], t["g2g"], t["gout"], t["inp"], t["grid"],
                                          pm, ac))


def _run2(hip, t, pm, ac):
    from op import grid_sample as R
    d = {k: v.to(hip) for k, v in t.items()}
    out = R.grid_sample2d_fwd_raw(d["inp"], d["grid"], pm, ac)
    gi, gg = R.grid_sample2d_bwd_raw(d["gout"], d["inp"], d["grid"], pm, ac)
    g2 = R.grid_sample2d_grad2_raw(d["g2i"], d["g2g"], d["gout"], d["inp"], d["grid"], pm, ac)
    return tuple(x.cpu() for x in (out, gi, gg) + tuple(g2))


def _ref3(t, pm, ac):
    out = gs.fwd3(t["inp"], t["grid"], pm, ac)
    gi, gg = gs.bwd3(t["gout"], t["inp"], t["grid"], pm, ac)
    return (out, gi, gg) + tuple(gs.grad3(t["g2i"], t["g2g"], t["gout"], t["inp"], t["grid"],
                                          pm, ac))


def _run3(hip, t, pm, ac):
    from op import grid_sample as R
    d = {k: v.to(hip) for k, v in t.items()}
    out = R.grid_sample3d_fwd_raw(d["inp"], d["grid"], pm, ac)
    gi, gg = R.grid_sample3d_bwd_raw(d["gout"], d["inp"], d["grid"], pm, ac)
    g2 = R.grid_sample3d_grad2_raw(d["g2i"], d["g2g"], d["gout"], d["inp"], d["grid"], pm, ac)
    return tuple(x.cpu() for x in (out, gi, gg) + tuple(g2))


_TRUTH = {}


def _check(tag, got, t, pm, ac, ref=_ref2, tol64=1e-10, key=None):
    """Compare the six outputs `got` of a kernel run on inputs t (in the kernel's dtype) with
    the float64 reference of the same values.  `key` shares one truth between the float32
    and float64 runs of a case."""
    if key is None or key not in _TRUTH:
        truth = ref(_cast(t, F64), pm, ac)
        if key is not None:
            _TRUTH[key] = truth
    else:
        truth = _TRUTH[key]
    if t["inp"].dtype == F32:
        for name, a, r64, r32 in zip(NAMES2, got, truth, ref(t, pm, ac)):
            _gate32(f"{tag} {name} f32", a, r64, r32)
    else:
        for name, a, r64 in zip(NAMES2, got, truth):
            _close64(f"{tag} {name} f64", a, r64, tol64)


def _inputs(g, N, C, in_sizes, grid, dtype):
    """Random input / grad_out / incoming second-order gradients around a given grid; drawn
    in float32, so the float32 and float64 runs of a case see the same values."""
    out_sizes = tuple(grid.shape[1:-1])
    t = {"inp": torch.randn(N, C, *in_sizes, generator=g),
         "grid": grid.float(),
         "gout": torch.randn(N, C, *out_sizes, generator=g),
         "g2i": torch.randn(N, C, *in_sizes, generator=g),
         "g2g": torch.randn(*grid.shape, generator=g)}
    assert torch.equal(t["grid"].double(), grid.double()), "grid must be float32-representable"
    return _cast(t, dtype)


# ------------------------------------------------------------------ B.1 channel slices
# seeds for which every sample of the [-1.2, 1.2] grid is >= 1e-3 pixel off the 6 x 9
# lattice under both align_corners conventions (asserted below)
_B1_OUT = {(2, 5, 7): 0, (3, 13, 11): 35}


def _b1_grid(out_shape):
    g = torch.Generator().manual_seed(_B1_OUT[out_shape])
    return torch.rand(*out_shape, 2, generator=g) * 2.4 - 1.2


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("pm,ac", MODES)
@pytest.mark.parametrize("C", [1, 3, 4, 7, 16, 19, 40])
def test_channel_slices_and_ragged_blocks(hip, C, pm, ac, dtype):
    """S = 1, 1, 4, 4, 8, 8, 8 channel slices with C % S != 0 in each sliced class; 70
    locations leave 6 in the last 32-location block of the S = 8 launch, 429 make it 14
    blocks."""
    H, W = 6, 9
    for out_shape in _B1_OUT:
        grid = _b1_grid(out_shape)
        assert_off_lattice(grid, (H, W), ac)
        g = torch.Generator().manual_seed(100 + C)
        t = _inputs(g, out_shape[0], C, (H, W), grid, dtype)
        tag = f"slices C={C} out={out_shape} pm={pm} ac={int(ac)}"
        _check(tag, _run2(hip, t, pm, ac), t, pm, ac, key=("b1", C, out_shape, pm, ac))


# ------------------------------------------------------------------ B.2 the PINN's warp
@pytest.mark.parametrize("N,C,H,W", [(4, 128, 2, 2), (4, 96, 4, 4), (2, 32, 16, 16),
                                      (2, 16, 32, 32)])
def test_pinn_warp_configuration_f32(hip, N, C, H, W):
    """grid = identity - flow as models/flownet.project builds it (border padding,
    align_corners=True, float32), the flow moving every sample by a fractional 0.1 .. 0.9
    pixel of either sign, up to 1.5 pixels: near-identity grids stack four contributions on
    every input pixel (contended atomics), and the samples pushed outside are clipped."""
    from models import flownet
    from op import channels
    g = torch.Generator().manual_seed(7 * H + C)
    frac = 0.1 + 0.8 * torch.rand(N, 2, H, W, generator=g)
    mag = frac + torch.randint(0, 2, (N, 2, H, W), generator=g)
    mag = torch.where(mag > 1.5, mag - 1, mag)
    u = (mag * (torch.randint(0, 2, (N, 2, H, W), generator=g) * 2 - 1)).to(hip)
    dt = 1.0
    with torch.no_grad():
        base = flownet._base_grid(u.shape, u.device)
        step = channels.swap_scale(u, (H - 1.0) / 2.0, (W - 1.0) / 2.0)
        grid = (base - step * dt).permute(0, 2, 3, 1).contiguous().cpu()
    assert_off_lattice(grid, (H, W), True, margin=0.05)
    ix = (grid[..., 0].double() + 1) / 2 * (W - 1)
    assert (ix < 0).any() and (ix > W - 1).any(), "some samples must be clipped"
    t = _inputs(g, N, C, (H, W), grid, F32)
    _check(f"pinn warp [{N},{C},{H},{W}]", _run2(hip, t, 1, True), t, 1, True)


# ------------------------------------------------------------------ B.3 exact lattice
# size - 1 (align_corners=True) or size (False) a power of two: the unnormalised coordinates
# are exact integers in float32 and float64 (asserted).  Other sizes are not, and the two
# precisions then disagree on the cell at several pixels.
_LATTICE = ([(True, (s, s)) for s in (2, 3, 5, 9, 17, 33)] + [(True, (5, 9)), (True, (1, 1)),
                                                               (True, (1, 3))] +
            [(False, (s, s)) for s in (1, 2, 4, 8, 16)] + [(False, (4, 16)), (False, (1, 8))])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("ac,hw", _LATTICE)
def test_samples_exactly_on_the_pixels(hip, ac, hw, dtype):
    """A zero flow -- the coarsest pyramid level -- samples every pixel centre, and the first
    and last row / column sit on the border clip, whose gradient ATen defines as 0."""
    N, C = 2, 17
    grid = lattice_grid(N, hw, ac, F32)
    assert_on_lattice(grid, hw, ac)
    assert_on_lattice(grid.double(), hw, ac)
    g = torch.Generator().manual_seed(31)
    t = _inputs(g, N, C, hw, grid, dtype)
    for pm in (0, 1):
        got = _run2(hip, t, pm, ac)
        tag = f"lattice {hw} pm={pm} ac={int(ac)}"
        assert torch.equal(got[0], t["inp"]), f"{tag}: the forward is not the identity"
        _check(tag, got, t, pm, ac, tol64=1e-12, key=("b3", ac, hw, pm))
        if pm == 1:
            for name, gg in (("bwd", got[2]), ("grad2", got[5])):
                assert (gg[:, :, [0, -1], 0] == 0).all(), f"{tag} {name}: x gradient, edge columns"
                assert (gg[:, [0, -1], :, 1] == 0).all(), f"{tag} {name}: y gradient, edge rows"
                if min(hw) >= 3:
                    assert (gg[:, 1:-1, 1:-1] != 0).all(), f"{tag} {name}: interior gradient is 0"


# ------------------------------------------------------------------ B.4 far out of range
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("pm,ac", MODES)
def test_far_out_of_range_samples(hip, pm, ac, dtype):
    """Finite coordinates far outside the image (no inf / NaN: the cast to int is then
    outside what ATen defines): zeros padding gives exactly 0, border padding the nearest
    corner pixel, and grad_grid is exactly 0 either way."""
    N, C, H, W = 2, 5, 6, 9
    vals = torch.tensor([-1e6, -1e4, -3.0, 3.0, 1e4, 1e6])
    grid = torch.stack(torch.meshgrid(vals, vals, indexing="ij")[::-1], -1)  # [6, 6, (x, y)]
    grid = grid.unsqueeze(0).expand(N, 6, 6, 2).contiguous()
    g = torch.Generator().manual_seed(41)
    t = _inputs(g, N, C, (H, W), grid, dtype)
    got = _run2(hip, t, pm, ac)
    if pm == 0:
        assert not got[0].any() and not got[1].any()
    else:
        rows = torch.tensor([0, 0, 0, H - 1, H - 1, H - 1])
        cols = torch.tensor([0, 0, 0, W - 1, W - 1, W - 1])
        assert torch.equal(got[0], t["inp"][:, :, rows][:, :, :, cols])
    assert not got[2].any(), "bwd grad_grid"
    assert not got[5].any(), "grad2 grad_grid"
    _check(f"far pm={pm} ac={int(ac)}", got, t, pm, ac, tol64=1e-12)


def _in_cell_grid(g, shape, sizes, ac):
    """float64 grid [*shape, len(sizes)] whose samples lie at integer + [0.01, 0.99] pixels,
    from one cell outside the image to one cell outside on the other side."""
    comps = []
    for size in sizes[::-1]:
        cell = torch.randint(-1, size, shape, generator=g).double()
        off = 0.01 + 0.98 * torch.rand(shape, generator=g, dtype=F64)
        comps.append(normalize(cell + off, size, ac))
    return torch.stack(comps, -1)


# ------------------------------------------------------------------ B.5 forward stride loop
def test_forward_stride_loop(hip):
    """gs_fwd launches at most 8192 x 256 threads: 2 x 1025 x 1025 = 2 101 250 locations
    make 4098 of them take a second trip through the grid-stride loop."""
    from op import grid_sample as R
    g = torch.Generator().manual_seed(51)
    N, H, W, Ho, Wo = 2, 8, 8, 1025, 1025
    assert N * Ho * Wo > 8192 * 256
    grid = _in_cell_grid(g, (N, Ho, Wo), (H, W), False)
    assert_off_lattice(grid, (H, W), False)
    inp = torch.randn(N, 1, H, W, generator=g, dtype=F64)
    for pm in (0, 1):
        out = R.grid_sample2d_fwd_raw(inp.to(hip), grid.to(hip), pm, False).cpu()
        _close64(f"fwd stride loop pm={pm} f64", out, gs.fwd(inp, grid, pm, False), 1e-10)


# ------------------------------------------------------------------ B.6 NULL paths, empties
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("C", [3, 19])
def test_bwd_null_outputs(hip, C, dtype):
    """A NULL grad_input / grad_grid skips that output and leaves the other bit for bit.
    grad_input is accumulated with atomics in no fixed order, so the samples here are three
    pixels apart: no two of them share a corner and every sum has one term."""
    from op import grid_sample as R
    N, H, W, Ho, Wo = 2, 9, 12, 3, 4
    g = torch.Generator().manual_seed(61)
    iy = 3 * torch.arange(Ho).double().view(1, Ho, 1) + 0.2 + 0.6 * torch.rand(N, Ho, Wo, generator=g)
    ix = 3 * torch.arange(Wo).double().view(1, 1, Wo) + 0.2 + 0.6 * torch.rand(N, Ho, Wo, generator=g)
    grid = torch.stack([normalize(ix, W, True), normalize(iy, H, True)], -1).float()
    assert_off_lattice(grid, (H, W), True, margin=0.1)
    inp = torch.randn(N, C, H, W, generator=g).to(dtype).to(hip)
    gout = torch.randn(N, C, Ho, Wo, generator=g).to(dtype).to(hip)
    grid = grid.to(dtype).to(hip)
    for pm in (0, 1):
        gi, gg = R.grid_sample2d_bwd_raw(gout, inp, grid, pm, True)
        gi_only, none_g = R.grid_sample2d_bwd_raw(gout, inp, grid, pm, True, need_grid=False)
        none_i, gg_only = R.grid_sample2d_bwd_raw(gout, inp, grid, pm, True, need_input=False)
        assert none_g is None and none_i is None
        assert gi.abs().sum() > 0 and gg.abs().sum() > 0
        assert torch.equal(gi_only, gi)
        assert torch.equal(gg_only, gg)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("C", [3, 19])
def test_grad2_null_incoming_gradients_are_zeros(hip, C, dtype):
    """g2_input / g2_grid = None (what autograd passes for an unused output) against
    explicit zeros: grad_grad_out and grad_grid bit for bit; grad_input, whose atomic order
    is free, to 1e-12 of its scale in float64 (and one float32 rounding, 1e-6, in float32)."""
    from op import grid_sample as R
    N, H, W = 2, 6, 9
    grid = _b1_grid((2, 5, 7))
    assert_off_lattice(grid, (H, W), True)
    g = torch.Generator().manual_seed(62)
    t = {k: v.to(hip) for k, v in _inputs(g, N, C, (H, W), grid, dtype).items()}
    zi, zg = torch.zeros_like(t["g2i"]), torch.zeros_like(t["g2g"])
    for pm in (0, 1):
        for g2i, g2g in ((None, t["g2g"]), (t["g2i"], None), (None, None)):
            got = R.grid_sample2d_grad2_raw(g2i, g2g, t["gout"], t["inp"], t["grid"], pm, True)
            ref = R.grid_sample2d_grad2_raw(zi if g2i is None else g2i, zg if g2g is None else g2g,
                                            t["gout"], t["inp"], t["grid"], pm, True)
            assert torch.equal(got[0], ref[0]), "grad_grad_out"
            assert torch.equal(got[2], ref[2]), "grad_grid"
            scale = max(float(ref[1].abs().max()), 1e-30)
            err = float((got[1] - ref[1]).abs().max()) / scale
            assert err <= (1e-12 if dtype == F64 else 1e-6), f"grad_input {err:.2e}"
            if g2i is None and g2g is None:
                assert not got[0].any() and not got[1].any() and not got[2].any()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("N,C,Ho", [(0, 3, 4), (2, 0, 4), (2, 3, 0), (2, 19, 0), (0, 0, 0)])
def test_empty_tensors(hip, N, C, Ho, dtype):
    """N = 0, C = 0 or H_out = 0: right shapes, zeros where anything is left, no error --
    through the raw entries and through autograd."""
    from op import grid_sample as R
    H, W, Wo = 4, 5, 3
    g = torch.Generator().manual_seed(63)
    grid = (torch.rand(N, Ho, Wo, 2, generator=g) * 2 - 1)
    t = {k: v.to(hip) for k, v in _inputs(g, N, C, (H, W), grid, dtype).items()}
    for pm, ac in MODES:
        out = R.grid_sample2d_fwd_raw(t["inp"], t["grid"], pm, ac)
        assert out.shape == (N, C, Ho, Wo) and out.dtype == dtype
        gi, gg = R.grid_sample2d_bwd_raw(t["gout"], t["inp"], t["grid"], pm, ac)
        ggo, gi2, gg2 = R.grid_sample2d_grad2_raw(t["g2i"], t["g2g"], t["gout"], t["inp"],
                                                  t["grid"], pm, ac)
        assert ggo.shape == (N, C, Ho, Wo)
        for a in (gi, gi2):
            assert a.shape == (N, C, H, W) and not a.any()
        for a in (gg, gg2):  # C = 0: the channel sum is empty, as in ATen
            assert a.shape == (N, Ho, Wo, 2) and not a.any()
        ri, rg = gs.bwd(*(t[k].cpu() for k in ("gout", "inp", "grid")), pm, ac)
        assert ri.shape == gi.shape and rg.shape == gg.shape and not ri.any() and not rg.any()
    inp, grid = t["inp"].clone().requires_grad_(True), t["grid"].clone().requires_grad_(True)
    out = R.grid_sample_2d(inp, grid, "border", True)
    d_inp, d_grid = torch.autograd.grad(out.sum(), (inp, grid), create_graph=True)
    (d_inp.sum() + (d_grid ** 2).sum()).backward()
    assert inp.grad.shape == inp.shape and grid.grad.shape == grid.shape
    assert not inp.grad.any() and not grid.grad.any()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ C. 3-D kernels
_C_SEED = 0  # every sample of the 3-D grid below is >= 1e-3 voxel off the 4 x 5 x 6 lattice


@pytest.mark.parametrize("pm", [0, 1])
def test_grid_sample_3d_grad2_align_corners_false(hip, pm):
    g = torch.Generator().manual_seed(_C_SEED)
    N, C, dhw = 2, 3, (4, 5, 6)
    grid = torch.rand(N, 3, 2, 4, 3, generator=g) * 2.4 - 1.2
    assert_off_lattice(grid, dhw, False)
    t = _inputs(g, N, C, dhw, grid, F64)
    _check(f"3d pm={pm} ac=0", _run3(hip, t, pm, False), t, pm, False, ref=_ref3)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_grid_sample_3d_samples_exactly_on_the_voxels(hip, dtype):
    N, C, dhw = 1, 3, (5, 5, 9)
    grid = lattice_grid(N, dhw, True, F32)
    assert_on_lattice(grid, dhw, True)
    assert_on_lattice(grid.double(), dhw, True)
    g = torch.Generator().manual_seed(71)
    t = _inputs(g, N, C, dhw, grid, dtype)
    for pm in (0, 1):
        got = _run3(hip, t, pm, True)
        tag = f"3d lattice pm={pm}"
        assert torch.equal(got[0], t["inp"]), f"{tag}: the forward is not the identity"
        _check(tag, got, t, pm, True, ref=_ref3, tol64=1e-12)
        if pm == 1:
            for name, gg in (("bwd", got[2]), ("grad2", got[5])):
                assert (gg[:, :, :, [0, -1], 0] == 0).all(), f"{tag} {name}: x"
                assert (gg[:, :, [0, -1], :, 1] == 0).all(), f"{tag} {name}: y"
                assert (gg[:, [0, -1], :, :, 2] == 0).all(), f"{tag} {name}: z"
                assert (gg[:, 1:-1, 1:-1, 1:-1] != 0).all(), f"{tag} {name}: interior"


def test_grid_sample_3d_stride_loops(hip):
    """129^3 = 2 146 689 locations > 8192 x 256: all three 3-D kernels loop."""
    N, C, dhw, n = 1, 1, (9, 9, 9), 129
    assert n ** 3 > 8192 * 256
    g = torch.Generator().manual_seed(72)
    grid = _in_cell_grid(g, (N, n, n, n), dhw, True)
    assert_off_lattice(grid, dhw, True)
    t = {"inp": torch.randn(N, C, *dhw, generator=g, dtype=F64), "grid": grid,
         "gout": torch.randn(N, C, n, n, n, generator=g, dtype=F64),
         "g2i": torch.randn(N, C, *dhw, generator=g, dtype=F64),
         "g2g": torch.randn(N, n, n, n, 3, generator=g, dtype=F64)}
    _check("3d stride loop", _run3(hip, t, 1, True), t, 1, True, ref=_ref3)


def test_grid_sample_3d_empty_tensors(hip):
    from op import grid_sample as R
    for N, C, Do in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        inp = torch.zeros(N, C, 2, 3, 4, dtype=F64, device=hip)
        grid = torch.zeros(N, Do, 2, 2, 3, dtype=F64, device=hip)
        gout = torch.zeros(N, C, Do, 2, 2, dtype=F64, device=hip)
        assert R.grid_sample3d_fwd_raw(inp, grid, 1, True).shape == gout.shape
        gi, gg = R.grid_sample3d_bwd_raw(gout, inp, grid, 1, True)
        ggo, gi2, gg2 = R.grid_sample3d_grad2_raw(torch.zeros_like(inp), torch.zeros_like(grid),
                                                  gout, inp, grid, 1, True)
        assert ggo.shape == gout.shape
        for a, like in ((gi, inp), (gi2, inp), (gg, grid), (gg2, grid)):
            assert a.shape == like.shape and not a.any()
    torch.cuda.synchronize()
