"""CPU: the blur measurement operator's definition (taps, boundary, decimation, adjoint) as
restated in tests/blur_ref.py against scipy, and the host side of op.blur / the operator
factory (argument validation, configs, no CPU path)."""
import ctypes

import numpy as np
import pytest
import torch

import blur_ref

SHAPES = [(7, 9), (16, 16), (2, 5)]          # (2, 5) with K = 5 is H = p


def _x(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape)


@pytest.mark.parametrize("K,std", [(5, 1.0), (9, 3.0), (13, 4.0), (1, 1.0)])
def test_taps_are_the_separated_multivariate_normal_grid(K, std):
    from scipy.stats import multivariate_normal
    from op.blur import gaussian_taps
    g = gaussian_taps(std, K)
    assert g.dtype == torch.float64 and g.device.type == "cpu" and g.shape == (K,)
    a = np.arange(K) - K // 2
    grid = np.stack(np.meshgrid(a, a), axis=-1)
    pdf = np.atleast_2d(multivariate_normal([0, 0], std * np.eye(2)).pdf(grid))
    want = pdf / pdf.sum()
    g = g.numpy()
    assert np.abs(np.outer(g, g) - want).max() <= 1e-15
    assert np.abs(blur_ref.taps(std, K) - g).max() <= 1e-16


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_is_scipy_symm_same(shape):
    from scipy.signal import convolve2d
    g = blur_ref.taps(2.0, 5)
    x = _x(shape)
    want = convolve2d(x, np.outer(g, g), boundary="symm", mode="same")
    assert np.abs(blur_ref.forward(x, g, 1) - want).max() <= 1e-13
    for s in (2, 3, 4):
        o = (s - 1) // 2
        y = blur_ref.forward(x, g, s)
        assert y.shape == want[o::s, o::s].shape == (blur_ref.out_size(shape[0], s),
                                                     blur_ref.out_size(shape[1], s))
        assert np.abs(y - want[o::s, o::s]).max() <= 1e-13
    assert blur_ref.forward(_x((7, 9)), g, 2).shape == (4, 5)


def test_forward_flips_asymmetric_taps_as_a_convolution():
    from scipy.signal import convolve2d
    g = np.array([0.5, 0.3, 0.1, 0.07, 0.03])
    x = _x((7, 9), 3)
    want = convolve2d(x, np.outer(g, g), boundary="symm", mode="same")
    assert np.abs(blur_ref.forward(x, g, 1) - want).max() <= 1e-13


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_adjoint_identity_of_the_restatement(shape, s):
    for g in (blur_ref.taps(2.0, 5), np.array([0.5, 0.3, 0.1, 0.07, 0.03])):
        x = _x((3,) + shape, 1)
        Ax = blur_ref.forward(x, g, s)
        y = _x(Ax.shape, 2)
        lhs, rhs = np.sum(Ax * y), np.sum(x * blur_ref.adjoint(y, g, s, shape))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


def test_argument_validation_needs_no_device():
    from op import _lib
    from op.blur import MAX_TAPS, blur2d, blur2d_adjoint, gaussian_taps, out_size
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError, match="odd"):
        blur2d(x, [0.25] * 4)
    with pytest.raises(ValueError, match="odd"):
        blur2d(x, [1 / 35] * 35)
    with pytest.raises(ValueError, match="odd"):
        gaussian_taps(1.0, 4)
    with pytest.raises(ValueError):
        gaussian_taps(1.0, MAX_TAPS + 2)
    with pytest.raises(ValueError, match="halo"):
        blur2d(torch.zeros(1, 1, 2, 5), [1 / 7] * 7)           # p = 3 > min(H, W) = 2
    with pytest.raises(ValueError, match="stride"):
        blur2d(x, [1.0], stride=0)
    with pytest.raises(ValueError, match="stride"):
        blur2d_adjoint(x, [1.0], 0, (8, 8))
    with pytest.raises(ValueError, match="needs"):
        blur2d_adjoint(x, [1.0], 2, (8, 8))                    # y would be 4 x 4
    assert out_size(7, 9, 5, 2) == (4, 5) and out_size(2, 5, 5, 1) == (2, 5)
    # the C entry points refuse the same arguments before any HIP call
    dll = _lib.lib.load()
    g = (ctypes.c_double * 35)(*([0.0] * 35))
    for fn in (dll.bpk_blur2d_f32, dll.bpk_blur2d_f64, dll.bpk_blur2d_adjoint_f32,
               dll.bpk_blur2d_adjoint_f64):
        assert fn(None, None, 1, 8, 8, g, 4, 1, None) == 1 and b"odd" in dll.bpk_last_error()
        assert fn(None, None, 1, 8, 8, g, 35, 1, None) == 1 and b"odd" in dll.bpk_last_error()
        assert fn(None, None, 1, 2, 5, g, 7, 1, None) == 1 and b"halo" in dll.bpk_last_error()
        assert fn(None, None, 1, 8, 8, g, 3, 0, None) == 1 and b"stride" in dll.bpk_last_error()
        assert fn(None, None, 1, 8, 8, None, 3, 1, None) == 1 and b"taps" in dll.bpk_last_error()
        assert fn(None, None, 1, 8, 8, g, 3, 1, None) == 1 and b"NULL" in dll.bpk_last_error()
        assert fn(None, None, 0, 8, 8, g, 3, 1, None) == 0      # nothing to do


def test_cpu_tensor_raises():
    from op.blur import blur2d, blur2d_adjoint
    with pytest.raises(RuntimeError, match="HIP"):
        blur2d(torch.zeros(1, 1, 8, 8), [0.25, 0.5, 0.25])
    with pytest.raises(RuntimeError, match="HIP"):
        blur2d_adjoint(torch.zeros(1, 1, 4, 4), [0.25, 0.5, 0.25], 2, (8, 8))


def test_get_operator_builds_the_new_operators_and_still_inpainting():
    from configs.inverse import nc_ddpmpp_deblur_dps, nc_ddpmpp_inpaint_dps, nc_ddpmpp_sr_dps
    from inverse.operators import GaussianBlurOperator, InpaintOperator, get_operator
    c = nc_ddpmpp_deblur_dps.get_config()
    op = get_operator(c)
    assert isinstance(op, GaussianBlurOperator) and op.factor == 1
    assert (c.inverse.blur_size, c.inverse.blur_std) == (13, 4.0)
    assert np.abs(op.taps.numpy() - blur_ref.taps(4.0, 13)).max() <= 1e-16
    assert op.out_shape((16, 1, 256, 256)) == (16, 1, 256, 256)
    op.next()
    c = nc_ddpmpp_sr_dps.get_config()
    op = get_operator(c)
    assert isinstance(op, GaussianBlurOperator) and op.factor == c.inverse.factor == 4
    assert op.taps.numel() == 13 and op.out_shape((16, 1, 256, 256)) == (16, 1, 64, 64)
    with pytest.raises(ValueError):
        op(torch.zeros(1, 1, 16, 16), invert=True)
    old = nc_ddpmpp_inpaint_dps.get_config()
    for c in (c, nc_ddpmpp_deblur_dps.get_config()):            # only the operator section differs
        assert (c.inverse.variance, c.inverse.solver, c.inverse.sampler, c.training.batch_size) == \
            (old.inverse.variance, old.inverse.solver, old.inverse.sampler, old.training.batch_size)
    mask = torch.ones(16, 1, 8, 8)
    op = get_operator(old, mask_source=[mask])
    assert isinstance(op, InpaintOperator) and op.mask is mask
    old.inverse.operator = "colorization"
    with pytest.raises(NotImplementedError):
        get_operator(old)
