"""The autograd triple of op/conv.py (`_Conv`, `_ConvT`, `_Wgrad`) on the host: float64 on the
CPU, where every raw dispatcher falls through to aten, so `gradcheck` and `gradgradcheck` test
the wiring of the three backward passes alone -- once per `kind` that has a CPU path.  The 1x1
kind has none (its GEMM needs the library); tests/test_gpu_ops.py checks its second order.

No GPU and no libbpk.so: the library handle is replaced by one that fails on any use.  The one
raw function of the 3x3 kind without an aten form is the unfused residual tail
(op.norm_act.residual_rescale, a HIP kernel); the test puts (skip + y) / div in its place."""
import pytest
import torch
import torch.nn.functional as F

D = torch.float64


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"host autograd test reached libbpk ({name})")


@pytest.fixture
def conv(monkeypatch):
    from op import conv, norm_act
    monkeypatch.setattr(conv, "lib", _NoLib())
    monkeypatch.setattr(norm_act, "residual_rescale",
                        lambda x, h, bias=None, div=2 ** 0.5: (x + h) / div)
    return conv


def _leaves(seed, *shapes):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*s, dtype=D, generator=g).requires_grad_() for s in shapes)


def _check(f, inputs):
    assert torch.autograd.gradcheck(f, inputs)
    assert torch.autograd.gradgradcheck(f, inputs)


def test_3x3_kind_bias_skip_div(conv):
    x, w, b, skip = _leaves(1, (2, 3, 5, 6), (4, 3, 3, 3), (4,), (2, 4, 5, 6))
    f = lambda x, w, b, skip: conv._Conv.apply(x, w, b, skip, 1.5, ("3x3",))  # noqa: E731
    assert torch.allclose(f(x, w, b, skip), (skip + F.conv2d(x, w, b, padding=1)) / 1.5,
                          rtol=0, atol=1e-12)
    _check(f, (x, w, b, skip))


def test_3x3_adjoint_and_weight_gradient_nodes(conv):
    """the other two Functions entered directly (in a network they are reached through _Conv's
    backward only)"""
    u, w, x = _leaves(2, (2, 4, 5, 6), (4, 3, 3, 3), (2, 3, 5, 6))
    k = ("3x3",)
    ft = lambda u, w: conv._ConvT.apply(u, w, (2, 3, 5, 6), k)  # noqa: E731
    assert torch.allclose(ft(u, w), F.conv_transpose2d(u, w, padding=1), rtol=0, atol=1e-12)
    _check(ft, (u, w))
    _check(lambda x, u: conv._Wgrad.apply(x, u, (4, 3, 3, 3), True, k), (x, u))


def test_general_kind_stride2(conv):
    x, w, b = _leaves(3, (2, 3, 5, 6), (4, 3, 3, 3), (4,))
    f = lambda x, w, b: conv.conv2d_general(x, w, b, stride=2, padding=1)  # noqa: E731
    assert torch.allclose(f(x, w, b), F.conv2d(x, w, b, stride=2, padding=1), rtol=0, atol=1e-12)
    _check(f, (x, w, b))


@pytest.mark.parametrize("cout_g,k,pad,groups", [(3, 2, 0, 1), (2, 2, 0, 2), (1, 4, 1, 2)])
def test_general_kind_conv_transpose(conv, cout_g, k, pad, groups):
    u, w, b = _leaves(4 + groups + k, (2, 4, 5, 6), (4, cout_g, k, k), (cout_g * groups,))
    f = lambda u, w, b: conv.conv_transpose2d_general(  # noqa: E731
        u, w, b, stride=2, padding=pad, groups=groups)
    ref = F.conv_transpose2d(u, w, b, stride=2, padding=pad, groups=groups)
    assert torch.allclose(f(u, w, b), ref, rtol=0, atol=1e-12)
    _check(f, (u, w, b))
