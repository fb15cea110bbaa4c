"""`op.blur` -- separable blur + decimation and its adjoint on HIP (csrc/blur.hip).

The blurred / low-resolution measurement operator of the inverse samplers.  For
x [B, C, H, W], K taps g (K odd, p = K // 2) and a stride s >= 1:

    G x = scipy.signal.convolve2d(x, outer(g, g), boundary='symm', mode='same')  per plane
    y[i, j] = (G x)[s i + o, s j + o],  o = (s - 1) // 2,  Ho = ceil((H - o) / s)

`blur2d` is A = D G Sym, `blur2d_adjoint` is A^T in gather form (no atomics, bitwise
reproducible).  Both are linear and each one's backward is the other, so the pair is
differentiable to any order.  float32 and float64; no CPU path.

`gaussian_taps(std, K)` restates the taps of the reference's GaussianFilter.get_kernel
(inverse/operators.py:79-90): that kernel is the pdf of N(0, std * I) on the integer grid,
normalised -- `std` is passed as the covariance, i.e. it is a VARIANCE -- and separates
exactly into outer(g, g) with g_i = exp(-(i - p)^2 / (2 std)) / sum.
"""
from __future__ import annotations

import ctypes
import math

import torch

from ._lib import check, lib, require_hip, stream_ptr

# the kernel's tile (csrc/blur.hip: BLUR_TH, BLUR_TW) and tap limit (BLUR_KMAX)
TILE_H = 16
TILE_W = 64
MAX_TAPS = 33


def gaussian_taps(std, K):
    """K float64 taps g_i = exp(-(i - K // 2)^2 / (2 std)), normalised to sum 1 (a CPU tensor).
    `std` is the variance of the Gaussian, as in the reference."""
    K = int(K)
    if K < 1 or K % 2 == 0 or K > MAX_TAPS:
        raise ValueError(f"blur: tap count must be odd, 1 <= K <= {MAX_TAPS} (got {K})")
    if not float(std) > 0:
        raise ValueError(f"blur: std must be positive (got {std})")
    p = K // 2
    g = [math.exp(-((i - p) ** 2) / (2.0 * float(std))) for i in range(K)]
    tot = math.fsum(g)
    return torch.tensor([v / tot for v in g], dtype=torch.float64)


def _taps_tuple(taps):
    if isinstance(taps, torch.Tensor):
        taps = taps.detach().cpu().reshape(-1).tolist()
    return tuple(float(v) for v in taps)


def out_size(H, W, K, stride=1):
    """(Ho, Wo) of blur2d on an H x W plane; ValueError for arguments the op does not take."""
    K, stride = int(K), int(stride)
    if K < 1 or K % 2 == 0 or K > MAX_TAPS:
        raise ValueError(f"blur: tap count must be odd, 1 <= K <= {MAX_TAPS} (got {K})")
    if stride < 1:
        raise ValueError(f"blur: stride >= 1 required (got {stride})")
    if H < 1 or W < 1 or K // 2 > min(H, W):
        raise ValueError(f"blur: halo K // 2 = {K // 2} exceeds min(H, W) = {min(H, W)}")
    o = (stride - 1) // 2
    if o >= min(H, W):
        raise ValueError(f"blur: stride {stride} leaves no sample in a {H} x {W} plane")
    return -((o - H) // stride), -((o - W) // stride)


_ENTRY = {
    (torch.float32, False): "bpk_blur2d_f32", (torch.float64, False): "bpk_blur2d_f64",
    (torch.float32, True): "bpk_blur2d_adjoint_f32", (torch.float64, True): "bpk_blur2d_adjoint_f64",
}


def _run(t, taps, stride, size, adjoint):
    what = "blur.blur2d_adjoint" if adjoint else "blur.blur2d"
    if t.ndim != 4:
        raise ValueError(f"{what}: expected a [B, C, H, W] tensor, got {tuple(t.shape)}")
    H, W = (int(size[0]), int(size[1])) if adjoint else (t.shape[2], t.shape[3])
    Ho, Wo = out_size(H, W, len(taps), stride)
    if adjoint and tuple(t.shape[2:]) != (Ho, Wo):
        raise ValueError(f"{what}: y is {tuple(t.shape[2:])}, size {(H, W)} at stride {stride} "
                         f"needs {(Ho, Wo)}")
    require_hip(t, what=what)
    if t.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"{what}: float32 or float64 tensors required, got {t.dtype}")
    t = t.contiguous()
    B, C = t.shape[:2]
    out = torch.empty((B, C, H, W) if adjoint else (B, C, Ho, Wo), device=t.device, dtype=t.dtype)
    g = (ctypes.c_double * len(taps))(*taps)
    check(getattr(lib, _ENTRY[t.dtype, adjoint])(t.data_ptr(), out.data_ptr(), B * C, H, W, g,
                                                 len(taps), int(stride), stream_ptr(t.device)),
          what)
    return out


class _Blur2d(torch.autograd.Function):
    """y = A x; linear, so the backward is the adjoint kernel, whose own backward is this."""

    @staticmethod
    def forward(ctx, x, taps, stride):
        ctx.taps, ctx.stride, ctx.size = taps, stride, tuple(x.shape[2:])
        return _run(x, taps, stride, None, False)

    @staticmethod
    def backward(ctx, gy):
        return _Blur2dAdjoint.apply(gy, ctx.taps, ctx.stride, ctx.size), None, None


class _Blur2dAdjoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, taps, stride, size):
        ctx.taps, ctx.stride = taps, stride
        return _run(y, taps, stride, size, True)

    @staticmethod
    def backward(ctx, gx):
        return _Blur2d.apply(gx, ctx.taps, ctx.stride), None, None, None


def blur2d(x, taps, stride=1):
    """A x: [B, C, H, W] -> [B, C, Ho, Wo].  `taps`: K host values (sequence or CPU tensor)."""
    return _Blur2d.apply(x, _taps_tuple(taps), int(stride))


def blur2d_adjoint(y, taps, stride, size):
    """A^T y: [B, C, Ho, Wo] -> [B, C, *size], size = (H, W) of the input side."""
    return _Blur2dAdjoint.apply(y, _taps_tuple(taps), int(stride), (int(size[0]), int(size[1])))
