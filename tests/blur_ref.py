"""Float64 numpy restatement of the blur measurement operator A = D G Sym and of A^T
(helper module of test_blur_host.py / test_gpu_blur.py; definition: DESIGN.md section 4).

forward : numpy.pad(mode='symmetric') by p = K // 2, the 'same' convolution with g per axis
          ((G x)[r] = sum_k g[k] xs[r + p - k]), then the samples [o::s], o = (s - 1) // 2.
adjoint : written independently in gather form, per axis: the zero-upsampled y correlated
          with g on the extended axis [-p, n + p), then each pixel m collects its pre-images
          under the symmetric map: m, -1 - m (m < p) and 2 n - 1 - m (m >= n - p).
Both act on the last two axes of an array of any leading shape.
"""
import numpy as np


def taps(std, K):
    """g_i = exp(-(i - K // 2)^2 / (2 std)), normalised (std is a variance)."""
    i = np.arange(K, dtype=np.float64) - K // 2
    g = np.exp(-i * i / (2.0 * std))
    return g / g.sum()


def out_size(n, s):
    o = (s - 1) // 2
    return -((o - n) // s)


def _forward_axis(x, g, s, axis):
    x = np.moveaxis(np.asarray(x, np.float64), axis, -1)
    K, n = len(g), x.shape[-1]
    p = K // 2
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(p, p)], mode="symmetric")
    out = np.zeros_like(x)
    for k in range(K):
        out += g[k] * xp[..., 2 * p - k:2 * p - k + n]
    return np.moveaxis(out[..., (s - 1) // 2::s], -1, axis)


def _adjoint_axis(y, g, s, n, axis):
    y = np.moveaxis(np.asarray(y, np.float64), axis, -1)
    K = len(g)
    p, o = K // 2, (s - 1) // 2
    assert y.shape[-1] == out_size(n, s)
    up = np.zeros(y.shape[:-1] + (n + 4 * p,))
    up[..., 2 * p + o:2 * p + n:s] = y                    # u on [-2p, n + 2p)
    w = np.zeros(y.shape[:-1] + (n + 2 * p,))             # w on [-p, n + p)
    for k in range(K):
        w += g[k] * up[..., k:k + n + 2 * p]
    out = w[..., p:p + n].copy()
    if p:
        out[..., :p] += w[..., :p][..., ::-1]             # -1 - m for m < p
        out[..., n - p:] += w[..., n + p:][..., ::-1]     # 2 n - 1 - m for m >= n - p
    return np.moveaxis(out, -1, axis)


def forward(x, g, s=1):
    g = np.asarray(g, np.float64)
    return _forward_axis(_forward_axis(x, g, s, -2), g, s, -1)


def adjoint(y, g, s, size):
    g = np.asarray(g, np.float64)
    return _adjoint_axis(_adjoint_axis(y, g, s, size[1], -1), g, s, size[0], -2)
