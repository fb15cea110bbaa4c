"""The PINN nets' spatial embedding as plain torch (helper, not a test): the reference
expression of models/layers.py:517-521,

    e = (sin(w sqrt(x^2 + y^2)) + sin(w sqrt((mx - x)^2 + (my - y)^2))) / s,

mx, my the maxima of x, y over one copy of a batch of k stacked copies, and its derivatives
taken by autograd in the residual's pattern.  Dtype- and device-generic: float64 = truth,
float32 = what the reference's own op chain achieves.  Nothing here knows the closed forms of
csrc/pinn_emb.hip, and nothing imports op.embedding -- this is the yardstick, not the product.
"""
import functools

import torch

OMEGAS = ((3.0, 2.5), (100.0, 100.0))  # (omega, s): a mild pair and the shipped configuration


def copy_max(v, k):
    """[k, 1, ..., 1] maxima of the k stacked copies of v [k * cb, ...] (ties share the gradient
    evenly, as max() over one batch does)."""
    g = v.reshape((k, v.shape[0] // k) + tuple(v.shape[1:]))
    return g.reshape(k, -1).amax(1).view((k,) + (1,) * (g.dim() - 1))


def forward(x, y, k, omega, s):
    """The embedding in the dtype of x, y, in the reference's operation order."""
    def max_minus(v):
        if k == 1:
            return v.max() - v
        # one view of v feeding both the maximum and the difference: autograd then sums the
        # two gradient paths in the reference's order (bit-identical second derivatives)
        g = v.reshape((k, v.shape[0] // k) + tuple(v.shape[1:]))
        m = g.reshape(k, -1).amax(1).view((k,) + (1,) * (g.dim() - 1))
        return (m - g).reshape(v.shape)
    e1 = torch.sin(omega * torch.sqrt(x ** 2 + y ** 2))
    e2 = torch.sin(omega * torch.sqrt(max_minus(x) ** 2 + max_minus(y) ** 2))
    return (e1 + e2) / s


def chain(x, y, W, a, b, k, omega, s):
    """(e, gx, gy, d2x, d2y, dW): the embedding, its first derivatives w.r.t. x, y under an
    upstream weight W (create_graph), and the derivatives of sum(gx a + gy b) w.r.t. x, y, W --
    the residual's derivative pattern -- all by autograd, in the dtype of the inputs.
    b = None: the second pass differentiates sum(gx a) alone."""
    x, y, W = (v.detach().clone().requires_grad_() for v in (x, y, W))
    e = forward(x, y, k, omega, s)
    gx, gy = torch.autograd.grad((e * W).sum(), (x, y), create_graph=True)
    l2 = (gx * a).sum() if b is None else (gx * a + gy * b).sum()
    d2x, d2y, dW = torch.autograd.grad(l2, (x, y, W))
    return tuple(t.detach() for t in (e, gx, gy, d2x, d2y, dW))


def truth(x, y, W, a, b, k, omega, s):
    """chain in float64 on the CPU."""
    return chain(*(None if v is None else v.detach().double().cpu() for v in (x, y, W, a, b)),
                 k, omega, s)


def argmax_mask(x, y, k):
    """Elements holding their copy's x or y maximum (the sets the max's gradient lands on)."""
    def one(v):
        g = v.reshape((k, v.shape[0] // k) + tuple(v.shape[1:]))
        return (g == copy_max(v, k)).reshape(v.shape)
    return one(x) | one(y)


@functools.lru_cache(maxsize=None)
def inputs(k, cb, h, w, seed, mode="jitter"):
    """float32 CPU (x, y, W, a, b), each [k * cb, 1, h, w] (cached: read only).  x, y are
    linspace(0.05, 1) coordinate meshes + 0.01 rand jitter, copy c scaled by 1 + 0.25 c so that
    the copies' maxima differ grossly.  mode "column_ties": the x mesh is exact, so the whole
    last column of every sample of a copy ties for mx (y stays jittered); the y maximum of
    each copy is then planted at (first sample, last row, column 0), away from the tied column
    -- an element holding both maxima has r2 = 0 and every derivative there is NaN, in the
    reference as well."""
    assert mode in ("jitter", "column_ties")
    g = torch.Generator().manual_seed(seed)
    B = k * cb
    jx = 0.01 * torch.rand(B, 1, h, w, generator=g)
    jy = 0.01 * torch.rand(B, 1, h, w, generator=g)
    x = torch.linspace(0.05, 1.0, w).view(1, 1, 1, w) + (jx if mode == "jitter" else 0.0 * jx)
    y = torch.linspace(0.05, 1.0, h).view(1, 1, h, 1) + jy
    scale = (1.0 + 0.25 * torch.arange(k, dtype=torch.float32)).repeat_interleave(cb)
    x = (x * scale.view(B, 1, 1, 1)).contiguous()
    y = (y * scale.view(B, 1, 1, 1)).contiguous()
    if mode == "column_ties":
        for c in range(k):
            y[c * cb, 0, h - 1, 0] = y[c * cb:(c + 1) * cb].max() + 0.01
    W, a, b = (torch.randn(B, 1, h, w, generator=g) for _ in range(3))
    for omega, s in OMEGAS:
        assert all(torch.isfinite(t).all() for t in truth(x, y, W, a, b, k, omega, s)), \
            f"inputs{(k, cb, h, w, seed, mode)}: the float64 truth is not finite"
    return x, y, W, a, b
