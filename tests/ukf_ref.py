"""CPU restatement of the square-root UKF of op/ukf.py (helper, not a test): the mathematics
of Van der Merwe & Wan (2001) with Merwe scaled sigma points, written with torch on the CPU,
dtype-generic (float64 = truth, float32 = what plain float32 arithmetic achieves), vectorised
over N filters.  Library QR and triangular solves are fine here -- this is the yardstick, not the
product.  Model callbacks map points [rows, dim] -> (points [rows, dim'], noise factor
[N, dim', dim']); every function returns a per-filter "not positive definite" flag.
"""
import functools
import math

import torch

EPS32 = float(torch.finfo(torch.float32).eps)


def merwe(n, alpha=1., beta=0., kappa=0.):
    lam = alpha * alpha * (n + kappa) - n
    wm0 = lam / (n + lam)
    return math.sqrt(n + lam), wm0, wm0 + 1 - alpha * alpha + beta, 1 / (2 * (n + lam))


@functools.lru_cache(maxsize=None)
def rows(N, n, groups=1):
    """[N, 2n+1] row of (filter i, sigma point s) in the (g, s, r) order, by the definition:
    i = g * (N / groups) + r -> ((g * (2n+1)) + s) * (N / groups) + r.  (Cached: read only.)"""
    ng = N // groups
    return torch.tensor([[((i // ng) * (2 * n + 1) + s) * ng + i % ng for s in range(2 * n + 1)]
                         for i in range(N)], dtype=torch.long)


def sigma(m, S, gamma, groups=1):
    N, n = m.shape
    pts = torch.cat([m.unsqueeze(1), m.unsqueeze(1) + (gamma * S).transpose(1, 2),
                     m.unsqueeze(1) - (gamma * S).transpose(1, 2)], 1)  # [N, 2n+1, n]
    out = torch.empty((2 * n + 1) * N, n, dtype=m.dtype)
    out[rows(N, n, groups).reshape(-1)] = pts.reshape(-1, n)
    return out


def rank1(S, x, sign):
    """Rank-1 update (sign = +1) / downdate (-1) of lower factors S [N, n, n] by x [N, n].
    Where a downdate meets S_kk^2 - x_k^2 <= 0 (or NaN): S_kk := eps_f32 |S_kk|, the column
    below stays, the rest of x is dropped, and the filter is flagged."""
    S, x = S.clone(), x.clone()
    N, n = x.shape
    flag = torch.zeros(N, dtype=torch.bool)
    for k in range(n):
        skk, xk = S[:, k, k].clone(), x[:, k].clone()
        r2 = skk * skk + sign * xk * xk
        bad = ~(r2 > 0) if sign < 0 else torch.zeros(N, dtype=torch.bool)
        r = torch.sqrt(torch.where(bad, torch.ones_like(r2), r2))
        c, s = (r / skk).unsqueeze(1), (xk / skk).unsqueeze(1)
        col = (S[:, k + 1:, k] + sign * s * x[:, k + 1:]) / c
        xn = c * x[:, k + 1:] - s * col
        S[:, k, k] = torch.where(bad, EPS32 * skk.abs(), r)
        S[:, k + 1:, k] = torch.where(bad.unsqueeze(1), S[:, k + 1:, k], col)
        x[:, k + 1:] = torch.where(bad.unsqueeze(1), torch.zeros_like(xn), xn)
        flag |= bad
    return S, flag


def root(pts, noise, n, wm0, wc0, wi, groups=1):
    """-> (mean [N, d], S [N, d, d], flag [N]) with S S^T = sum_s wc_s D_s D_s^T + R R^T."""
    N = noise.shape[0]
    Y = pts[rows(N, n, groups)]  # [N, 2n+1, d]
    mean = wm0 * Y[:, 0] + wi * Y[:, 1:].sum(1)
    D = Y - mean.unsqueeze(1)
    A = torch.cat([math.sqrt(wi) * D[:, 1:], noise.tril().transpose(1, 2)], 1)
    R = torch.linalg.qr(A, mode='r').R
    sgn = torch.where(torch.diagonal(R, dim1=1, dim2=2) < 0, -1., 1.).to(pts.dtype)
    S = (R.transpose(1, 2) * sgn.unsqueeze(1)).tril()
    flag = torch.zeros(N, dtype=torch.bool)
    if wc0 != 0:
        S, flag = rank1(S, math.sqrt(abs(wc0)) * D[:, 0], 1 if wc0 > 0 else -1)
    return mean, S, flag


def update(m, S, xp, zp, zhat, Sz, z, wc0, wi, groups=1):
    """-> (m+, S+, flag, dict(P_xz, K, U))."""
    N, n = m.shape
    idx = rows(N, n, groups)
    X, Z = xp[idx], zp[idx]
    wc = torch.full((2 * n + 1,), wi, dtype=m.dtype)
    wc[0] = wc0
    Pxz = torch.einsum('s,nsi,nsj->nij', wc, X - m.unsqueeze(1), Z - zhat.unsqueeze(1))
    T1 = torch.linalg.solve_triangular(Sz, Pxz.transpose(1, 2), upper=False)
    Kg = torch.linalg.solve_triangular(Sz.transpose(1, 2), T1, upper=True).transpose(1, 2)
    m1 = m + (Kg @ (z - zhat).unsqueeze(2)).squeeze(2)
    U = Kg @ Sz
    flag = torch.zeros(N, dtype=torch.bool)
    S1 = S
    for c in range(U.shape[2]):
        S1, f = rank1(S1, U[:, :, c], -1)
        flag |= f
    return m1, S1, flag, dict(P_xz=Pxz, K=Kg, U=U)


def step(m, S, dyn, meas, z, abk=(1., 0., 0.), groups=1):
    """One predict + update; returns every intermediate."""
    n = m.shape[1]
    gamma, wm0, wc0, wi = merwe(n, *abk)
    X = sigma(m, S, gamma, groups)
    Y, Q = dyn(X)
    m_pred, S_pred, f1 = root(Y, Q, n, wm0, wc0, wi, groups)
    X2 = sigma(m_pred, S_pred, gamma, groups)
    Z, R = meas(X2)
    z_mean, z_tril, f2 = root(Z, R, n, wm0, wc0, wi, groups)
    m_post, S_post, f3, extra = update(m_pred, S_pred, X2, Z, z_mean, z_tril, z, wc0, wi, groups)
    return dict(X=X, Y=Y, Q=Q, m_pred=m_pred, S_pred=S_pred, X2=X2, Z=Z, R=R, z_mean=z_mean,
                z_tril=z_tril, m_post=m_post, S_post=S_post, flag=f1 | f2 | f3, **extra)
