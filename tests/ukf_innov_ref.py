"""Numpy restatement of the innovation statistics of op.ukf.innovation and of the evidence of a
linear-Gaussian Kalman filter (helper, not a test).  dtype-generic: float64 is the truth,
float32 is what plain float32 arithmetic achieves on the same recursion.  The reference has no
counterpart (it delegates to torchfilter, which reports no such statistic); the truth is the
Gaussian density in closed form.
"""
import math

import numpy as np

LOG_2PI = math.log(2 * math.pi)


def solve_lower(S, r):
    """Forward substitution on the lower triangle of S [N, d, d], row by row (dot-product
    order: not the order of the kernel's column sweep): e with tril(S) e = r [N, d]."""
    S = np.tril(S)
    e = np.zeros_like(r)
    for i in range(r.shape[1]):
        e[:, i] = (r[:, i] - np.einsum('nc,nc->n', S[:, i, :i], e[:, :i])) / S[:, i, i]
    return e


def innovation(z_mean, z_tril, obs, dtype=np.float64):
    """-> (white [N, dz], nis [N], loglik [N], status int32 [N]): e = S_z^-1 (obs - z_mean),
    nis = e^T e, loglik = -0.5 (nis + 2 sum_i log S_z[i,i] + dz log(2 pi)); status 1 and NaN
    outputs where a diagonal entry of z_tril is not > 0 or not finite."""
    zm, S, z = (np.asarray(a, dtype) for a in (z_mean, z_tril, obs))
    N, dz = zm.shape
    diag = np.diagonal(S, axis1=1, axis2=2)
    bad = ~((diag > 0) & np.isfinite(diag)).all(1)
    Sg = np.where(bad[:, None, None], np.eye(dz, dtype=dtype), S)
    e = solve_lower(Sg, z - zm)
    nis = (e * e).sum(1)
    loglik = -0.5 * (nis + 2 * np.log(np.diagonal(Sg, axis1=1, axis2=2)).sum(1) + dz * LOG_2PI)
    nan = np.asarray(np.nan, dtype)
    return (np.where(bad[:, None], nan, e), np.where(bad, nan, nis), np.where(bad, nan, loglik),
            bad.astype(np.int32))


def kappa_inf(S):
    """inf-norm condition number of each lower factor tril(S) [N, d, d], in float64."""
    S = np.tril(np.asarray(S, np.float64))
    inv = np.linalg.inv(S)
    return np.abs(S).sum(2).max(1) * np.abs(inv).sum(2).max(1)


def kalman_evidence(F, H, Q, R, m0, P0, zs, dtype=np.float64):
    """The exact Kalman filter of x+ = F x + q, z = H x + r (q ~ N(0, Q), r ~ N(0, R)) for N
    filters sharing the model: m0 [N, n], P0 [n, n], zs [T, N, dz] ->
    (logliks [T, N], nis [T, N], means [T, N, n]) with logliks[t] = log N(z_t; H m-, H P- H^T + R),
    the evidence of step t."""
    F, H, Q, R, m, P, zs = (np.asarray(a, dtype) for a in (F, H, Q, R, m0, P0, zs))
    dz = H.shape[0]
    lls, nis, means = [], [], []
    for z in zs:
        m = m @ F.T
        P = F @ P @ F.T + Q
        Sz = H @ P @ H.T + R
        r = z - m @ H.T
        w = np.linalg.solve(Sz, r.T).T  # S^-1 r
        q = (r * w).sum(1)
        lls.append(-0.5 * (q + np.linalg.slogdet(Sz)[1] + dz * LOG_2PI))
        nis.append(q)
        Kg = np.linalg.solve(Sz, H @ P).T  # P H^T S^-1 (S, P symmetric)
        m = m + r @ Kg.T
        P = P - Kg @ Sz @ Kg.T
        P = 0.5 * (P + P.T)
        means.append(m)
    return np.stack(lls), np.stack(nis), np.stack(means)
