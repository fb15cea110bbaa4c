"""NumPy restatement of the LETKF analysis of include/bpk.h, section "letkf" (Hunt, Kostelich &
Szunyogh 2007, identity observation), in two forms:

  analysis(..., dtype=np.float64, solver="eigh")    the truth: float64, np.linalg.eigh
  analysis(..., dtype=np.float32, solver="jacobi")  the yardstick for what float32 arithmetic
                                                    costs: every operation in float32, the
                                                    eigenproblem by an explicit cyclic Jacobi

    A    = (m-1)/inflation I + sum_j rho_j dX_j dX_j^T,   g = sum_j rho_j dX_j (obs_j - xbar_j)
    A    = Q L Q^T,   wbar = Q L^-1 Q^T g,   Wa = sqrt(m-1) Q L^-1/2 Q^T
    out[i, c, y0, x0] = xbar_c + sum_k dX_k[c, y0, x0] (wbar_k + Wa[k, i])

over the window |y - y0| <= R, |x - x0| <= R clipped at the domain edge, rho_j = taper * prec_j,
entries with rho_j == 0 skipped (obs may be NaN there).  The reference project has no ensemble
filter; nothing here is derived from it.
"""
import numpy as np

SWEEP_CAP = 16


def round_robin(t, n):
    """The n / 2 disjoint pairs (p < q) of round t (0 <= t < n - 1) of the round-robin
    tournament of n players (n even): player n - 1 stays, the others rotate."""
    n1 = n - 1
    i = np.arange(n // 2)
    a, b = (t + i) % n1, (t - i) % n1
    a[0] = n1
    return np.minimum(a, b), np.maximum(a, b)


def jacobi_eigh(A, cap=SWEEP_CAP):
    """Two-sided cyclic Jacobi on a batch A [N, m, m] of symmetric matrices, in A's dtype.
    A rotation is skipped when |a_pq| <= u sqrt(a_pp a_qq), u the unit roundoff of the dtype;
    the iteration ends after the first sweep that rotates nothing, or at `cap` sweeps.  The rotations of a round (disjoint pairs) are applied together: A J, then J^T A.
    -> (lam [N, m], Q [N, m, m], sweeps [N] (sweeps that rotated), capped [N] bool)."""
    dt = A.dtype
    u = float(np.finfo(dt).eps) / 2
    N, m, _ = A.shape
    n = m + (m & 1)
    W = np.zeros((n, n, N), dt)  # batch index last: row and column gathers are block copies
    W[:m, :m] = A.transpose(1, 2, 0)
    if n != m:
        W[m, m] = 1  # a decoupled bye player: its rotations are all skipped
    Q = np.zeros((n, n, N), dt)
    Q[np.arange(n), np.arange(n)] = 1
    sweeps = np.zeros(N, np.int64)
    capped = np.zeros(N, bool)
    one, half = dt.type(1), dt.type(0.5)
    for sweep in range(cap):
        rotated = np.zeros(N, bool)
        for t in range(n - 1):
            P, K = round_robin(t, n)
            app, aqq, apq = W[P, P], W[K, K], W[K, P]  # [n / 2, N]
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                skip = np.abs(apq) <= dt.type(u) * np.sqrt(np.abs(app * aqq))
                theta = (aqq - app) / (2 * np.where(skip, one, apq))
                at = np.abs(theta)
                big = at > 1e9  # sqrt(theta^2 + 1) == |theta| long before theta^2 overflows
                at_s = np.where(big, one, at)
                tt = np.where(big, half / np.where(big, at, one),
                              one / (at_s + np.sqrt(at_s * at_s + one)))
                tt = np.copysign(tt, theta)
                c = one / np.sqrt(tt * tt + one)
                s = tt * c
            c = np.where(skip, one, c).astype(dt)
            s = np.where(skip, 0, s).astype(dt)
            did = s != 0
            rotated |= did.any(0)
            for M in (W, Q):  # M J
                mp, mk = M[:, P], M[:, K]  # copies (fancy index)
                M[:, P], M[:, K] = c * mp - s * mk, s * mp + c * mk
            wp, wk = W[P], W[K]  # J^T W
            W[P], W[K] = c[:, None] * wp - s[:, None] * wk, s[:, None] * wp + c[:, None] * wk
            W[P, K] = np.where(did, 0, W[P, K])
            W[K, P] = np.where(did, 0, W[K, P])
        sweeps += rotated
        capped = rotated if sweep == cap - 1 else capped
        if not rotated.any():
            break
    assert W.dtype == dt and Q.dtype == dt
    lam = W[np.arange(m), np.arange(m)].T.copy()
    return lam, Q[:m, :m].transpose(2, 0, 1).copy(), sweeps, capped


def system(ens, obs, prec, taper, inflation, dtype):
    """-> xbar [B, C, H, W], dX [B, m, C, H, W], A [B, H, W, m, m], g [B, H, W, m]."""
    dt = np.dtype(dtype)
    ens, prec, taper = (np.asarray(v, dt) for v in (ens, prec, taper))
    obs = np.asarray(obs, dt)
    B, m, C, H, W = ens.shape
    R = taper.shape[0] // 2
    assert taper.shape == (2 * R + 1, 2 * R + 1) and obs.shape == prec.shape == (B, C, H, W)
    xbar = (ens.sum(1, dtype=dt) / dt.type(m)).astype(dt)
    dX = ens - xbar[:, None]
    A = np.zeros((B, H, W, m, m), dt)
    g = np.zeros((B, H, W, m), dt)
    A[..., np.arange(m), np.arange(m)] = dt.type(m - 1) / dt.type(inflation)
    with np.errstate(invalid="ignore"):
        innov = obs - xbar
    for dy in range(-R, R + 1):
        ys = slice(max(0, -dy), min(H, H - dy))           # centres y0
        yw = slice(max(0, -dy) + dy, min(H, H - dy) + dy)  # window rows y = y0 + dy
        if ys.start >= ys.stop:
            continue
        for dx in range(-R, R + 1):
            xs = slice(max(0, -dx), min(W, W - dx))
            xw = slice(max(0, -dx) + dx, min(W, W - dx) + dx)
            if xs.start >= xs.stop or taper[dy + R, dx + R] == 0:
                continue
            rho = taper[dy + R, dx + R] * prec[:, :, yw, xw]           # [B, C, h, w]
            d = dX[:, :, :, yw, xw]                                    # [B, m, C, h, w]
            v = np.where(rho != 0, innov[:, :, yw, xw], 0).astype(dt)  # skipped, not multiplied
            A[:, ys, xs] += np.einsum("bkcyx,bcyx,blcyx->byxkl", d, rho, d).astype(dt)
            g[:, ys, xs] += np.einsum("bkcyx,bcyx->byxk", d, rho * v).astype(dt)
    assert A.dtype == dt and g.dtype == dt
    return xbar, dX, A, g


def analysis(ens, obs, prec, taper, inflation=1.0, dtype=np.float64, solver="eigh",
             return_sweeps=False):
    """-> (ens_out [B, m, C, H, W] in `dtype`, status int32 [B, H, W]) (and the Jacobi sweep
    counts [B, H, W] with return_sweeps).  status / fall-back as the kernel's contract: 1 where
    the Jacobi iteration was capped or the result is not finite, and the output there is
    xbar + sqrt(inflation) dX."""
    dt = np.dtype(dtype)
    xbar, dX, A, g = system(ens, obs, prec, taper, inflation, dt)
    B, m, C, H, W = dX.shape
    flat = A.reshape(-1, m, m)
    if solver == "eigh":
        lam, Q = np.linalg.eigh(flat)
        sweeps, capped = np.zeros(len(flat), np.int64), np.zeros(len(flat), bool)
    elif solver == "jacobi":
        lam, Q, sweeps, capped = jacobi_eigh(flat)
    else:
        raise ValueError(solver)
    lam, Q = lam.astype(dt).reshape(B, H, W, m), Q.astype(dt).reshape(B, H, W, m, m)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.einsum("byxkl,byxk->byxl", Q, g) / lam
        wbar = np.einsum("byxkl,byxl->byxk", Q, z)
        Wa = np.einsum("byxkl,byxl,byxil->byxki", Q, np.sqrt(dt.type(m - 1)) / np.sqrt(lam), Q)
        T = (wbar[..., None] + Wa).astype(dt)
        out = xbar[:, None] + np.einsum("bkcyx,byxki->bicyx", dX, T)
    out = out.astype(dt)
    status = capped.reshape(B, H, W) | ~np.isfinite(out).all(axis=(1, 2))
    fallback = xbar[:, None] + np.sqrt(dt.type(inflation)) * dX
    out = np.where(status[:, None, None], fallback, out).astype(dt)
    if return_sweeps:
        return out, status.astype(np.int32), sweeps.reshape(B, H, W)
    return out, status.astype(np.int32)


def truth(ens, obs, prec, taper, inflation=1.0):
    return analysis(ens, obs, prec, taper, inflation, np.float64, "eigh")


def ref32(ens, obs, prec, taper, inflation=1.0, return_sweeps=False):
    return analysis(ens, obs, prec, taper, inflation, np.float32, "jacobi", return_sweeps)


def kalman_update(ens, obs, prec):
    """The textbook update of one sample's whole state with the ensemble's sample covariance
    (float64): ens [m, n], obs / prec [n] (prec 0 = unobserved) -> (mean [n], cov [n, n]) with
    mean = xbar + K (y - H xbar), cov = (I - K H) Pb, Pb = dX dX^T / (m - 1),
    K = Pb H^T (H Pb H^T + R)^-1, H the rows of the identity at the observed entries."""
    ens = np.asarray(ens, np.float64)
    m, n = ens.shape
    xbar = ens.mean(0)
    dX = ens - xbar
    Pb = dX.T @ dX / (m - 1)
    sel = np.flatnonzero(np.asarray(prec) != 0)
    Hm = np.eye(n)[sel]
    Rm = np.diag(1.0 / np.asarray(prec, np.float64)[sel])
    K = Pb @ Hm.T @ np.linalg.inv(Hm @ Pb @ Hm.T + Rm)
    mean = xbar + K @ (np.asarray(obs, np.float64)[sel] - Hm @ xbar)
    return mean, (np.eye(n) - K @ Hm) @ Pb
