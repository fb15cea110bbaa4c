"""CPU restatement of the unscented Rauch-Tung-Striebel smoother step of op/ukf.py
(`rts_smooth`; helper, not a test), on the pieces of tests/ukf_ref.py: dtype-generic (float64 =
truth, float32 = what plain float32 arithmetic achieves), vectorised over N filters, library
triangular solves.  Anchored to the closed-form RTS recursion in test_urts_host.py.

One step t+1 -> t, with (m, S) the posterior at t, X its sigma points, Y = f(X), (mp, Sp) the
prediction at t+1 and (ms1, Ss1) the smoothed belief at t+1:

  C = sum_s wc_s (X_s - m)(Y_s - mp)^T,  U = C Sp^-T  (G = U Sp^-1),
  ms = m + U Sp^-1 (ms1 - mp),  W = U Sp^-1 Ss1,
  Ss = S after n rank-1 updates by W's columns, then n rank-1 downdates by U's columns
  (P^s = P + G P^s_+ G^T - G P- G^T; updates first, so every intermediate dominates P^s).
"""
import torch

import ukf_ref


def smooth(m, S, X, Y, mp, Sp, ms1, Ss1, wc0, wi, groups=1):
    """-> (ms, Ss, flag, dict(C, U, W))."""
    N, n = m.shape
    idx = ukf_ref.rows(N, n, groups)
    wc = torch.full((2 * n + 1,), wi, dtype=m.dtype)
    wc[0] = wc0
    C = torch.einsum('s,nsi,nsj->nij', wc, X[idx] - m.unsqueeze(1), Y[idx] - mp.unsqueeze(1))
    U = torch.linalg.solve_triangular(Sp, C.transpose(1, 2), upper=False).transpose(1, 2)
    y = torch.linalg.solve_triangular(Sp, (ms1 - mp).unsqueeze(2), upper=False)
    ms = m + (U @ y).squeeze(2)
    W = U @ torch.linalg.solve_triangular(Sp, Ss1, upper=False)
    S1, flag = S, torch.zeros(N, dtype=torch.bool)
    for c in range(n):
        S1, f = ukf_ref.rank1(S1, W[:, :, c], +1)
        flag |= f
    for c in range(n):
        S1, f = ukf_ref.rank1(S1, U[:, :, c], -1)
        flag |= f
    return ms, S1, flag, dict(C=C, U=U, W=W)


def chain(m, S, dyn, meas, zs, abk=(1., 0., 0.), groups=1):
    """len(zs) steps of `ukf_ref.step`, then the smoother back to index 0.  -> (means_s,
    trils_s, flag, steps): lists of length T + 1 (index T is the filtered posterior), the OR of
    every flag, and the forward steps' intermediates."""
    n = m.shape[1]
    _, _, wc0, wi = ukf_ref.merwe(n, *abk)
    steps, means, trils = [], [m], [S]
    flag = torch.zeros(m.shape[0], dtype=torch.bool)
    for z in zs:
        o = ukf_ref.step(means[-1], trils[-1], dyn, meas, z, abk, groups)
        flag = flag | o["flag"]
        steps.append(o)
        means.append(o["m_post"])
        trils.append(o["S_post"])
    T = len(steps)
    ms, Ss = [None] * (T + 1), [None] * (T + 1)
    ms[T], Ss[T] = means[T], trils[T]
    for t in range(T - 1, -1, -1):
        o = steps[t]
        ms[t], Ss[t], f, _ = smooth(means[t], trils[t], o["X"], o["Y"], o["m_pred"], o["S_pred"],
                                    ms[t + 1], Ss[t + 1], wc0, wi, groups)
        flag = flag | f
    return ms, Ss, flag, steps
