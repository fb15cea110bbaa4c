"""GPU: the unscented Rauch-Tung-Striebel smoother -- the kernel behind op.ukf.rts_smooth
(csrc/ukf.hip), SquareRootUKF.filter / smooth, UKF.filter / smooth and the masked measurement
model -- against the CPU restatement tests/urts_ref.py (anchored to the closed-form RTS
recursion in test_urts_host.py).

Gate of every float comparison (the project's rule, as in test_gpu_ukf.py): with the float64
restatement fed the same float32 inputs as truth, err(kernel) <= max(1e-5, 2 x err(restatement
run in float32)); means relative to max|mean64|, factors compared as S S^T relative to
max|P64|.  Structure (exact zeros above the diagonal, a positive diagonal, status 0) is checked
separately and exactly."""
import functools

import numpy as np
import pytest
import torch

import ukf_ref
import urts_ref
from op import ukf as K
from test_gpu_ukf import TRIPLES, _cov, _gate, _models, _structure, _tril  # the gate and models

pytestmark = pytest.mark.gpu

STAGE_KEYS = ("m", "S", "X", "Y", "mp", "Sp", "ms1", "Ss1")


@functools.lru_cache(maxsize=None)
def _stage(n, abk, N=4, groups=2):
    """Float32 inputs of one backward stage (computed once, never modified): a float32 forward
    step of the restatement with the models, scales and seed formula of test_gpu_ukf._case
    gives the posterior at t (m, S), its points X, Y = f(X), the prediction at t+1 (mp, Sp)
    and the filtered posterior at t+1, which is the smoothed belief there (ms1, Ss1) when t+1
    is the last frame.  Neither restatement may flag a filter."""
    g = torch.Generator().manual_seed(1000 * n + 10 * n + int(2 * abk[0] + abk[2]))
    _, _, wc0, wi = ukf_ref.merwe(n, *abk)
    f, h = _models(n, n, g)
    m = 0.5 * torch.randn(N, n, generator=g)
    S, Q, R = _tril(N, n, g, 0.1, 0.3), _tril(N, n, g, 0.05, 0.05), _tril(N, n, g, 0.05, 0.2)
    z = 0.5 * torch.randn(N, n, generator=g)
    o = ukf_ref.step(m, S, lambda x: (f(x), Q), lambda x: (h(x), R), z, abk, groups)
    assert not o["flag"].any(), "restatement flagged a filter in the forward step"
    c = dict(n=n, N=N, groups=groups, w=(wc0, wi), m=m, S=S, X=o["X"], Y=o["Y"], mp=o["m_pred"],
             Sp=o["S_pred"], ms1=o["m_post"], Ss1=o["S_post"])
    args = [c[k] for k in STAGE_KEYS]
    c["s64"] = urts_ref.smooth(*(a.double() for a in args), wc0, wi, groups)
    c["s32"] = urts_ref.smooth(*args, wc0, wi, groups)
    assert not c["s64"][2].any() and not c["s32"][2].any(), "restatement flagged a filter"
    return c


@pytest.mark.parametrize("abk", TRIPLES)
@pytest.mark.parametrize("n,N,groups", [(4, 4, 2), (9, 4, 2), (16, 4, 2), (64, 4, 2), (16, 5, 1),
                                        (16, 12, 4)])
def test_rts_smooth_vs_float64(hip, n, N, groups, abk):
    """n below and off the 16-wide thread tiling, 2n+1 off the 32-point chunk, a full
    64-register row, an odd N, groups > 1 addressing."""
    c = _stage(n, abk, N, groups)
    wc0, wi = c["w"]
    mean, S, status = K.rts_smooth(*(c[k].to(hip) for k in STAGE_KEYS), wc0, wi, groups)
    assert mean.shape == (N, n) and S.shape == (N, n, n)
    _structure(S, status)
    what = f"ukf.smooth n={n} N={N} groups={groups} abk={abk}"
    _gate(what + " mean", mean, c["s64"][0], c["s32"][0])
    _gate(what + " cov", _cov(S), _cov(c["s64"][1]), _cov(c["s32"][1]))


@pytest.mark.parametrize("abk", TRIPLES)
def test_filter_and_smooth_three_steps(hip, abk):
    from pinn_kalman.ukf import SquareRootUKF
    n, N, T = 16, 3, 3
    g = torch.Generator().manual_seed(77)
    f, h = _models(n, n, g)
    m, S = 0.5 * torch.randn(N, n, generator=g), _tril(N, n, g, 0.1, 0.3)
    Q, R = _tril(N, n, g, 0.05, 0.05), _tril(N, n, g, 0.05, 0.2)
    zs = 0.5 * torch.randn(T, N, n, generator=g)
    Qd, Rd = Q.to(hip), R.to(hip)
    filt = SquareRootUKF(lambda x, u: (f(x), Qd), lambda x: (h(x), Rd), *abk)
    # T forward calls
    filt.initialize_beliefs(m.to(hip), scale_tril=S.to(hip))
    fw = [(filt(zs[t].to(hip)), filt.belief_scale_tril) for t in range(T)]
    runs = []
    for _ in range(2):
        filt.initialize_beliefs(m.to(hip), scale_tril=S.to(hip))
        hist = filt.filter(zs.to(hip))
        runs.append((hist, filt.smooth(hist), filt.status.clone()))
    hist, (ms, Ss), status = runs[0]
    assert ms.shape == (T + 1, N, n) and Ss.shape == (T + 1, N, n, n)
    assert hist.pred_means.shape == (T, N, n) and hist.pred_trils.shape == (T, N, n, n)
    assert torch.equal(hist.means[0].cpu(), m) and torch.equal(hist.scale_trils[0].cpu(), S)
    for t in range(T):
        assert torch.equal(hist.means[t + 1], fw[t][0]), f"filter != forward at step {t}"
        assert torch.equal(hist.scale_trils[t + 1], fw[t][1])
    assert torch.equal(filt.belief_mean, fw[-1][0])
    for a, b in zip((runs[0][0].means, runs[0][0].pred_trils) + runs[0][1],
                    (runs[1][0].means, runs[1][0].pred_trils) + runs[1][1]):
        assert torch.equal(a, b), "two identical runs differ"
    assert torch.equal(ms[T], hist.means[T]) and torch.equal(Ss[T], hist.scale_trils[T])
    # the same sequence of op.ukf calls by hand
    gamma, wm0, wc0, wi = K.merwe_weights(n, *abk)
    mh, Sh = ms[T], Ss[T]
    for t in range(T - 1, -1, -1):
        X = K.sigma_points(hist.means[t], hist.scale_trils[t], gamma)
        Y = f(X)
        pm, pt, _ = K.unscented_root(Y, Qd, n, wm0, wc0, wi)
        assert torch.equal(pm, hist.pred_means[t]) and torch.equal(pt, hist.pred_trils[t])
        mh, Sh, st = K.rts_smooth(hist.means[t], hist.scale_trils[t], X, Y, pm, pt, mh, Sh, wc0,
                                  wi)
        assert torch.equal(mh, ms[t]) and torch.equal(Sh, Ss[t]), f"smooth != by hand at {t}"
        _structure(Sh, st)
    assert status.tolist() == [0] * N
    # against the restatement chains, each in its own precision throughout
    ref = {}
    for dt in (torch.float64, torch.float32):
        r = urts_ref.chain(m.to(dt), S.to(dt), lambda x: (f(x), Q.to(dt)),
                           lambda x: (h(x), R.to(dt)), zs.to(dt), abk)
        assert not r[2].any()
        ref[dt] = (r[0][0], r[1][0])
    _gate(f"ukf.smooth chain3 abk={abk} mean", ms[0], ref[torch.float64][0], ref[torch.float32][0])
    _gate(f"ukf.smooth chain3 abk={abk} cov", _cov(Ss[0]), _cov(ref[torch.float64][1]),
          _cov(ref[torch.float32][1]))


def _isolation_case():
    """n = 16, N = 4, (1, 0, 0), seed 6: a healthy backward stage with next_tril = 0.7 pred_tril
    and next_mean = pred_mean + 0.1 randn."""
    n, N = 16, 4
    wm0, wc0, wi = 0., 0., 1. / (2 * n)
    g = torch.Generator().manual_seed(6)
    m, S, Q = 0.5 * torch.randn(N, n, generator=g), _tril(N, n, g, 0.1, 0.3), _tril(N, n, g, 0.05,
                                                                                  0.05)
    X = ukf_ref.sigma(m, S, 4., 1)
    Y = X + 0.2 * torch.sin(3 * X)
    mp, Sp, flag = ukf_ref.root(Y, Q, n, wm0, wc0, wi)
    assert not flag.any()
    ms1 = mp + 0.1 * torch.randn(N, n, generator=g)
    return n, N, wc0, wi, [m, S, X, Y, mp, Sp, ms1, 0.7 * Sp]


def test_a_nan_filter_leaves_the_others_bit_identical(hip):
    n, N, wc0, wi, args = _isolation_case()
    bad = 1
    good = [t.cpu() for t in K.rts_smooth(*(a.to(hip) for a in args), wc0, wi)]
    assert good[2].tolist() == [0] * N
    args[6] = args[6].clone()
    args[6][bad] = float("nan")
    got = [t.cpu() for t in K.rts_smooth(*(a.to(hip) for a in args), wc0, wi)]  # the call returns
    keep = torch.tensor([i for i in range(N) if i != bad])
    for i, (a, b) in enumerate(zip(good, got)):
        assert torch.equal(a[keep], b[keep]), f"output {i} of a healthy filter changed"
    assert torch.isnan(got[0][bad]).all()


def test_a_lost_downdate_is_flagged_finite_and_isolated(hip):
    """Filter 2's prediction factor 1e-3 times and its smoothed factor 1e-6 times too small: the
    columns of U = G S- are 1e3 times too large while those of W = G S^s_+ keep their size, so
    the downdates remove 1e6 times what the updates added.  A numerical condition, handled by the policy of the
    downdate: flagged, finite, the other filters untouched."""
    n, N, wc0, wi, args = _isolation_case()
    bad = 2
    good = [t.cpu() for t in K.rts_smooth(*(a.to(hip) for a in args), wc0, wi)]
    assert good[2].tolist() == [0] * N
    args[5], args[7] = args[5].clone(), args[7].clone()
    args[5][bad] *= 1e-3
    args[7][bad] *= 1e-6
    for dt in (torch.float64, torch.float32):
        ms, Ss, flag, _ = urts_ref.smooth(*(a.to(dt) for a in args), wc0, wi)
        assert flag.tolist() == [False, False, True, False]
        assert torch.isfinite(ms).all() and torch.isfinite(Ss).all()
    got = [t.cpu() for t in K.rts_smooth(*(a.to(hip) for a in args), wc0, wi)]
    assert got[2].dtype == torch.int32 and got[2].tolist() == [0, 0, 1, 0]
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    assert (got[1].triu(1) == 0).all()
    keep = torch.tensor([i for i in range(N) if i != bad])
    assert torch.equal(good[0][keep], got[0][keep]) and torch.equal(good[1][keep], got[1][keep])


@pytest.mark.parametrize("masked", [False, True])
def test_ukf_smooth_on_ns_dynamics_stagewise(hip, masked):
    """UKF(config, compat=False[, mask]): image 16, patch 8, B = 1 -> 16 filters of n = 64, T = 2
    frames of the truth rollout + N(0, 1e-3), once fully observed and once with about half of
    the density pixels observed.  Each backward stage is compared on the device's own stage
    inputs, so the stencil's sensitivity stays out of the tolerance; nothing is flagged."""
    from configs.pinn import pinn_pde
    from pinn_kalman.ukf import UKF
    from pinn_kalman.ukf_utils import InpaintKFMeasure, patch, unpatch
    c = pinn_pde.get_config()
    c.data.image_size = 16
    c.device = hip
    rng = np.random.default_rng(4)
    B, size, n, N, T = 1, 16, 64, 16, 2
    fields = torch.from_numpy(np.concatenate([
        rng.uniform(0.1, 1.0, (B, 1, size, size)),
        rng.uniform(0.05, 0.5, (B, 2, size, size)) * rng.choice([-1, 1], (B, 2, size, size)),
        rng.normal(0, 0.01, (B, 1, size, size))], 1).astype(np.float32))
    noise = torch.from_numpy(rng.normal(0, 1e-3, (T,) + tuple(fields.shape)).astype(np.float32))
    mask = torch.from_numpy((rng.random((size, size)) < 0.5).astype(np.float32))
    assert 0.35 < float(mask.mean()) < 0.65
    filt = UKF(c, compat=False, mask=mask if masked else None)
    assert isinstance(filt.measurement, InpaintKFMeasure) is masked
    x0 = patch(fields, 8)
    truth, obs = x0.to(hip), []
    for t in range(T):  # observation t sees the state after step t
        truth = filt.dynamic(truth)[0]
        obs.append(unpatch(truth, 8, size, 4) + noise[t].to(hip))
    obs = torch.stack(obs)
    assert obs.shape == (T, B, 4, size, size) and torch.isfinite(obs).all()
    filt.initialize(x0, var=1e-6)
    filtered, smoothed = filt.smooth(obs)
    assert filtered.shape == smoothed.shape == (T, B, 4, size, size)
    assert torch.isfinite(filtered).all() and torch.isfinite(smoothed).all()
    assert torch.equal(smoothed[T - 1], filtered[T - 1])
    assert filt.ukf.status.tolist() == [0] * N, "a filter was flagged"
    hist = filt.history
    # the forward half is T calls of forward
    ref = UKF(c, compat=False, mask=mask if masked else None)
    ref.initialize(x0, var=1e-6)
    for t in range(T):
        assert torch.equal(ref(obs[t]), filtered[t]), f"filter != forward at frame {t}"
        assert torch.equal(ref.ukf.belief_mean, hist.means[t + 1])
        assert torch.equal(ref.ukf.belief_scale_tril, hist.scale_trils[t + 1])
    if masked:  # the observation rows the filters saw: density masked, the rest untouched
        z = filt._observation(obs[0]).cpu()
        want = obs[0].cpu().clone()
        want[:, 0] *= mask
        assert torch.equal(z, patch(want, 8))
    # the backward half by hand, stage by stage
    gamma, wm0, wc0, wi = K.merwe_weights(n)
    ms, Ss = hist.means[T], hist.scale_trils[T]
    by_hand = [None] * T + [ms]
    for t in range(T - 1, -1, -1):
        X = K.sigma_points(hist.means[t], hist.scale_trils[t], gamma, 4)
        Y = filt.dynamic(X)[0]
        args = (hist.means[t], hist.scale_trils[t], X, Y, hist.pred_means[t], hist.pred_trils[t],
                ms, Ss)
        ms, Ss, st = K.rts_smooth(*args, wc0, wi, 4)
        _structure(Ss, st)
        cpu = [a.cpu() for a in args]
        s64 = urts_ref.smooth(*(a.double() for a in cpu), wc0, wi, 4)
        s32 = urts_ref.smooth(*cpu, wc0, wi, 4)
        assert not s64[2].any() and not s32[2].any()
        what = f"ukf.ns smooth masked={masked} t={t}"
        _gate(what + " mean", ms, s64[0], s32[0])
        _gate(what + " cov", _cov(Ss), _cov(s64[1]), _cov(s32[1]))
        by_hand[t] = ms
    # UKF.smooth is exactly that composition
    means_s, trils_s = filt.ukf.smooth(hist)
    assert torch.equal(means_s, torch.stack(by_hand)) and torch.equal(trils_s[0], Ss)
    for t in range(T):
        assert torch.equal(smoothed[t], unpatch(by_hand[t + 1], 8, size, 4))
