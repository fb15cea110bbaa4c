"""CPU: the LETKF restatement tests/letkf_ref.py against the textbook Kalman update (a route
that forms no eigen-decomposition), the taper tables, the argument checks of the ABI entry
point and of op.letkf.analysis, and the host logic of pinn_kalman.enkf.LETKF on an injected
step and analysis (float64)."""
import math

import numpy as np
import pytest
import torch

import letkf_ref as R
from op import letkf as K
from pinn_kalman.enkf import LETKF, EnsembleHistory


def global_case(dtype=np.float64):
    """C = 2, 3 x 3, m = 6, boxcar with R = 2 >= max(H, W) - 1: every grid point sees every
    observation.  Three entries are unobserved (and hold NaN)."""
    rng = np.random.default_rng(7)
    m, C, H, W = 6, 2, 3, 3
    ens = rng.standard_normal((1, m, C, H, W)).astype(dtype)
    obs = rng.standard_normal((1, C, H, W)).astype(dtype)
    prec = rng.uniform(0.5, 4.0, (1, C, H, W)).astype(dtype)
    prec.reshape(-1)[[1, 5, 11]] = 0
    obs[prec == 0] = np.nan
    return ens, obs, prec, np.ones((5, 5), dtype)


def moments(out):
    """Member mean [n] and sample covariance [n, n] (float64) of out [1, m, C, H, W]."""
    o = np.asarray(out[0], np.float64).reshape(out.shape[1], -1)
    d = o - o.mean(0)
    return o.mean(0), d.T @ d / (o.shape[0] - 1)


def test_global_window_analysis_is_the_kalman_update():
    ens, obs, prec, taper = global_case()
    out, status = R.truth(ens, obs, prec, taper, 1.0)
    assert status.tolist() == [[[0] * 3] * 3]
    mean, cov = moments(out)
    kmean, kcov = R.kalman_update(ens[0].reshape(6, -1), obs.reshape(-1), prec.reshape(-1))
    assert np.abs(mean - kmean).max() <= 1e-12
    assert np.abs(cov - kcov).max() <= 1e-12


def test_float32_jacobi_restatement_is_close_to_the_truth():
    """The yardstick is what it says: same equations, float32, explicit Jacobi."""
    ens, obs, prec, taper = global_case(np.float32)
    out, status, sweeps = R.ref32(ens, obs, prec, taper, 1.0, return_sweeps=True)
    truth, _ = R.truth(ens, obs, prec, taper, 1.0)
    assert out.dtype == np.float32 and status.sum() == 0 and 1 <= sweeps.max() < R.SWEEP_CAP
    assert np.abs(out - truth).max() <= 64 * 2.0 ** -24 * np.abs(truth).max()
    lam, Q, _, capped = R.jacobi_eigh(np.eye(5, dtype=np.float32)[None] * 3)
    assert not capped.any() and np.array_equal(Q[0], np.eye(5, dtype=np.float32))
    # a sweep cap that is reached is reported, per problem
    A = np.stack([np.eye(5), np.eye(5) + 0.3 * np.ones((5, 5))]).astype(np.float32)
    lam, Q, sweeps, capped = R.jacobi_eigh(A, cap=1)
    assert capped.tolist() == [False, True] and sweeps.tolist() == [0, 1]
    lam, Q, sweeps, capped = R.jacobi_eigh(A)
    assert not capped.any() and np.abs(np.sort(lam[1]) - [1, 1, 1, 1, 2.5]).max() < 1e-6


def test_round_robin_meets_every_pair_once():
    for n in (2, 8, 16, 64):
        seen = set()
        for t in range(n - 1):
            p, q = R.round_robin(t, n)
            assert len(set(p.tolist()) | set(q.tolist())) == n and (p < q).all()
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == n * (n - 1) // 2


@pytest.mark.parametrize("radius", [0, 1, 2, 5, 8])
def test_gaspari_cohn_table(radius):
    t = K.gaspari_cohn_taper(radius)
    n = 2 * radius + 1
    assert t.dtype == torch.float32 and tuple(t.shape) == (n, n) and not t.is_cuda
    assert t[radius, radius].item() == 1.0
    for sym in (t.flip(0), t.flip(1), t.t(), t.flip(0).t(), t.flip(1).t(), t.flip(0, 1),
                t.flip(0, 1).t()):
        assert torch.equal(sym, t)
    cutoff = (radius + 1) / 2
    d = torch.arange(-radius, radius + 1, dtype=torch.float64)
    dist = (d[:, None] ** 2 + d[None, :] ** 2).sqrt().reshape(-1)
    v = t.reshape(-1)
    assert (v[dist >= 2 * cutoff] == 0).all() and (v >= 0).all()
    order = torch.argsort(dist)
    assert (v[order][1:] <= v[order][:-1]).all()           # never increases with distance
    inside = dist[order] < 2 * cutoff - 1e-9
    ds, vs = dist[order][inside], v[order][inside]
    assert (vs[1:][ds[1:] > ds[:-1]] < vs[:-1][ds[1:] > ds[:-1]]).all()  # decreases in support
    # the edge midpoints of the window are inside the support, as the default promises
    if radius:
        assert t[0, radius].item() > 0
    wide = K.gaspari_cohn_taper(2, cutoff=40.0)  # z <= sqrt(8) / 40: GC >= 1 - 5/3 z^2 > 0.99
    assert (wide > 0.99).all()
    assert K.gaspari_cohn(torch.tensor([0.0, 1.0, 2.0, 3.0])).tolist() == pytest.approx(
        [1.0, 5.0 / 24.0, 0.0, 0.0], abs=1e-15)


def test_boxcar_and_taper_arguments():
    assert torch.equal(K.boxcar_taper(3), torch.ones(7, 7))
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError):
            K.gaspari_cohn_taper(bad)
        with pytest.raises(ValueError):
            K.boxcar_taper(bad)
    with pytest.raises(ValueError):
        K.gaspari_cohn_taper(2, cutoff=0.0)


def test_abi_argument_errors_without_a_device():
    from op import _lib
    dll = _lib.lib.load()
    syms = _lib.exported_symbols()
    assert "bpk_letkf_analysis_f32" in syms and "bpk_letkf_workspace_bytes" in syms

    def call(ens=None, out=None, B=1, m=8, C=4, H=5, W=6, R=2, inflation=1.0):
        rc = dll.bpk_letkf_analysis_f32(ens, None, None, None, out, None, None, B, m, C, H, W, R,
                                        inflation, None)
        return rc, dll.bpk_last_error()

    for kw, name in ((dict(m=1), b"m = 1"), (dict(m=65), b"m = 65"), (dict(C=0), b"C = 0"),
                     (dict(C=9), b"C = 9"), (dict(R=-1), b"R = -1"), (dict(R=9), b"R = 9"),
                     (dict(H=0), b"H = 0"), (dict(W=0), b"W = 0"),
                     (dict(inflation=0.0), b"inflation"), (dict(inflation=-2.0), b"inflation"),
                     (dict(ens=64, out=64), b"ens_out")):
        rc, msg = call(**kw)
        assert rc == 1 and name in msg, (kw, rc, msg)
    rc, msg = call()  # valid sizes, NULL pointers: still an argument error, not a crash
    assert rc == 1 and b"NULL" in msg
    assert call(B=0)[0] == 0
    assert dll.bpk_letkf_workspace_bytes(2, 33, 4, 9, 12) == 2 * 4 * 9 * 12 * (1 + 64) * 4
    assert dll.bpk_letkf_workspace_bytes(1, 8, 1, 3, 3) == 9 * (1 + 8) * 4
    assert dll.bpk_letkf_workspace_bytes(1, 65, 1, 3, 3) == -1


def test_op_argument_checks(monkeypatch):
    ens, obs = torch.zeros(1, 4, 2, 5, 6), torch.zeros(1, 2, 5, 6)
    taper = K.boxcar_taper(1)
    with pytest.raises(RuntimeError, match="HIP"):
        K.analysis(ens, obs, obs, taper)
    monkeypatch.setattr(K, "require_hip", lambda *a, **k: None)  # none of these reaches the library
    with pytest.raises(RuntimeError, match="float32"):
        K.analysis(ens.double(), obs, obs, taper)
    with pytest.raises(RuntimeError, match="not differentiable"):
        K.analysis(ens.clone().requires_grad_(True), obs, obs, taper)
    with pytest.raises(RuntimeError, match="ens must be"):
        K.analysis(ens[0], obs, obs, taper)
    with pytest.raises(RuntimeError, match="m = 1"):
        K.analysis(ens[:, :1], obs, obs, taper)
    with pytest.raises(RuntimeError, match="C = 9"):
        K.analysis(torch.zeros(1, 4, 9, 5, 6), torch.zeros(1, 9, 5, 6), torch.zeros(1, 9, 5, 6), taper)
    with pytest.raises(RuntimeError, match="prec must be"):
        K.analysis(ens, obs, obs[:, :1], taper)
    with pytest.raises(RuntimeError, match="taper"):
        K.analysis(ens, obs, obs, torch.ones(2, 2))
    with pytest.raises(RuntimeError, match="R = 9"):
        K.analysis(ens, obs, obs, torch.ones(19, 19))
    with pytest.raises(RuntimeError, match="inflation"):
        K.analysis(ens, obs, obs, taper, inflation=0.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        K.analysis(ens, torch.zeros(1, 2, 6, 5).transpose(2, 3), obs, taper)


# ---- filter host logic: a cyclic shift as the step, the float64 restatement as the analysis ----

def shift_step(f, v, p):
    return tuple(torch.roll(t, 1, dims=-1) for t in (f, v, p))


def ref_analysis(ens, obs, prec, taper, inflation):
    out, status = R.truth(ens.numpy(), obs.numpy(), prec.numpy(), taper.numpy(), inflation)
    return torch.from_numpy(out), torch.from_numpy(status)


def make_filter(m=5, radius=1, **kw):
    return LETKF(m, radius, step_fn=shift_step, analysis_fn=ref_analysis, **kw)


def test_filter_shapes_and_missing_frames():
    g = torch.Generator().manual_seed(3)
    T, B, H, W, m = 4, 2, 5, 6, 5
    truth0 = torch.randn(B, 4, H, W, generator=g, dtype=torch.float64)
    obs = torch.stack([torch.roll(truth0, t + 1, dims=-1) for t in range(T)])
    obs[1] = float("nan")                         # the missing frame may hold anything
    weights = torch.zeros(1, B, 4, H, W, dtype=torch.float64)
    weights[:, :, 0] = 100.0
    valid = torch.tensor([True, False, True, True])
    f = make_filter(m, inflation=1.05)
    ens0 = f.initialize(truth0 + 0.3, std=0.3, generator=g)
    assert tuple(ens0.shape) == (B, m, 4, H, W)
    assert (ens0.mean(1) - (truth0 + 0.3)).abs().max() < 1e-14  # centred perturbations
    # 240 independent deviations per channel: the sample std scatters by 1 / sqrt(480) = 4.6 %
    per_channel = (ens0 - ens0.mean(1, keepdim=True)).std(dim=(0, 1, 3, 4))
    assert torch.allclose(per_channel, torch.full((4,), 0.3 * math.sqrt((m - 1) / m),
                                                  dtype=torch.float64), rtol=0.2)
    h = f.filter(obs, weights, valid=valid, keep_ensembles=True)
    assert isinstance(h, EnsembleHistory) and len(h) == T
    for name in ("means", "spreads", "forecast_means"):
        assert tuple(getattr(h, name).shape) == (T, B, 4, H, W), name
    assert tuple(h.flagged.shape) == (T,) and h.flagged.dtype == torch.int64
    assert h.flagged.tolist() == [0] * T
    assert tuple(h.forecast_ensembles.shape) == tuple(h.analysis_ensembles.shape) == (T, B, m, 4, H, W)
    assert torch.equal(h.analysis_ensembles[1], h.forecast_ensembles[1])   # bit for bit
    assert torch.equal(h.means[1], h.forecast_means[1])
    assert not torch.equal(h.analysis_ensembles[0], h.forecast_ensembles[0])
    assert torch.isfinite(h.means).all() and torch.isfinite(h.spreads).all()
    # forecast of frame t + 1 is the step applied to the analysis of frame t
    assert torch.equal(h.forecast_ensembles[2], torch.roll(h.analysis_ensembles[1], 1, dims=-1))
    # spread is the unbiased standard deviation over the members
    assert torch.equal(h.spreads[3], h.analysis_ensembles[3].std(1, unbiased=True))
    # the observed channel's spread shrinks where it is assimilated
    assert h.spreads[0][:, 0].mean() < h.forecast_ensembles[0].std(1)[:, 0].mean()
    f2 = make_filter(m)
    f2.initialize(truth0, std=[0.1, 0.2, 0.3, 0.4], generator=g)
    h2 = f2.filter(obs[:1], weights)
    assert h2.analysis_ensembles is None and h2.forecast_ensembles is None and len(h2) == 1


def test_per_sample_valid_mask_keeps_that_sample():
    g = torch.Generator().manual_seed(4)
    T, B, H, W, m = 2, 2, 4, 4, 4
    mean = torch.randn(B, 4, H, W, generator=g, dtype=torch.float64)
    obs = torch.randn(T, B, 4, H, W, generator=g, dtype=torch.float64)
    valid = torch.tensor([[True, False], [True, True]])
    obs[0, 1] = float("nan")
    f = make_filter(m, steps_per_frame=2)
    f.initialize(mean, perturbations=torch.randn(B, m, 4, H, W, generator=g, dtype=torch.float64))
    h = f.filter(obs, torch.ones(B, 4, H, W, dtype=torch.float64), valid=valid, keep_ensembles=True)
    assert torch.equal(h.analysis_ensembles[0, 1], h.forecast_ensembles[0, 1])
    assert not torch.equal(h.analysis_ensembles[0, 0], h.forecast_ensembles[0, 0])
    assert torch.isfinite(h.analysis_ensembles).all()
    assert torch.equal(h.forecast_ensembles[1], torch.roll(h.analysis_ensembles[0], 2, dims=-1))


def test_constructor_and_state_errors():
    with pytest.raises(ValueError):
        LETKF(1, 2)
    with pytest.raises(ValueError):
        LETKF(65, 2)
    with pytest.raises(ValueError):
        LETKF(8, 9)
    with pytest.raises(ValueError):
        LETKF(8, 2, taper="cosine")
    with pytest.raises(ValueError):
        LETKF(8, 2, inflation=0.0)
    with pytest.raises(ValueError):
        LETKF(8, 2, steps_per_frame=0)
    with pytest.raises(ValueError):
        LETKF(8, 2, taper=torch.ones(3, 3))
    f = LETKF(8, 2, taper="boxcar")
    assert torch.equal(f.taper, torch.ones(5, 5)) and f.radius == 2
    assert torch.equal(LETKF(8, 2).taper, K.gaspari_cohn_taper(2))
    with pytest.raises(RuntimeError, match="initialize"):
        f.mean()
    with pytest.raises(ValueError):
        f.initialize(torch.zeros(3, 4, 4), std=1.0)
    with pytest.raises(ValueError):
        f.initialize(torch.zeros(1, 4, 4, 4))


def smooth_fields(shape, g):
    """Unit-variance random fields, correlated over a few pixels (cyclic binomial smoothing)."""
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    for _ in range(3):
        for d in (-1, -2):
            x = 0.25 * (torch.roll(x, 1, dims=d) + torch.roll(x, -1, dims=d)) + 0.5 * x
    return x / x.std()


def twin(seed):
    """8 x 8, C = 1, m = 8, R = 2, every second pixel of every second row observed with
    sigma = 0.05, inflation 1.05, six frames of a cyclic shift.  The background error is a draw
    from the distribution of the perturbations.  -> (rmse of the filter mean, rmse of the
    unassimilated ensemble mean) at the last frame."""
    g = torch.Generator().manual_seed(seed)
    T, H, W, m, sigma = 6, 8, 8, 8, 0.05
    truth = smooth_fields((1, 1, H, W), g)
    background = truth + 0.5 * smooth_fields((1, 1, H, W), g)
    pert = 0.5 * smooth_fields((1, m, 1, H, W), g)
    mask = torch.zeros(H, W, dtype=torch.float64)
    mask[::2, ::2] = 1
    weights = (mask / sigma ** 2).view(1, 1, H, W)
    frames = torch.stack([torch.roll(truth, t + 1, dims=-1) for t in range(T)])
    obs = frames + sigma * torch.randn(frames.shape, generator=g, dtype=torch.float64)
    f = make_filter(m, radius=2, inflation=1.05)
    f.initialize(background, perturbations=pert)
    free = torch.roll(f.mean(), T, dims=-1)
    h = f.filter(obs, weights)
    assert h.flagged.sum().item() == 0

    def rmse(x):
        return ((x - frames[-1]) ** 2).mean().sqrt().item()
    return rmse(h.means[-1]), rmse(free)


def test_twin_experiment_beats_the_free_run():
    ours, free = twin(0)
    assert ours < free
