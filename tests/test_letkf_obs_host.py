"""CPU: the LETKF restatement for observations behind an operator (tests/letkf_obs_ref.py)
against the textbook Kalman update with a dense H, its reduction to tests/letkf_ref.py for the
identity, the argument checks of bpk_letkf_analysis_obs_f32 and op.letkf.analysis_obs, and the
host logic of pinn_kalman.enkf.LETKF(observe=...) on an injected step and analysis (float64)."""
import numpy as np
import pytest
import torch

import letkf_obs_ref as RO
import letkf_ref as R
from op import letkf as K
from pinn_kalman.enkf import LETKF, EnsembleHistory
from test_letkf_host import moments, shift_step, smooth_fields


def blur_decimate(x, stride, offset=0):
    """3-tap binomial blur (symmetric boundary) of every channel, then [offset::stride]."""
    return RO.binomial_blur(x)[..., offset::stride, offset::stride]


def global_case():
    """C = 2, 5 x 5, m = 8; observed through the binomial blur + stride-2 decimation (3 x 3 per
    channel); boxcar with R = 4 = max(H, W) - 1: every grid point sees every observation.  Two
    observations are missing (and hold NaN)."""
    rng = np.random.default_rng(17)
    m, C, H, W = 8, 2, 5, 5
    ens = rng.standard_normal((1, m, C, H, W))
    yens = blur_decimate(ens, 2)
    Hmat = np.stack([blur_decimate(e.reshape(C, H, W), 2).reshape(-1)
                     for e in np.eye(C * H * W)], 1)
    assert Hmat.shape == (18, 50) and np.abs(Hmat @ ens[0, 0].reshape(-1)
                                             - yens[0, 0].reshape(-1)).max() < 1e-14
    obs = rng.standard_normal(yens.shape[:1] + yens.shape[2:])
    prec = rng.uniform(0.5, 4.0, obs.shape)
    prec.reshape(-1)[[2, 13]] = 0
    obs[prec == 0] = np.nan
    return ens, yens, Hmat, obs, prec, np.ones((9, 9))


def test_global_window_analysis_is_the_kalman_update_with_H():
    ens, yens, Hmat, obs, prec, taper = global_case()
    out, status = RO.truth(ens, yens, obs, prec, taper, 1.0, stride=2, offset=0)
    assert status.sum() == 0
    mean, cov = moments(out)
    kmean, kcov = RO.kalman_update_linear(ens[0].reshape(8, -1), Hmat, obs.reshape(-1),
                                          prec.reshape(-1))
    assert np.abs(mean - kmean).max() <= 1e-10 * np.abs(kmean).max()
    assert np.abs(cov - kcov).max() <= 1e-10 * np.abs(kcov).max()
    # and it is not the update that mistakes the blurred image for the state's own samples
    wrong, _ = RO.truth(ens, ens[:, :, :, ::2, ::2], obs, prec, taper, 1.0, stride=2, offset=0)
    assert np.abs(moments(wrong)[0] - kmean).max() > 1e-3


def test_identity_observation_reduces_to_letkf_ref():
    rng = np.random.default_rng(3)
    ens = rng.standard_normal((2, 5, 3, 4, 6))
    obs = rng.standard_normal((2, 3, 4, 6))
    prec = rng.uniform(0.5, 4.0, obs.shape) * (rng.random(obs.shape) < 0.7)
    obs[prec == 0] = np.nan
    taper = K.gaspari_cohn_taper(2).numpy()
    a, sa = RO.truth(ens, ens, obs, prec, taper, 1.1, stride=1, offset=0)
    b, sb = R.truth(ens, obs, prec, taper, 1.1)
    assert np.array_equal(sa, sb) and np.abs(a - b).max() <= 1e-13
    e32 = ens.astype(np.float32)
    a, _ = RO.ref32(e32, e32, obs, prec, taper, 1.1)      # stride 1: offset None is 0
    b, _ = R.ref32(e32, obs, prec, taper, 1.1)
    assert a.dtype == np.float32 and np.array_equal(a, b)


def test_scatter_and_default_offset():
    v = np.arange(6.0).reshape(2, 3)
    s = RO.scatter(v, 5, 9, 3, 1)
    assert s.shape == (5, 9) and np.array_equal(s[1::3, 1::3][:2, :3], v) and s.sum() == v.sum()
    with pytest.raises(AssertionError):
        RO.scatter(v, 4, 9, 3, 1)    # 3 * 1 + 1 > 4 - 1
    x = np.random.default_rng(0).standard_normal((6, 6))
    assert np.allclose(RO.binomial_blur(x)[0, 0],
                       (9 * x[0, 0] + 3 * x[0, 1] + 3 * x[1, 0] + x[1, 1]) / 16)


def test_abi_argument_errors_without_a_device():
    from op import _lib
    dll = _lib.lib.load()
    syms = _lib.exported_symbols()
    assert "bpk_letkf_analysis_obs_f32" in syms and "bpk_letkf_obs_workspace_bytes" in syms

    def call(ens=None, yens=None, out=None, B=1, m=8, C=4, H=5, W=6, Cy=2, Hy=2, Wy=3, stride=2,
             offset=0, R=2, inflation=1.0):
        rc = dll.bpk_letkf_analysis_obs_f32(ens, yens, None, None, None, out, None, None, B, m, C,
                                            H, W, Cy, Hy, Wy, stride, offset, R, inflation, None)
        return rc, dll.bpk_last_error()

    for kw, name in ((dict(m=1), b"m = 1"), (dict(m=65), b"m = 65"), (dict(C=0), b"C = 0"),
                     (dict(C=9), b"C = 9"), (dict(Cy=0), b"Cy = 0"), (dict(Cy=9), b"Cy = 9"),
                     (dict(R=-1), b"R = -1"), (dict(R=9), b"R = 9"),
                     (dict(H=0), b"H = 0"), (dict(W=0), b"W = 0"),
                     (dict(Hy=0), b"Hy = 0"), (dict(Wy=0), b"Wy = 0"),
                     (dict(stride=0), b"stride = 0"), (dict(offset=-1), b"offset = -1"),
                     (dict(offset=2), b"offset = 2"),
                     (dict(Hy=4), b"Hy = 4"),             # 2 * 3 + 0 > 4
                     (dict(Wy=4), b"Wy = 4"),             # 2 * 3 + 0 > 5
                     (dict(offset=1, Hy=3), b"Hy = 3"),   # 2 * 2 + 1 > 4
                     (dict(inflation=0.0), b"inflation"), (dict(inflation=-2.0), b"inflation"),
                     (dict(ens=64, out=64), b"alias ens"),
                     (dict(yens=64, out=64), b"alias yens")):
        rc, msg = call(**kw)
        assert rc == 1 and name in msg, (kw, rc, msg)
    assert call(Hy=3)[1].count(b"Hy = 3") == 0            # 2 * 2 + 0 <= 4 fits: the NULL check is next
    rc, msg = call()  # valid sizes, NULL pointers: still an argument error, not a crash
    assert rc == 1 and b"ens is NULL" in msg
    rc, msg = call(ens=64)
    assert rc == 1 and b"yens is NULL" in msg
    rc, msg = call(ens=64, yens=64)                       # yens may alias ens
    assert rc == 1 and b"obs is NULL" in msg
    assert call(B=0)[0] == 0
    ws = dll.bpk_letkf_obs_workspace_bytes
    assert ws(2, 33, 4, 9, 12, 1, 3, 4) == (1 + 64) * (2 * 4 * 9 * 12 + 2 * 1 * 3 * 4) * 4
    assert ws(1, 8, 1, 3, 3, 1, 3, 3) == (1 + 8) * (9 + 9) * 4
    assert ws(3, 16, 4, 16, 16, 8, 4, 4) == (1 + 16) * (3 * 4 * 256 + 3 * 8 * 16) * 4
    assert ws(1, 65, 1, 3, 3, 1, 3, 3) == -1
    assert ws(1, 8, 1, 3, 3, 9, 3, 3) == -1
    assert ws(1, 8, 1, 3, 3, 1, 0, 3) == -1
    assert ws(1, 8, 1, 1 << 16, 1 << 15, 1, 1, 1) == -1


def test_op_argument_checks(monkeypatch):
    ens, yens, obs = torch.zeros(1, 4, 2, 5, 6), torch.zeros(1, 4, 1, 2, 3), torch.zeros(1, 1, 2, 3)
    taper = K.boxcar_taper(1)

    def run(ens=ens, yens=yens, obs=obs, prec=obs, taper=taper, **kw):
        kw.setdefault("stride", 2)
        return K.analysis_obs(ens, yens, obs, prec, taper, **kw)
    with pytest.raises(RuntimeError, match="HIP"):
        run()
    monkeypatch.setattr(K, "require_hip", lambda *a, **k: None)  # none of these reaches the library
    with pytest.raises(RuntimeError, match="float32"):
        run(yens=yens.double())
    with pytest.raises(RuntimeError, match="not differentiable"):
        run(yens=yens.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="ens must be"):
        run(ens=ens[0])
    with pytest.raises(RuntimeError, match="m = 1"):
        run(ens=ens[:, :1], yens=yens[:, :1])
    with pytest.raises(RuntimeError, match="C = 9"):
        run(ens=torch.zeros(1, 4, 9, 5, 6))
    with pytest.raises(RuntimeError, match="yens must be"):
        run(yens=yens[:, :3])
    with pytest.raises(RuntimeError, match="yens must be"):
        run(yens=yens[0])
    with pytest.raises(RuntimeError, match="Cy = 9"):
        run(yens=torch.zeros(1, 4, 9, 2, 3))
    with pytest.raises(RuntimeError, match=r"obs must be \[1, 1, 2, 3\]"):
        run(obs=torch.zeros(1, 2, 5, 6))
    with pytest.raises(RuntimeError, match="prec must be"):
        run(prec=obs[:, :, :1])
    with pytest.raises(RuntimeError, match="taper"):
        run(taper=torch.ones(2, 2))
    with pytest.raises(RuntimeError, match="R = 9"):
        run(taper=torch.ones(19, 19))
    with pytest.raises(RuntimeError, match="inflation"):
        run(inflation=0.0)
    with pytest.raises(RuntimeError, match="stride = 0"):
        run(stride=0)
    with pytest.raises(RuntimeError, match="stride = 1.5"):
        run(stride=1.5)
    with pytest.raises(RuntimeError, match="offset = 2"):
        run(offset=2)
    with pytest.raises(RuntimeError, match="offset = -1"):
        run(offset=-1)
    with pytest.raises(RuntimeError, match="Hy = 2 does not fit"):
        run(stride=4)                     # default offset 1: 4 * 1 + 1 > 4
    with pytest.raises(RuntimeError, match="Wy = 3 does not fit"):
        run(stride=2, offset=1, ens=torch.zeros(1, 4, 2, 5, 5))   # 2 * 2 + 1 > 4
    with pytest.raises(RuntimeError, match="contiguous"):
        run(yens=torch.zeros(1, 4, 1, 3, 2).transpose(3, 4))


# ---- filter host logic: a cyclic shift as the step, the float64 restatement as the analysis ----

def np_observe(stride, channels):
    def observe(x):
        return torch.from_numpy(np.ascontiguousarray(
            blur_decimate(x[:, channels].numpy(), stride, (stride - 1) // 2)))
    return observe


def ref_obs_analysis(ens, yens, obs, prec, taper, inflation, stride, offset):
    out, status = RO.truth(ens.numpy(), yens.numpy(), obs.numpy(), prec.numpy(), taper.numpy(),
                           inflation, stride, offset)
    return torch.from_numpy(out), torch.from_numpy(status)


def make_filter(m=5, radius=2, stride=2, channels=(0,), **kw):
    return LETKF(m, radius, step_fn=shift_step, obs_analysis_fn=ref_obs_analysis,
                 observe=np_observe(stride, list(channels)), obs_stride=stride, **kw)


def test_filter_shapes_and_missing_frames():
    g = torch.Generator().manual_seed(3)
    T, B, H, W, m = 4, 2, 6, 8, 5
    truth0 = torch.randn(B, 4, H, W, generator=g, dtype=torch.float64)
    observe = np_observe(2, [0, 3])
    obs = torch.stack([observe(torch.roll(truth0, t + 1, dims=-1)) for t in range(T)])
    assert tuple(obs.shape) == (T, B, 2, 3, 4)
    obs[1] = float("nan")                         # the missing frame may hold anything
    weights = torch.full((1, 2, 1, 1), 100.0, dtype=torch.float64)   # broadcast to [B, Cy, Hy, Wy]
    valid = torch.tensor([True, False, True, True])
    f = make_filter(m, channels=(0, 3), inflation=1.05)
    assert f.obs_stride == 2 and f.obs_offset == 0
    f.initialize(truth0 + 0.3, std=0.3, generator=g)
    assert f.observation_shape() == (B, 2, 3, 4)
    h = f.filter(obs, weights, valid=valid, keep_ensembles=True)
    assert isinstance(h, EnsembleHistory) and len(h) == T
    for name in ("means", "spreads", "forecast_means"):
        assert tuple(getattr(h, name).shape) == (T, B, 4, H, W), name
    assert h.flagged.dtype == torch.int64 and h.flagged.tolist() == [0] * T
    assert tuple(h.forecast_ensembles.shape) == tuple(h.analysis_ensembles.shape) == (T, B, m, 4, H, W)
    assert torch.equal(h.analysis_ensembles[1], h.forecast_ensembles[1])   # bit for bit
    assert torch.equal(h.means[1], h.forecast_means[1])
    assert not torch.equal(h.analysis_ensembles[0], h.forecast_ensembles[0])
    assert torch.isfinite(h.means).all() and torch.isfinite(h.spreads).all()
    # forecast of frame t + 1 is the step applied to the analysis of frame t
    for t in range(T - 1):
        assert torch.equal(h.forecast_ensembles[t + 1], torch.roll(h.analysis_ensembles[t], 1, dims=-1))
    # every grid point is updated, also those that carry no observation and the unobserved
    # channels (through the ensemble's covariances)
    assert ((h.analysis_ensembles[0] != h.forecast_ensembles[0]).all(dim=1)).all()
    # the observed image of the ensemble contracts
    ya, yf = (observe(e.reshape(B * m, 4, H, W)).reshape(B, m, 2, 3, 4).std(1)
              for e in (h.analysis_ensembles[0], h.forecast_ensembles[0]))
    assert ya.mean() < 0.7 * yf.mean()
    # a frame analysed alone is what the restatement makes of the recorded forecast
    fc = h.forecast_ensembles[2]
    want, _ = RO.truth(fc.numpy(), observe(fc.reshape(B * m, 4, H, W)).reshape(B, m, 2, 3, 4).numpy(),
                       obs[2].numpy(), np.full((B, 2, 3, 4), 100.0), f.taper.numpy(), 1.05, 2, 0)
    assert np.array_equal(h.analysis_ensembles[2].numpy(), want)


def test_per_sample_valid_mask_keeps_that_sample():
    g = torch.Generator().manual_seed(4)
    T, B, H, W, m = 2, 2, 4, 4, 4
    mean = torch.randn(B, 4, H, W, generator=g, dtype=torch.float64)
    obs = torch.randn(T, B, 1, 2, 2, generator=g, dtype=torch.float64)
    valid = torch.tensor([[True, False], [True, True]])
    obs[0, 1] = float("nan")
    f = make_filter(m, steps_per_frame=2)
    f.initialize(mean, perturbations=torch.randn(B, m, 4, H, W, generator=g, dtype=torch.float64))
    h = f.filter(obs, torch.ones(B, 1, 2, 2, dtype=torch.float64), valid=valid, keep_ensembles=True)
    assert torch.equal(h.analysis_ensembles[0, 1], h.forecast_ensembles[0, 1])
    assert not torch.equal(h.analysis_ensembles[0, 0], h.forecast_ensembles[0, 0])
    assert torch.isfinite(h.analysis_ensembles).all()
    assert torch.equal(h.forecast_ensembles[1], torch.roll(h.analysis_ensembles[0], 2, dims=-1))


def test_shape_errors_name_the_observation_shape():
    f = make_filter(4)
    f.initialize(torch.zeros(2, 4, 6, 8, dtype=torch.float64),
                 perturbations=torch.randn(2, 4, 4, 6, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\[2, 1, 3, 4\]"):
        f.filter(torch.zeros(3, 2, 4, 6, 8, dtype=torch.float64), 1.0)   # the state's shape
    with pytest.raises(ValueError, match=r"\[2, 1, 3, 4\]"):
        f.filter(torch.zeros(2, 1, 3, 4, dtype=torch.float64), 1.0)      # no frame axis
    f.forecast()
    with pytest.raises(ValueError, match=r"obs must be \[2, 1, 3, 4\]"):
        f.analyze(torch.zeros(2, 4, 6, 8, dtype=torch.float64), 1.0)
    with pytest.raises(ValueError, match="obs_stride"):
        LETKF(4, 2, observe=np_observe(2, [0]), obs_stride=0)
    with pytest.raises(ValueError, match="obs_offset"):
        LETKF(4, 2, observe=np_observe(2, [0]), obs_stride=2, obs_offset=2)
    assert LETKF(4, 2, obs_stride=4).obs_offset == 1 and LETKF(4, 2, obs_stride=4).observe is None


def test_without_observe_the_identity_path_runs():
    """observe=None: analysis_fn is what is called, with its five arguments, and
    obs_analysis_fn never."""
    calls = []

    def analysis_fn(ens, obs, prec, taper, inflation):
        calls.append((tuple(ens.shape), tuple(obs.shape)))
        return ens + 1, torch.zeros(ens.shape[0], *ens.shape[3:], dtype=torch.int32)

    def never(*a):
        raise AssertionError("obs_analysis_fn called without observe")
    f = LETKF(4, 1, step_fn=shift_step, analysis_fn=analysis_fn, obs_analysis_fn=never)
    f.initialize(torch.zeros(1, 4, 3, 3, dtype=torch.float64),
                 perturbations=torch.randn(1, 4, 4, 3, 3, dtype=torch.float64))
    f.filter(torch.zeros(2, 1, 4, 3, 3, dtype=torch.float64), 1.0)
    assert calls == [((1, 4, 4, 3, 3), (1, 4, 3, 3))] * 2


def twin(seed):
    """As test_letkf_host.twin (8 x 8, C = 1, m = 8, six frames of a cyclic shift), but the field
    is observed through the 3-tap binomial blur (symmetric boundary) at stride 2, offset 0:
    4 x 4 observations, sigma = 0.05, R = 2, inflation 1.05.  -> (rmse of the filter mean, rmse
    of the unassimilated ensemble mean) at the last frame."""
    g = torch.Generator().manual_seed(seed)
    T, H, W, m, sigma = 6, 8, 8, 8, 0.05
    truth = smooth_fields((1, 1, H, W), g)
    background = truth + 0.5 * smooth_fields((1, 1, H, W), g)
    pert = 0.5 * smooth_fields((1, m, 1, H, W), g)
    observe = np_observe(2, [0])
    frames = torch.stack([torch.roll(truth, t + 1, dims=-1) for t in range(T)])
    clean = torch.stack([observe(fr) for fr in frames])
    assert tuple(clean.shape) == (T, 1, 1, 4, 4)
    obs = clean + sigma * torch.randn(clean.shape, generator=g, dtype=torch.float64)
    f = LETKF(m, 2, inflation=1.05, step_fn=shift_step, obs_analysis_fn=ref_obs_analysis,
              observe=observe, obs_stride=2, obs_offset=0)
    f.initialize(background, perturbations=pert)
    free = torch.roll(f.mean(), T, dims=-1)
    h = f.filter(obs, 1.0 / sigma ** 2)
    assert h.flagged.sum().item() == 0

    def rmse(x):
        return ((x - frames[-1]) ** 2).mean().sqrt().item()
    return rmse(h.means[-1]), rmse(free)


def test_twin_experiment_through_the_blur_beats_the_free_run():
    ours, free = twin(0)
    print(f"letkf obs twin seed 0: filter rmse {ours:.4f}, free run {free:.4f}, ratio {ours / free:.3f}")
    assert ours < 0.5 * free
