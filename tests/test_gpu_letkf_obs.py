"""GPU: the LETKF analysis for observations on a grid of their own behind an operator
(csrc/letkf.hip, op.letkf.analysis_obs) and the filter built on it
(pinn_kalman.enkf.LETKF(observe=...)).

Truth: tests/letkf_obs_ref.py in float64 (np.linalg.eigh) on the same float32 inputs.  The
conventions are those of tests/test_gpu_letkf.py; the tolerance is measured per case,

    max|ours - truth| <= max(4 max|ref32 - truth|, 4 u max|truth|),   u = 2^-24,

with ref32 the float32 restatement with an explicit cyclic Jacobi.  Inflation 1.1.

Inputs: `ens` as there (fields of scale 2, spread 0.03).  `yens` is a linear image of `ens`:
observation channel c is the 3-tap binomial blur (symmetric boundary) of state channel c % C
times a gain 1 + 0.25 c, decimated [o::s, o::s], computed in float64 and rounded once.  `obs`
is that image of the mean plus noise of 0.03.  The fixture asserts cond(A) < 1e6 in float64 and
status 0 from both references.
"""
import functools

import numpy as np
import pytest
import torch

import letkf_obs_ref as RO
from conftest import record_err
from op import letkf as K
from test_gpu_letkf import CASES as ID_CASES
from test_gpu_letkf import _inflation_only
from test_gpu_letkf import _inputs as id_inputs
from test_gpu_letkf import _run as id_run

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
INFLATION = 1.1
#        B, m,  C, Cy, H, W, s, o, R
CASES = [(1, 2, 1, 1, 1, 1, 1, 0, 0),     # single site, smallest ensemble
         (2, 3, 4, 2, 5, 7, 2, 0, 2),     # odd sizes, window clipped on every side, batch
         (1, 33, 4, 1, 9, 12, 3, 1, 4),   # one past a padded size, stride 3 with an offset
         (1, 64, 2, 8, 8, 8, 1, 0, 3),    # full wave, more observed channels than state channels
         (1, 8, 4, 4, 6, 6, 4, 1, 8),     # window larger than the domain (boxcar)
         (1, 16, 8, 1, 8, 8, 4, 1, 1)]    # 28 of the 64 grid points see no observation at all
FOOTPRINT = (1, 8, 2, 1, 9, 9, 3, 1, 2)   # one observation, at (1, 2) = state point (4, 7)
PATTERNS = ["half_density", "prec1e4", "prec1e6"]


def _observe(x, case):
    """The linear image of x [..., C, H, W] (float64) on the observation grid of `case`."""
    _, _, C, Cy, _, _, s, o, _ = case
    blurred = RO.binomial_blur(np.asarray(x, np.float64))
    return np.stack([(1 + 0.25 * c) * blurred[..., c % C, o::s, o::s] for c in range(Cy)], -3)


def _taper(R_, kind="default"):
    if kind == "asymmetric":   # no symmetry at all, a few zeros: a transposed or mirrored index shows
        rng = np.random.default_rng(99)
        t = rng.uniform(0.5, 1.0, (2 * R_ + 1, 2 * R_ + 1)).astype(np.float32)
        t.reshape(-1)[rng.choice(t.size, 4, replace=False)] = 0
        assert not np.array_equal(t, t.T) and not np.array_equal(t, t[::-1]) \
            and not np.array_equal(t, t[:, ::-1])
        return t
    # the window-larger-than-the-domain case uses the boxcar so that every entry counts
    return (K.boxcar_taper(R_) if R_ == 8 else K.gaspari_cohn_taper(R_)).numpy()


@functools.lru_cache(maxsize=None)
def _fields(case):
    B, m, C, Cy, H, W, s, o, _ = case
    rng = np.random.default_rng(sum(v * 10 ** i for i, v in enumerate(case)))
    mean = 2 * rng.standard_normal((B, 1, C, H, W))
    ens = (mean + 0.03 * rng.standard_normal((B, m, C, H, W))).astype(np.float32)
    yens = _observe(ens, case).astype(np.float32)
    ymean = _observe(mean[:, 0], case)
    obs = (ymean + 0.03 * rng.standard_normal(ymean.shape)).astype(np.float32)
    half = rng.random((B, 1) + ymean.shape[2:]) < 0.5
    assert yens.shape == (B, m, Cy, len(range(o, H, s)), len(range(o, W, s)))
    return ens, yens, obs, half


@functools.lru_cache(maxsize=None)
def _inputs(case, pattern, taper_kind="default"):
    """(ens, yens, obs, prec, taper) float32 and their float64 / float32 reference results,
    computed once and never modified."""
    s, o, R_ = case[6:]
    ens, yens, obs, half = _fields(case)
    obs = obs.copy()
    if pattern == "none":
        prec = np.zeros(obs.shape, np.float32)
    elif pattern == "half_density":
        prec = np.zeros(obs.shape, np.float32)
        prec[:, 0:1] = 1e4 * half
    elif pattern == "one":
        prec = np.zeros(obs.shape, np.float32)
        prec[0, 0, 1, 2] = 1e4
    else:
        prec = np.full(obs.shape, {"prec1e4": 1e4, "prec1e6": 1e6}[pattern], np.float32)
    obs[prec == 0] = np.nan   # the masked-frame convention: anything may stand there
    taper = _taper(R_, taper_kind)
    A = RO.system(ens, yens, np.nan_to_num(obs), prec, taper, INFLATION, s, o, np.float64)[2]
    cond = np.linalg.cond(A)
    assert cond.max() < 1e6, f"input family: cond(A) = {cond.max():.2e}"
    truth, st = RO.truth(ens, yens, obs, prec, taper, INFLATION, s, o)
    ref32, st32 = RO.ref32(ens, yens, obs, prec, taper, INFLATION, s, o)
    assert st.sum() == 0 and st32.sum() == 0
    tol = max(4 * np.abs(ref32 - truth).max(), 4 * U * np.abs(truth).max())
    return ens, yens, obs, prec, taper, truth, tol


def _run(hip, ens, yens, obs, prec, taper, stride, offset, inflation=INFLATION):
    out, status = K.analysis_obs(*(torch.from_numpy(np.ascontiguousarray(v)).to(hip)
                                   for v in (ens, yens, obs, prec)), torch.from_numpy(taper),
                                 inflation, stride, offset)
    assert out.dtype == torch.float32 and status.dtype == torch.int32
    assert tuple(out.shape) == ens.shape and tuple(status.shape) == (ens.shape[0],) + ens.shape[3:]
    return out.cpu().numpy(), status.cpu().numpy()


def _id(case):
    return "x".join(str(v) for v in case)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernel_vs_float64(hip, case, pattern):
    ens, yens, obs, prec, taper, truth, tol = _inputs(case, pattern)
    out, status = _run(hip, ens, yens, obs, prec, taper, case[6], case[7])
    err = np.abs(out - truth).max()
    print(f"letkf obs {_id(case)} {pattern}: err {err:.3e} tol {tol:.3e}")
    record_err(f"letkf analysis_obs {_id(case)} {pattern}", err, tol)
    assert np.isfinite(out).all() and status.sum() == 0
    assert err <= tol
    merr = np.abs(out.astype(np.float64).mean(1) - truth.mean(1)).max()
    record_err(f"letkf analysis_obs mean {_id(case)} {pattern}", merr, tol)
    assert merr <= tol
    if pattern != "half_density":
        # every channel observed: the observed image of the mean moves towards the observations
        after = _observe(out.astype(np.float64).mean(1), case)
        before = _observe(ens.astype(np.float64).mean(1), case)
        assert np.abs(after - obs).mean() < np.abs(before - obs).mean()


def test_asymmetric_taper(hip):
    case = CASES[1]
    ens, yens, obs, prec, taper, truth, tol = _inputs(case, "prec1e4", "asymmetric")
    out, status = _run(hip, ens, yens, obs, prec, taper, case[6], case[7])
    err = np.abs(out - truth).max()
    record_err(f"letkf analysis_obs asymmetric taper {_id(case)}", err, tol)
    assert status.sum() == 0 and err <= tol
    # the check has teeth: the truth under the transposed or mirrored table is further away
    for other in (taper.T, taper[::-1], taper[:, ::-1], taper[::-1, ::-1]):
        wrong, _ = RO.truth(ens, yens, obs, prec, np.ascontiguousarray(other), INFLATION,
                            case[6], case[7])
        assert np.abs(wrong - truth).max() > 10 * tol


@pytest.mark.parametrize("case", ID_CASES[1:4], ids=_id)
def test_identity_observation_gives_the_bits_of_analysis(hip, case):
    ens, obs, prec, taper, _, _ = id_inputs(case, "prec1e4")
    want, wstatus = id_run(hip, ens, obs, prec, taper)
    out, status = _run(hip, ens, ens, obs, prec, taper, 1, 0)
    assert np.array_equal(out, want) and np.array_equal(status, wstatus)
    out, status = _run(hip, ens, ens, obs, prec, taper, 1, None)   # offset None is 0 at stride 1
    assert np.array_equal(out, want) and np.array_equal(status, wstatus)


def test_footprint_of_one_observation(hip):
    case = FOOTPRINT
    ens, yens, obs, prec, taper, truth, tol = _inputs(case, "one")
    assert np.count_nonzero(prec) == 1 and yens.shape[2:] == (1, 3, 3)
    out, status = _run(hip, ens, yens, obs, prec, taper, 3, 1)
    err = np.abs(out - truth).max()
    record_err(f"letkf analysis_obs one observation {_id(case)}", err, tol)
    assert status.sum() == 0 and err <= tol
    R_ = case[8]
    sees = np.zeros((9, 9), bool)
    for y0 in range(9):
        for x0 in range(9):
            dy, dx = 4 - y0, 7 - x0
            sees[y0, x0] = abs(dy) <= R_ and abs(dx) <= R_ and taper[dy + R_, dx + R_] != 0
    # rows 2..6, columns 5..8 (the window is clipped at x = 8); Gaspari-Cohn with the default
    # cutoff is 5e-5 in the window's corners, not 0
    assert sees.sum() == 20 and sees[4, 7] and sees[2, 5] and not sees[4, 4] and not sees[1, 7]
    _, want = _inflation_only(ens, INFLATION)
    differs = (out != want).any(axis=(1, 2))[0]
    assert np.array_equal(differs, sees)
    same = ~np.broadcast_to(sees, out.shape)
    assert np.array_equal(out[same], want[same])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_nothing_observed_is_inflation_only(hip, case):
    ens, yens, obs, prec, taper, truth, tol = _inputs(case, "none")
    assert np.isnan(obs).all()
    out, status = _run(hip, ens, yens, obs, prec, taper, case[6], case[7])
    assert status.sum() == 0 and np.isfinite(out).all()
    err = np.abs(out - truth).max()
    record_err(f"letkf analysis_obs inflation only {_id(case)}", err, tol)
    assert err <= tol
    assert np.array_equal(out, _inflation_only(ens, INFLATION)[1])


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[3]], ids=_id)
def test_two_runs_are_bit_identical(hip, case):
    ens, yens, obs, prec, taper, _, _ = _inputs(case, "prec1e4")
    a, sa = _run(hip, ens, yens, obs, prec, taper, case[6], case[7])
    b, sb = _run(hip, ens, yens, obs, prec, taper, case[6], case[7])
    assert np.array_equal(a, b) and np.array_equal(sa, sb)


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[5]], ids=_id)
def test_member_permutation_permutes_the_output(hip, case):
    ens, yens, obs, prec, taper, truth, tol = _inputs(case, "prec1e4")
    perm = np.random.default_rng(5).permutation(ens.shape[1])
    out, status = _run(hip, ens[:, perm], yens[:, perm], obs, prec, taper, case[6], case[7])
    err = np.abs(out - truth[:, perm]).max()
    record_err(f"letkf analysis_obs permuted members {_id(case)}", err, tol)
    assert status.sum() == 0 and err <= tol


def test_global_window_is_the_kalman_update_with_H(hip):
    """The host test's setup in float32: C = 2, 5 x 5, m = 8, blur + stride-2 decimation, boxcar
    with R = 4, inflation 1, two observations missing.  Mean and sample covariance of the
    analysis ensemble against xbar + K (y - H xbar) and (I - K H) Pb with the dense H (float64,
    no eigen-decomposition on that route)."""
    from test_letkf_host import moments
    from test_letkf_obs_host import blur_decimate, global_case
    ens, _, Hmat, obs, prec, taper = global_case()
    ens = ens.astype(np.float32)
    yens = blur_decimate(ens.astype(np.float64), 2).astype(np.float32)
    obs, prec, taper = obs.astype(np.float32), prec.astype(np.float32), taper.astype(np.float32)
    kmean, kcov = RO.kalman_update_linear(ens[0].reshape(8, -1), Hmat, obs.reshape(-1),
                                          prec.reshape(-1))
    rmean, rcov = moments(RO.ref32(ens, yens, obs, prec, taper, 1.0, 2, 0)[0])
    out, status = _run(hip, ens, yens, obs, prec, taper, 2, 0, inflation=1.0)
    mean, cov = moments(out)
    assert status.sum() == 0
    for name, got, ref, want in (("mean", mean, rmean, kmean), ("cov", cov, rcov, kcov)):
        err = np.abs(got - want).max()
        tol = max(4 * np.abs(ref - want).max(), 4 * U * np.abs(want).max())
        record_err(f"letkf analysis_obs global window kalman {name}", err, tol)
        assert err <= tol, (name, err, tol)


def test_status_and_fallback_on_non_finite_input(hip):
    """An observed NaN reaches A and g of every grid point that sees it: those are flagged and
    keep the inflated background; the others are analysed as if nothing had happened."""
    case = CASES[1]
    ens, yens, obs, prec, taper, truth, tol = _inputs(case, "prec1e4")
    obs = obs.copy()
    obs[0, 1, 1, 2] = np.nan                       # sample 0, observation (1, 2) = state point (2, 4)
    out, status = _run(hip, ens, yens, obs, prec, taper, 2, 0)
    want = np.zeros(status.shape, np.int32)
    for y0 in range(5):
        for x0 in range(7):
            dy, dx = 2 - y0, 4 - x0
            want[0, y0, x0] = abs(dy) <= 2 and abs(dx) <= 2 and taper[dy + 2, dx + 2] != 0
    assert 0 < want.sum() < 35 and np.array_equal(status, want)
    flagged = np.broadcast_to(status[:, None, None].astype(bool), out.shape)
    background = _inputs(case, "none")[5]          # xbar + sqrt(inflation) dX in float64
    assert np.abs(out - background)[flagged].max() <= 4 * U * np.abs(background).max()
    assert np.abs(out - truth)[~flagged].max() <= tol


# ---- the filter on the simulator step -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _filter_run(missing):
    """LETKF.filter on ns_step.full_step(compat=False): 16 x 16, B = 2, m = 8, R = 2, T = 3, two
    simulator steps per frame; the density is observed through a 5-tap Gaussian blur at stride
    2 (8 x 8), half of the observations present.  `missing`: the middle frame is not valid (and
    holds NaN).  The members in observation space are recorded as the analysis receives them."""
    from op import blur
    from pinn_kalman.enkf import LETKF, blur_observation
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(21)
    T, B, H, W, m = 3, 2, 16, 16, 8
    taps = blur.gaussian_taps(1.0, 5)
    y, x = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([torch.exp(-((x - 0.4) ** 2 + (y - 0.5) ** 2) / 0.05),
                        0.3 * torch.sin(6.28 * y), 0.3 * torch.cos(6.28 * x), 0.1 * x * y])
    mean = (base[None] + 0.02 * torch.randn(B, 4, H, W, generator=g)).to(dev)
    image = blur.blur2d(base[None, 0:1].to(dev), taps, 2)                # [1, 1, 8, 8]
    obs = image[None] + (0.02 * torch.randn(T, B, 1, 8, 8, generator=g)).to(dev)
    weights = ((torch.rand(B, 1, 8, 8, generator=g) < 0.5).float() / 0.02 ** 2).to(dev)
    valid = None
    if missing:
        valid = torch.tensor([True, False, True])
        obs[1] = float("nan")
    seen = []

    def recording(ens, yens, *rest):
        seen.append(yens)
        return K.analysis_obs(ens, yens, *rest)
    f = LETKF(m, 2, inflation=1.05, steps_per_frame=2, observe=blur_observation(taps, 2, [0]),
              obs_stride=2, obs_analysis_fn=recording)
    f.initialize(mean, std=[0.05, 0.02, 0.02, 0.01], length=2.0,
                 generator=torch.Generator().manual_seed(22))
    h = f.filter(obs, weights, valid=valid, keep_ensembles=True)
    return f, h, obs, weights, seen, taps


@pytest.mark.parametrize("missing", [False, True], ids=["all_frames", "missing_middle"])
def test_filter_on_the_simulator(hip, missing):
    from op import blur, ns_step
    f, h, obs, weights, seen, taps = _filter_run(missing)
    T, B, m = 3, 2, 8
    assert f.obs_stride == 2 and f.obs_offset == 0
    assert tuple(h.means.shape) == tuple(h.spreads.shape) == tuple(h.forecast_means.shape) \
        == (T, B, 4, 16, 16)
    assert h.flagged.is_cuda and h.flagged.tolist() == [0] * T
    assert tuple(h.analysis_ensembles.shape) == (T, B, m, 4, 16, 16)
    assert torch.isfinite(h.analysis_ensembles).all()
    assert len(seen) == (2 if missing else 3)
    taper = f.taper.numpy()
    prec = weights.cpu().numpy()
    seen = iter(seen)
    for t in range(T):
        fc, an = h.forecast_ensembles[t], h.analysis_ensembles[t]
        if missing and t == 1:
            assert torch.equal(fc, an)           # forecast only: bit for bit
        else:
            yens = next(seen)
            assert tuple(yens.shape) == (B, m, 1, 8, 8)
            density = fc.reshape(B * m, 4, 16, 16)[:, 0:1].contiguous()
            assert torch.equal(yens, blur.blur2d(density, taps, 2).view(B, m, 1, 8, 8))
            # the reference analysis of the recorded forecast, fed the device's yens, is the
            # recorded analysis: nothing accumulates across frames, the kernel tolerance applies
            o = obs[t].cpu().numpy()
            o[prec == 0] = np.nan
            args = (fc.cpu().numpy(), yens.cpu().numpy(), o, prec, taper, f.inflation, 2, 0)
            truth, _ = RO.truth(*args)
            ref32, _ = RO.ref32(*args)
            tol = max(4 * np.abs(ref32 - truth).max(), 4 * U * np.abs(truth).max())
            err = np.abs(an.cpu().numpy() - truth).max()
            record_err(f"letkf obs filter frame {t} missing={missing}", err, tol)
            assert err <= tol, (t, err, tol)
            assert not torch.equal(fc, an)
        assert torch.equal(h.means[t], an.mean(1))
        assert torch.equal(h.forecast_means[t], fc.mean(1))
        if t + 1 < T:   # the next forecast is steps_per_frame simulator steps of this analysis
            p = an.reshape(B * m, 4, 16, 16)
            s = (p[:, 0:1].contiguous(), p[:, 1:3].contiguous(), p[:, 3:4].contiguous())
            for _ in range(f.steps_per_frame):
                s = ns_step.full_step(*s, f.dt, f.dx, compat=False)
            assert torch.equal(torch.cat(s, 1).view(B, m, 4, 16, 16), h.forecast_ensembles[t + 1])
