"""GPU: the LETKF analysis kernel (csrc/letkf.hip, op.letkf.analysis) and the filter built on
it (pinn_kalman.enkf.LETKF).

Truth: tests/letkf_ref.py in float64 (np.linalg.eigh) on the same float32 inputs; the reference
project has no ensemble filter.  The tolerance is measured, not chosen: per case

    max|ours - truth| <= max(4 max|ref32 - truth|, 4 u max|truth|),   u = 2^-24,

where ref32 is the float32 restatement with an explicit cyclic Jacobi: the kernel may be four
times as far from the truth as plain float32 arithmetic is (another summation order over the
window, another order of the rotations), with a floor of four units of roundoff of the
largest value.

Inputs: fields of scale 2 carrying an ensemble spread of 0.03 -- an ensemble that has been
assimilating for a while.  With all C channels observed at precision 1e6 (sigma = 1e-3) the
m x m problems reach cond(A) of order 1e4 .. 1e5 (asserted < 1e6 on the inputs, in float64);
a spread of order one under such observations would put cond(A) near 1 / u, where no float32
eigen-solver has correct digits in the small eigenvalues.
"""
import functools

import numpy as np
import pytest
import torch

import letkf_ref as R
from conftest import record_err
from op import letkf as K

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
INFLATION = 1.1
#        B, m,  C, H, W,  R
CASES = [(1, 2, 1, 1, 1, 0),     # single site, smallest ensemble
         (2, 3, 4, 5, 7, 2),     # odd sizes, window clipped on every side, batch
         (1, 33, 4, 9, 12, 4),   # one past a padded size
         (1, 64, 2, 8, 8, 3),    # full wave
         (1, 8, 4, 6, 6, 8),     # window larger than the domain
         (1, 16, 8, 4, 4, 1)]    # C at its limit
PATTERNS = ["half_density", "prec1e4", "prec1e6"]


def _taper(R_):
    # the window-larger-than-the-domain case uses the boxcar so that every entry counts
    return (K.boxcar_taper(R_) if R_ == 8 else K.gaspari_cohn_taper(R_)).numpy()


@functools.lru_cache(maxsize=None)
def _fields(case):
    B, m, C, H, W, _ = case
    rng = np.random.default_rng(sum(v * 10 ** i for i, v in enumerate(case)))
    mean = 2 * rng.standard_normal((B, 1, C, H, W))
    ens = (mean + 0.03 * rng.standard_normal((B, m, C, H, W))).astype(np.float32)
    obs = (mean[:, 0] + 0.03 * rng.standard_normal((B, C, H, W))).astype(np.float32)
    half = rng.random((B, 1, H, W)) < 0.5
    return ens, obs, half


@functools.lru_cache(maxsize=None)
def _inputs(case, pattern):
    """(ens, obs, prec, taper) float32 and their float64 / float32 reference results, computed
    once and never modified."""
    B, m, C, H, W, R_ = case
    ens, obs, half = _fields(case)
    obs = obs.copy()
    if pattern == "none":
        prec = np.zeros((B, C, H, W), np.float32)
    elif pattern == "half_density":
        prec = np.zeros((B, C, H, W), np.float32)
        prec[:, 0:1] = 1e4 * half
    else:
        prec = np.full((B, C, H, W), {"prec1e4": 1e4, "prec1e6": 1e6}[pattern], np.float32)
    obs[prec == 0] = np.nan   # the masked-frame convention: anything may stand there
    taper = _taper(R_)
    cond = np.linalg.cond(R.system(ens, np.nan_to_num(obs), prec, taper, INFLATION, np.float64)[2])
    assert cond.max() < 1e6, f"input family: cond(A) = {cond.max():.2e}"
    truth, st = R.truth(ens, obs, prec, taper, INFLATION)
    ref32, st32 = R.ref32(ens, obs, prec, taper, INFLATION)
    assert st.sum() == 0 and st32.sum() == 0
    tol = max(4 * np.abs(ref32 - truth).max(), 4 * U * np.abs(truth).max())
    return ens, obs, prec, taper, truth, tol


def _run(hip, ens, obs, prec, taper, inflation=INFLATION):
    out, status = K.analysis(*(torch.from_numpy(np.ascontiguousarray(v)).to(hip)
                               for v in (ens, obs, prec)), torch.from_numpy(taper), inflation)
    assert out.dtype == torch.float32 and status.dtype == torch.int32
    assert tuple(out.shape) == ens.shape and tuple(status.shape) == (ens.shape[0],) + ens.shape[3:]
    return out.cpu().numpy(), status.cpu().numpy()


def _id(case):
    return "x".join(str(v) for v in case)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_kernel_vs_float64(hip, case, pattern):
    ens, obs, prec, taper, truth, tol = _inputs(case, pattern)
    out, status = _run(hip, ens, obs, prec, taper)
    err = np.abs(out - truth).max()
    print(f"letkf {_id(case)} {pattern}: err {err:.3e} tol {tol:.3e}")
    record_err(f"letkf analysis {_id(case)} {pattern}", err, tol)
    assert np.isfinite(out).all() and status.sum() == 0
    assert err <= tol
    # the analysis perturbations sum to zero over the members: the member mean is the
    # analysis mean xbar + dX wbar
    merr = np.abs(out.astype(np.float64).mean(1) - truth.mean(1)).max()
    record_err(f"letkf analysis mean {_id(case)} {pattern}", merr, tol)
    assert merr <= tol
    if pattern != "half_density":
        # every channel observed: the mean moves towards the observations
        xbar = ens.astype(np.float64).mean(1)
        assert np.abs(out.astype(np.float64).mean(1) - obs).mean() < np.abs(xbar - obs).mean()


def _inflation_only(ens, inflation):
    """What the kernel's arithmetic gives with nothing observed and Jacobi a no-op (Q = I
    exactly): xbar by a sequential float32 sum over the members, one float32 factor
    sqrt(m-1) / sqrt((m-1) / inflation), one rounding of the product, one of the sum."""
    f32 = np.float32
    m = ens.shape[1]
    s = np.zeros_like(ens[:, 0])
    for k in range(m):
        s = s + ens[:, k]
    xbar = s / f32(m)
    d = np.sqrt(f32(m - 1)) / np.sqrt(f32(m - 1) / f32(inflation))
    assert xbar.dtype == f32 and d.dtype == f32
    return xbar, xbar[:, None] + (ens - xbar[:, None]) * d


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_nothing_observed_is_inflation_only(hip, case):
    ens, obs, prec, taper, truth, tol = _inputs(case, "none")
    assert np.isnan(obs).all()
    out, status = _run(hip, ens, obs, prec, taper)
    assert status.sum() == 0 and np.isfinite(out).all()
    err = np.abs(out - truth).max()           # truth = xbar + sqrt(inflation) dX in float64
    record_err(f"letkf inflation only {_id(case)}", err, tol)
    assert err <= tol                         # a few ulp: 4 max(ref32's error, u max|truth|)
    xbar, want = _inflation_only(ens, INFLATION)
    assert np.array_equal(out, want)          # any rotation at all would change these bits
    # ... and the member mean is xbar, untouched
    merr = np.abs(out.astype(np.float64).mean(1) - xbar).max()
    assert merr <= 4 * U * np.abs(xbar).max()
    out1, _ = _run(hip, ens, obs, prec, taper, inflation=1.0)
    assert np.array_equal(out1, _inflation_only(ens, 1.0)[1])


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[3]], ids=_id)
def test_two_runs_are_bit_identical(hip, case):
    ens, obs, prec, taper, _, _ = _inputs(case, "prec1e4")
    a, sa = _run(hip, ens, obs, prec, taper)
    b, sb = _run(hip, ens, obs, prec, taper)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[5]], ids=_id)
def test_member_permutation_permutes_the_output(hip, case):
    ens, obs, prec, taper, truth, tol = _inputs(case, "prec1e4")
    perm = np.random.default_rng(5).permutation(ens.shape[1])
    out, status = _run(hip, ens[:, perm], obs, prec, taper)
    err = np.abs(out - truth[:, perm]).max()
    record_err(f"letkf permuted members {_id(case)}", err, tol)
    assert status.sum() == 0 and err <= tol


def test_global_window_is_the_kalman_update(hip):
    """The host test's setup in float32: C = 2, 3 x 3, m = 6, boxcar, R = 2, inflation 1, three
    entries unobserved.  Mean and sample covariance of the analysis ensemble against
    xbar + K (y - H xbar) and (I - K H) Pb (float64, no eigen-decomposition on that route)."""
    from test_letkf_host import global_case, moments
    ens, obs, prec, taper = global_case(np.float32)
    kmean, kcov = R.kalman_update(ens[0].reshape(6, -1), obs.reshape(-1), prec.reshape(-1))
    rmean, rcov = moments(R.ref32(ens, obs, prec, taper, 1.0)[0])
    out, status = _run(hip, ens, obs, prec, taper, inflation=1.0)
    mean, cov = moments(out)
    assert status.sum() == 0
    for name, got, ref, want in (("mean", mean, rmean, kmean), ("cov", cov, rcov, kcov)):
        err = np.abs(got - want).max()
        tol = max(4 * np.abs(ref - want).max(), 4 * U * np.abs(want).max())
        record_err(f"letkf global window kalman {name}", err, tol)
        assert err <= tol, (name, err, tol)


def test_status_and_fallback_on_non_finite_input(hip):
    """An observed NaN reaches A and g of every grid point that sees it: those are flagged and
    keep the inflated background; the others are analysed as if nothing had happened."""
    case = CASES[1]
    ens, obs, prec, taper, truth, tol = _inputs(case, "prec1e4")
    obs = obs.copy()
    obs[0, 1, 0, 0] = np.nan                       # sample 0, corner: seen within R = 2
    out, status = _run(hip, ens, obs, prec, taper)
    want = np.zeros(status.shape, np.int32)
    want[0, :3, :3] = 1
    want[0][np.pad(taper[2:, 2:], ((0, 2), (0, 4))) == 0] = 0   # tapered out: not seen
    assert np.array_equal(status, want)
    flagged = np.broadcast_to(status[:, None, None].astype(bool), out.shape)
    background = _inputs(case, "none")[4]          # xbar + sqrt(inflation) dX in float64
    assert np.abs(out - background)[flagged].max() <= 4 * U * np.abs(background).max()
    assert np.abs(out - truth)[~flagged].max() <= tol


# ---- the filter on the simulator step -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _filter_run(missing):
    """LETKF.filter on ns_step.full_step(compat=False): 16 x 16, B = 2, m = 8, R = 2, T = 3, two
    simulator steps per frame; `missing`: the middle frame is not valid (and holds NaN)."""
    from pinn_kalman.enkf import LETKF
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    T, B, H, W, m = 3, 2, 16, 16, 8
    y, x = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([torch.exp(-((x - 0.4) ** 2 + (y - 0.5) ** 2) / 0.05),
                        0.3 * torch.sin(6.28 * y), 0.3 * torch.cos(6.28 * x), 0.1 * x * y])
    mean = (base[None] + 0.02 * torch.randn(B, 4, H, W, generator=g)).to(dev)
    obs = (base[None, None] + 0.02 * torch.randn(T, B, 4, H, W, generator=g)).to(dev)
    weights = torch.zeros(1, B, 4, H, W, device=dev)
    weights[:, :, 0] = (torch.rand(H, W, generator=g) < 0.5).float().to(dev) / 0.02 ** 2
    valid = None
    if missing:
        valid = torch.tensor([True, False, True])
        obs[1] = float("nan")
    f = LETKF(m, 2, inflation=1.05, steps_per_frame=2)
    f.initialize(mean, std=[0.05, 0.02, 0.02, 0.01], length=2.0,
                 generator=torch.Generator().manual_seed(12))
    h = f.filter(obs, weights, valid=valid, keep_ensembles=True)
    return f, h, obs, weights


@pytest.mark.parametrize("missing", [False, True], ids=["all_frames", "missing_middle"])
def test_filter_on_the_simulator(hip, missing):
    from op import ns_step
    f, h, obs, weights = _filter_run(missing)
    T, B, m = 3, 2, 8
    assert tuple(h.means.shape) == tuple(h.spreads.shape) == tuple(h.forecast_means.shape) \
        == (T, B, 4, 16, 16)
    assert h.flagged.is_cuda and h.flagged.tolist() == [0] * T
    assert tuple(h.analysis_ensembles.shape) == (T, B, m, 4, 16, 16)
    assert torch.isfinite(h.analysis_ensembles).all()
    taper = f.taper.numpy()
    prec = weights[0].cpu().numpy()
    for t in range(T):
        fc, an = h.forecast_ensembles[t], h.analysis_ensembles[t]
        if missing and t == 1:
            assert torch.equal(fc, an)           # forecast only: bit for bit
        else:
            # the reference analysis of the recorded forecast is the recorded analysis: nothing
            # accumulates across frames, the kernel tolerance applies
            o = obs[t].cpu().numpy()
            o[prec == 0] = np.nan
            truth, _ = R.truth(fc.cpu().numpy(), o, prec, taper, f.inflation)
            ref32, _ = R.ref32(fc.cpu().numpy(), o, prec, taper, f.inflation)
            tol = max(4 * np.abs(ref32 - truth).max(), 4 * U * np.abs(truth).max())
            err = np.abs(an.cpu().numpy() - truth).max()
            record_err(f"letkf filter frame {t} missing={missing}", err, tol)
            assert err <= tol, (t, err, tol)
        assert torch.equal(h.means[t], an.mean(1))
        assert torch.equal(h.spreads[t], an.std(1, unbiased=True))
        assert torch.equal(h.forecast_means[t], fc.mean(1))
        if t + 1 < T:   # the next forecast is steps_per_frame simulator steps of this analysis
            p = an.reshape(B * m, 4, 16, 16)
            s = (p[:, 0:1].contiguous(), p[:, 1:3].contiguous(), p[:, 3:4].contiguous())
            for _ in range(f.steps_per_frame):
                s = ns_step.full_step(*s, f.dt, f.dx, compat=False)
            assert torch.equal(torch.cat(s, 1).view(B, m, 4, 16, 16), h.forecast_ensembles[t + 1])


def test_initial_perturbations_are_smooth_scaled_and_centred(hip):
    from pinn_kalman.enkf import LETKF
    f = LETKF(16, 2)
    mean = torch.zeros(1, 4, 32, 32, device=hip)
    std = torch.tensor([0.5, 0.1, 0.2, 0.05])
    ens = f.initialize(mean, std=std, length=4.0, generator=torch.Generator().manual_seed(1))
    assert ens.is_cuda and tuple(ens.shape) == (1, 16, 4, 32, 32)
    assert ens.mean(1).abs().max().item() <= 4 * U * ens.abs().max().item() * 4
    # 15 x 1024 deviations per channel, correlated over ~(2 pi 4) pixels: a few per cent
    got = ens.std(dim=(0, 1, 3, 4)).cpu() / (std * (15 / 16) ** 0.5)
    assert ((got - 1).abs() < 0.1).all()
    # smoothed: neighbouring pixels correlate as exp(-1 / (4 length)) = 0.94 says, white noise at 0
    d = ens - ens.mean(dim=(3, 4), keepdim=True)
    corr = (d[..., 1:] * d[..., :-1]).mean() / (d * d).mean()
    assert corr.item() > 0.8
