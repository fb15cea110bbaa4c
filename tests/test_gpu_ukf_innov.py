"""GPU: the innovation statistics (csrc/ukf.hip k_innovation, op.ukf.innovation) and what
pinn_kalman.ukf builds on them: NIS / log-likelihood, gating, missing frames.

Truth: tests/ukf_innov_ref.py in float64 on the same float32 inputs (the Gaussian density in
closed form; the reference project has no counterpart).

Kernel tolerances (Higham, Accuracy and Stability of Numerical Algorithms, Thm 8.5: the computed
e solves (S + dS) e = r with |dS| <= gamma_dz |S|, and r = obs - z_mean carries one rounding),
with u = 2^-24 and kappa the inf-norm condition number of that filter's factor (asserted <= 10
on the inputs, in float64 on the CPU):
    white   max|e_hat - e|    <= (dz + 2) u kappa max|e|                       =: tol_white
    nis     |nis_hat - nis|   <= 2 sqrt(dz) tol_white ||e||_2 + (dz + 2) u nis  =: tol_nis
    loglik                    <= 0.5 tol_nis + 4 dz u max(1, sum_i |log S_ii|)
Factors are a I + 0.1 L / sqrt(dz) (L strictly lower, standard normal), a in {0.5, 1, 3}: with
the 0.3 first intended the family reaches kappa = 38 at dz = 64, a = 0.5 (12 at a = 1), so the
off-diagonal scale was lowered until the condition on the inputs holds (largest kappa 6.9).

Note on the masked field test: the measurement model hands the filter config.inverse.variance as
the *factor* entry of a density pixel (IdentityKFMeasure, unchanged), so the innovation variance
of an unobserved pixel is variance^2 and the closed-form density gives
-0.5 p^2 log(2 pi variance^2) for a fully unobserved patch; that is what is asserted (to 1e-6
relative), not the -0.5 p^2 log(2 pi variance) a variance-valued setting would give."""
import functools
import math

import numpy as np
import pytest
import torch

import ukf_innov_ref as R
import ukf_ref
from conftest import record_err
from op import ukf as K

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DZS = [1, 2, 7, 63, 64]
NS = [1, 3, 257]
OFF = 0.1


@functools.lru_cache(maxsize=None)
def _inputs(N, dz):
    """float32 inputs (a cycles over 0.5, 1, 3 along the filters) and their float64 results,
    computed once and never modified."""
    rng = np.random.default_rng(1000 * dz + N)
    a = np.array([0.5, 1., 3.])[np.arange(N) % 3]
    L = np.tril(rng.standard_normal((N, dz, dz)), -1)
    S = (a[:, None, None] * np.eye(dz) + OFF * L / math.sqrt(dz)).astype(np.float32)
    zm = rng.standard_normal((N, dz)).astype(np.float32)
    z = (zm + a[:, None] * rng.standard_normal((N, dz))).astype(np.float32)
    kappa = R.kappa_inf(S)
    assert kappa.max() <= 10, f"input family: kappa_inf = {kappa.max():.2f} > 10"
    return S, zm, z, kappa, R.innovation(zm, S, z)


def _run(hip, zm, S, z, **kw):
    out = K.innovation(*(torch.from_numpy(np.ascontiguousarray(v)).to(hip) for v in (zm, S, z)),
                       **kw)
    return [None if o is None else o.cpu().numpy() for o in out]


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dz", DZS)
def test_kernel_vs_float64(hip, N, dz):
    S, zm, z, kappa, (e, nis, ll, st) = _inputs(N, dz)
    ge, gn, gl, gs = _run(hip, zm, S, z)
    assert ge.shape == (N, dz) and gn.shape == gl.shape == gs.shape == (N,)
    assert ge.dtype == gn.dtype == gl.dtype == np.float32 and gs.dtype == np.int32
    assert gs.tolist() == [0] * N == st.tolist()
    tol_w = (dz + 2) * U * kappa * np.abs(e).max(1)
    tol_n = 2 * math.sqrt(dz) * tol_w * np.sqrt(nis) + (dz + 2) * U * nis
    logs = np.abs(np.log(np.diagonal(S.astype(np.float64), axis1=1, axis2=2))).sum(1)
    tol_l = 0.5 * tol_n + 4 * dz * U * np.maximum(1., logs)
    worst = {}
    for name, got, ref, tol in (("white", np.abs(ge - e).max(1), 0., tol_w),
                                ("nis", gn, nis, tol_n), ("loglik", gl, ll, tol_l)):
        err = np.abs(got - ref)
        i = int(np.argmax(err / tol))
        worst[name] = (err[i], tol[i])
        record_err(f"ukf.innovation {name} N={N} dz={dz}", err[i], tol[i])
        print(f"ukf.innovation {name} N={N} dz={dz}: err {err[i]:.3e} tol {tol[i]:.3e}")
    for name, (err, tol) in worst.items():
        assert err <= tol, f"{name}: {err:.3e} > {tol:.3e}"
    # white = None: the same statistics, nothing else written
    ne, nn, nl, ns = _run(hip, zm, S, z, white=False)
    assert ne is None and np.array_equal(nn, gn) and np.array_equal(nl, gl) and not ns.any()
    # only the lower triangle is read
    rng = np.random.default_rng(7)
    junk = S + np.triu(rng.standard_normal(S.shape).astype(np.float32) * 1e3, 1)
    if dz > 1:
        junk[0, 0, dz - 1] = np.nan
    for a, b in zip(_run(hip, zm, junk, z), (ge, gn, gl, gs)):
        assert np.array_equal(a, b), "the upper triangle leaked into the result"
    # deterministic
    for a, b in zip(_run(hip, zm, S, z), (ge, gn, gl, gs)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dz", [1, 7, 64])
def test_a_bad_factor_is_flagged_nan_and_isolated(hip, dz):
    N = 7
    S, zm, z, _, _ = _inputs(257, dz)
    S, zm, z = S[:N].copy(), zm[:N], z[:N]
    bad = {1: 0., 3: -0.5, 4: np.nan}
    Sb = S.copy()
    for i, v in bad.items():
        Sb[i, (i * 5) % dz, (i * 5) % dz] = v
    ge, gn, gl, gs = _run(hip, zm, Sb, z)
    assert gs.tolist() == [int(i in bad) for i in range(N)]
    for i in bad:
        assert np.isnan(ge[i]).all() and np.isnan(gn[i]) and np.isnan(gl[i])
    keep = [i for i in range(N) if i not in bad]
    he, hn, hl, hs = _run(hip, zm[keep], S[keep], z[keep])
    assert not hs.any() and np.isfinite(he).all() and np.isfinite(hl).all()
    assert np.array_equal(ge[keep], he) and np.array_equal(gn[keep], hn)
    assert np.array_equal(gl[keep], hl)
    # +inf on the diagonal is no factor either
    Sb = S.copy()
    Sb[2, 0, 0] = np.inf
    assert _run(hip, zm, Sb, z)[3].tolist() == [0, 0, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("n,dz,abk", [(16, 16, (1., 0., 0.)), (9, 9, (0.5, 2., 0.)),
                                      (4, 3, (1., 2., 1.)), (64, 64, (1., 0., 0.))])
def test_white_is_the_vector_the_update_applied(hip, n, dz, abk):
    """m+ - m- of kalman_update against U e with e from the innovation kernel and U = P_xz S_z^-T
    rebuilt in float64, at the update test's own gate (tests/test_gpu_ukf.py: max(1e-5, 2 x the
    float32 restatement's error), relative to max|m+|)."""
    import test_gpu_ukf as T
    c = T._case(n, dz, abk)
    _, _, wc0, wi = c["w"]
    args = [c[k].to(hip) for k in ("m1", "S1", "X2", "Z", "zm", "zt", "z")]
    mean, _, status = K.kalman_update(*args, wc0, wi, c["groups"])
    e, nis, _, st = K.innovation(args[4], args[5], args[6])
    assert not status.any() and not st.any()
    U64 = c["up64"][3]["U"]
    step = torch.einsum('nij,nj->ni', U64, e.double().cpu())
    ref64, ref32 = c["up64"][0], c["up32"][0]
    scale = float(ref64.abs().max())
    err = float((mean.double().cpu() - (c["m1"].double() + step)).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    tol = max(1e-5, 2 * e32)
    record_err(f"ukf.innovation U e vs update n={n} dz={dz} abk={abk}", err, tol)
    print(f"U e vs update n={n} dz={dz}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    # nis is e^T e of that very vector (summation order apart: dz products, float32)
    assert torch.allclose(nis, (e * e).sum(1), rtol=dz * 2 * U, atol=0)


# ----------------------------------------------------------------------------------------
# the filter on a small model: n = dz = 4, N = 8

@functools.lru_cache(maxsize=None)
def _small(seed=11, N=8, n=4):
    """The model's tensors on the CPU (read only): F, m, S, three observations."""
    g = torch.Generator().manual_seed(seed)
    F = torch.eye(n) + 0.3 * torch.randn(n, n, generator=g) / math.sqrt(n)
    m = 0.5 * torch.randn(N, n, generator=g)
    S = (0.1 * torch.randn(N, n, n, generator=g) / math.sqrt(n)).tril() + 0.3 * torch.eye(n)
    zs = 0.5 * torch.randn(3, N, n, generator=g)
    return F, m, S, zs


Q_DIAG, R_DIAG = 0.05, 0.2


def _models(F, N=8, n=4):
    """f(x) = F x + 0.2 sin 3x (no BLAS: the same float32 products everywhere), h(x) = x +
    0.1 tanh(x)^2, constant noise factors; on F's device and dtype."""
    Q = (Q_DIAG * torch.eye(n)).repeat(N, 1, 1).to(F)
    Rf = (R_DIAG * torch.eye(n)).repeat(N, 1, 1).to(F)

    def dyn(x, u=None):
        return (x.unsqueeze(1) * F).sum(-1) + 0.2 * torch.sin(3 * x), Q

    class Measure(torch.nn.Module):
        calls = 0

        def forward(self, x):
            self.calls += 1
            return x + 0.1 * torch.tanh(x) ** 2, Rf
    return dyn, Measure()


def _filter(hip, groups, **kw):
    from pinn_kalman.ukf import SquareRootUKF
    F, m, S, zs = _small()
    dyn, meas = _models(F.to(hip))
    f = SquareRootUKF(dyn, meas, groups=groups, **kw)
    f.initialize_beliefs(m.to(hip), scale_tril=S.to(hip))
    return f, meas, zs.to(hip)


@pytest.mark.parametrize("groups", [1, 4])
def test_off_means_off(hip, groups):
    f0, _, zs = _filter(hip, groups)
    f1, _, _ = _filter(hip, groups, diagnostics=True)
    h0, h1 = f0.filter(zs), f1.filter(zs)
    assert torch.equal(f0.belief_mean, f1.belief_mean)
    assert torch.equal(f0.belief_scale_tril, f1.belief_scale_tril)
    assert torch.equal(f0.status, f1.status)
    assert torch.equal(h0.means, h1.means) and torch.equal(h0.scale_trils, h1.scale_trils)
    assert f0.nis is None and f0.loglik is None and f0.accepted is None
    assert h0.nis is None and h0.logliks is None and h0.accepted is None
    assert f1.nis.shape == f1.loglik.shape == (8,) and f1.accepted.dtype == torch.bool
    assert h1.nis.shape == h1.logliks.shape == h1.accepted.shape == (3, 8)
    assert h1.accepted.all() and torch.isfinite(h1.nis).all() and torch.isfinite(h1.logliks).all()
    assert torch.equal(h1.nis[2], f1.nis)


def _nis64(groups, z):
    """NIS of the small model's first step in float64 (the tests/ukf_ref.py chain on the CPU)."""
    F, m, S, _ = _small()
    dyn, meas = _models(F.double())
    o = ukf_ref.step(m.double(), S.double(), dyn, meas, z.double(), (1., 0., 0.), groups)
    assert not o["flag"].any()
    return R.innovation(o["z_mean"].numpy(), o["z_tril"].numpy(), z.double().numpy())[1]


@pytest.mark.parametrize("groups", [1, 4])
def test_gating_and_valid(hip, groups):
    out = [2, 5]
    expected = torch.tensor([i not in out for i in range(8)])
    _, _, zs = _filter(hip, groups)
    z = zs[0].clone()
    z[out] += 100.
    nis64 = _nis64(groups, z.cpu())
    gate = 1e3
    assert nis64[expected.numpy()].max() < gate / 10 and nis64[out].min() > gate * 10, nis64
    plain, _, _ = _filter(hip, groups)
    plain.predict()
    pm, pS = plain.belief_mean.clone(), plain.belief_scale_tril.clone()
    plain.update(z)
    for kw, valid in ((dict(gate=gate), None), (dict(), expected.to(hip))):
        f, _, _ = _filter(hip, groups, **kw)
        got = f(z, valid=valid)
        acc = f.accepted.cpu()
        assert torch.equal(acc, expected)
        assert torch.equal(got[out], pm[out]) and torch.equal(f.belief_scale_tril[out], pS[out])
        assert torch.equal(got[acc], plain.belief_mean[acc])
        assert torch.equal(f.belief_scale_tril[acc], plain.belief_scale_tril[acc])
        assert f.nis.shape == (8,) and not f.status.any()
        if valid is None:  # the gate saw the statistics of every filter
            assert torch.isfinite(f.nis).all() and torch.isfinite(f.loglik).all()
        else:              # no observation, no statistic
            assert torch.isnan(f.nis[out]).all() and torch.isnan(f.loglik[out]).all()
            assert torch.isfinite(f.nis[acc]).all()
    # a NaN statistic is rejected by the gate
    zn = z.clone()
    zn[0, 0] = float("nan")
    f, _, _ = _filter(hip, groups, gate=gate)
    got = f(zn)
    assert f.accepted.cpu().tolist() == [False] + expected.tolist()[1:]
    assert torch.equal(got[0], pm[0]) and torch.isfinite(got).all()


def test_a_missing_frame_is_predict_only_and_smooths(hip):
    f, meas, zs = _filter(hip, 1)
    h = f.filter([zs[0], None, zs[2]], valid=[True, False, True])
    assert meas.calls == 2, "the measurement model ran on the missing frame"
    assert torch.equal(h.means[2], h.pred_means[1])
    assert torch.equal(h.scale_trils[2], h.pred_trils[1])
    assert torch.isnan(h.nis[1]).all() and torch.isnan(h.logliks[1]).all()
    assert not h.accepted[1].any() and h.accepted[0].all() and h.accepted[2].all()
    assert torch.isfinite(h.nis[[0, 2]]).all()
    # the other steps are what a filter without the gap computes up to the gap
    g, _, _ = _filter(hip, 1)
    assert torch.equal(g(zs[0]), h.means[1])
    ms, Ss = f.smooth(h)
    assert ms.shape == h.means.shape and torch.isfinite(ms).all() and torch.isfinite(Ss).all()
    assert not f.status.any()
    # a [T, N] mask and a device [T] vector: same beliefs as the skip, the model is called
    f2, meas2, _ = _filter(hip, 1)
    v = torch.tensor([True, False, True], device=hip)
    h2 = f2.filter(torch.stack([zs[0], torch.zeros_like(zs[1]), zs[2]]), valid=v)
    assert meas2.calls == 3
    assert torch.equal(h2.means, h.means) and torch.equal(h2.scale_trils, h.scale_trils)
    assert torch.equal(h2.accepted, h.accepted)
    f3, _, _ = _filter(hip, 1)
    h3 = f3.filter(torch.stack([zs[0], torch.zeros_like(zs[1]), zs[2]]),
                   valid=v.unsqueeze(1).expand(3, 8))
    assert torch.equal(h3.means, h.means)


# ----------------------------------------------------------------------------------------
def test_evidence_of_a_linear_gaussian_model(hip):
    """n = dz = 4, H = I, N = 4096 filters sharing one model, T = 5, observations drawn from the
    model: the UKF is exact, so sum_t loglik_t is the Kalman evidence.  Per filter:
    |error| <= max(2 x the largest error of the float32 numpy Kalman recursion against float64,
    1e-4 |evidence|) (the rule of conftest.param_grads_vs_truth); every filter is checked.  The
    noise scales keep |evidence| >= 1 (asserted on the float64 values), so the floor is a
    relative bound.  The mean NIS over filters and steps is within 5 sigma of the chi-square
    mean: 5 sqrt(2 dz / (N T)) = 0.0988 of dz; the float64 reference first."""
    from pinn_kalman.ukf import SquareRootUKF
    n, N, T = 4, 4096, 5
    rng = np.random.default_rng(2024)
    F = np.eye(n) + 0.3 * rng.standard_normal((n, n)) / math.sqrt(n)
    F = (F * 0.9 / np.abs(np.linalg.eigvals(F)).max()).astype(np.float32)  # spectral radius 0.9
    assert np.abs(np.linalg.eigvals(F.astype(np.float64))).max() < 1
    q, r, p0 = np.float32(0.02), np.float32(0.05), np.float32(0.3)
    Q, Rm, P0 = (float(v) ** 2 * np.eye(n) for v in (q, r, p0))
    m0 = rng.standard_normal((N, n)).astype(np.float32)
    x = m0 + float(p0) * rng.standard_normal((N, n))
    zs = []
    for _ in range(T):
        x = x @ F.T.astype(np.float64) + float(q) * rng.standard_normal((N, n))
        zs.append((x + float(r) * rng.standard_normal((N, n))).astype(np.float32))
    zs = np.stack(zs)
    ll64, nis64, _ = R.kalman_evidence(F, np.eye(n), Q, Rm, m0, P0, zs)
    ll32, _, _ = R.kalman_evidence(F, np.eye(n), Q, Rm, m0, P0, zs, dtype=np.float32)
    ev64 = ll64.sum(0)
    assert np.abs(ev64).min() >= 1, "input family: an evidence close to zero"
    band = 5 * math.sqrt(2 * n / (N * T))
    assert abs(nis64.mean() - n) <= band, f"float64 mean NIS {nis64.mean():.4f}"

    Fd = torch.from_numpy(F).to(hip)
    eye = torch.eye(n, device=hip)
    Qf, Rf = (float(q) * eye).expand(N, n, n), (float(r) * eye).expand(N, n, n)
    filt = SquareRootUKF(lambda x, u: ((x.unsqueeze(1) * Fd).sum(-1), Qf),
                         lambda x: (x.clone(), Rf), diagnostics=True)
    filt.initialize_beliefs(torch.from_numpy(m0).to(hip),
                            scale_tril=(float(p0) * eye).expand(N, n, n))
    h = filt.filter(torch.from_numpy(zs).to(hip))
    assert not filt.status.any() and h.accepted.all()
    ev = h.logliks.double().sum(0).cpu().numpy()
    e32 = float(np.abs(ll32.astype(np.float64).sum(0) - ev64).max())
    tol = np.maximum(2 * e32, 1e-4 * np.abs(ev64))
    err = np.abs(ev - ev64)
    i = int(np.argmax(err / tol))
    record_err("ukf evidence, linear-Gaussian, worst of 4096 filters", err[i], tol[i])
    print(f"evidence: worst err {err[i]:.3e} tol {tol[i]:.3e} (float32 Kalman {e32:.3e}); "
          f"max err {err.max():.3e}")
    assert (err <= tol).all(), f"{int((err > tol).sum())} filters off: {err[i]:.3e} > {tol[i]:.3e}"
    mean_nis = float(h.nis.double().mean())
    record_err("ukf mean NIS - dz, linear-Gaussian", abs(mean_nis - n), band)
    print(f"mean NIS {mean_nis:.4f} (float64 {nis64.mean():.4f}), band {band:.4f}")
    assert abs(mean_nis - n) <= band


# ----------------------------------------------------------------------------------------
def _field_case(hip, mask=None):
    from configs.pinn import pinn_pde
    from conftest import small_config
    from pinn_kalman.ukf import UKF
    from pinn_kalman.ukf_utils import patch
    c = small_config(pinn_pde.get_config)
    c.kf.patch_size = 4
    c.device = hip
    rng = np.random.default_rng(4)
    T, B, size = 2, 2, 16
    fields = np.concatenate([
        rng.uniform(0.1, 1.0, (B, 1, size, size)),
        rng.uniform(0.05, 0.5, (B, 2, size, size)) * rng.choice([-1, 1], (B, 2, size, size)),
        rng.normal(0, 0.01, (B, 1, size, size))], 1).astype(np.float32)
    obs = torch.from_numpy(np.stack([
        fields + rng.normal(0, 1e-3, fields.shape).astype(np.float32) for _ in range(T)]))
    filt = UKF(c, compat=False, mask=mask, diagnostics=True)
    filt.initialize(patch(torch.from_numpy(fields), 4).to(hip), var=1e-6)
    return c, filt, obs.to(hip), (T, B)


def test_fields(hip):
    c, filt, obs, (T, B) = _field_case(hip)
    out = filt.filter(obs)
    assert out.shape == (T, B, 4, 16, 16) and torch.isfinite(out).all()
    h = filt.history
    assert h.nis.shape == h.logliks.shape == (T, 4 * B * 16)
    maps, ll = filt.nis_maps().cpu(), filt.log_likelihood().cpu()
    assert maps.shape == (T, B, 4, 4, 4) and ll.shape == (T, B)
    nis, logliks = h.nis.cpu(), h.logliks.cpu()
    assert torch.isfinite(nis).all() and torch.isfinite(logliks).all()
    for t in range(T):
        for b in range(B):
            s = 0.
            for ch in range(4):
                for i in range(4):
                    for j in range(4):
                        row = (ch * B + b) * 16 + i * 4 + j  # (channel, sample, patch) rows
                        assert maps[t, b, ch, i, j] == nis[t, row]
                        s += float(logliks[t, row])
            assert float(ll[t, b]) == pytest.approx(s, rel=1e-5)
    # a sample's missing frame: its rows keep the prediction, the other sample is untouched
    c2, f2, _, _ = _field_case(hip)
    valid = torch.tensor([[True, True], [True, False]], device=hip)
    out2 = f2.filter(obs, valid=valid)
    assert torch.equal(out2[0], out[0]) and torch.equal(out2[1, 0], out[1, 0])
    acc = f2.history.accepted.reshape(T, 4, B, 16)
    assert acc[0].all() and acc[1, :, 0].all() and not acc[1, :, 1].any()
    assert torch.isnan(f2.log_likelihood()[1, 1]) and torch.isfinite(f2.log_likelihood()[1, 0])
    from pinn_kalman.ukf import UKF
    with pytest.raises(RuntimeError, match="diagnostics"):
        UKF(c).nis_maps()


def test_fields_under_a_mask(hip):
    """Patch (0, 0) of the density channel fully unobserved: zero deviation, zero innovation,
    S_z = r I with r the measurement model's factor entry (module docstring)."""
    mask = torch.ones(16, 16)
    mask[:4, :4] = 0
    mask[5, 9] = 0
    c, filt, obs, (T, B) = _field_case(hip, mask)
    filt.filter(obs)
    maps = filt.nis_maps().cpu()
    ll = filt.history.logliks.reshape(T, 4, B, 4, 4).transpose(1, 2).cpu()
    r = float(np.float32(c.inverse.variance))
    want = -0.5 * 16 * math.log(2 * math.pi * r * r)
    for t in range(T):
        for b in range(B):
            assert maps[t, b, 0, 0, 0] == 0
            assert float(ll[t, b, 0, 0, 0]) == pytest.approx(want, rel=1e-6)
    assert (maps[:, :, 0, 1:, :] > 0).all() and (maps[:, :, 1:] > 0).all()


def test_pinn_kf_reports_its_step(hip):
    from configs.pinn import pinn_pde
    from conftest import build_pinn_weights, full_pinn_config, make_pinn_inputs
    from pinn_kalman.pinn import B_PINN, PINN
    from pinn_kalman.ukf import PINN_KF
    c = full_pinn_config(pinn_pde.get_config)
    f1, f2, x, y, t, _ = (v.to(hip) for v in make_pinn_inputs(c, 1))
    c.device = hip
    c.model.bpinn_moped_delta = 2.0
    bp = B_PINN(c, build_pinn_weights(PINN, c))
    g = torch.Generator().manual_seed(4)
    v0 = (0.1 * torch.randn(1, 2, 64, 64, generator=g)).to(hip)
    p0 = (0.1 * torch.randn(1, 1, 64, 64, generator=g)).to(hip)
    kf = PINN_KF(c, diagnostics=True)
    kf.pinn.load_state_dict(bp.state_dict())
    kf.pinn.reseed(6)
    kf.initialize(f1[:1], v0, p0)
    out = kf(x[:1], y[:1], t[:1], f2[:1], n=4)
    u = kf.ukf.ukf
    assert torch.isfinite(out).all() and not u.status.any()
    assert u.nis.shape == u.loglik.shape == u.accepted.shape == (256,)
    assert torch.isfinite(u.nis).all() and torch.isfinite(u.loglik).all() and u.accepted.all()
