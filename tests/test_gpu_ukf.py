"""GPU: the square-root UKF kernels (csrc/ukf.hip) behind op.ukf and pinn_kalman.ukf against
the CPU restatement tests/ukf_ref.py (anchored to the closed-form Kalman filter in
test_ukf_host.py).

Gate of every float comparison (the project's rule, conftest.param_grads_vs_truth and the
1e-5 of the op tests): with the float64 restatement fed the same float32 inputs as truth,
err(kernel) <= max(1e-5, 2 x err(restatement run in float32)); means relative to max|mean64|,
factors compared as S S^T relative to max|P64|.  Structure (exact zeros above the diagonal, a
positive diagonal, status 0) is checked separately and exactly."""
import functools
import math

import numpy as np
import pytest
import torch

import ukf_ref
from conftest import record_err
from op import ukf as K

pytestmark = pytest.mark.gpu

TRIPLES = [(1., 0., 0.), (0.5, 2., 0.), (1., 2., 1.)]
DIMS = [(4, 4), (4, 3), (9, 9), (16, 16), (64, 64)]  # (n, obs dim)


def _gate(what, got, ref64, ref32):
    scale = float(ref64.abs().max())
    err = float((got.double().cpu() - ref64).abs().max()) / scale
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    tol = max(1e-5, 2 * e32)
    record_err(what, err, tol)
    print(f"{what}: err {err:.3e}  float32 restatement {e32:.3e}  tol {tol:.3e}")
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e} (float32 restatement {e32:.3e})"


def _cov(S):
    S = S.double().cpu()
    return S @ S.transpose(1, 2)


def _structure(S, status):
    S = S.cpu()
    assert (S.triu(1) == 0).all(), "non-zero above the diagonal"
    assert (torch.diagonal(S, dim1=1, dim2=2) > 0).all(), "diagonal not positive"
    assert status.dtype == torch.int32 and status.cpu().tolist() == [0] * S.shape[0]


def _models(n, dz, g):
    F = torch.eye(n) + 0.3 * torch.randn(n, n, generator=g) / math.sqrt(n)
    H = (torch.eye(n) + 0.3 * torch.randn(n, n, generator=g) / math.sqrt(n))[:dz]

    def f(x):
        return x @ F.to(x).T + 0.2 * torch.sin(3 * x)

    def h(x):
        return x @ H.to(x).T + 0.1 * torch.tanh(x)[:, :dz] ** 2
    return f, h


def _tril(N, d, g, off, diag):
    return (off * torch.randn(N, d, d, generator=g) / math.sqrt(d)).tril() + diag * torch.eye(d)


@functools.lru_cache(maxsize=None)
def _case(n, dz, abk, N=4, groups=2):
    """Float32 inputs of one predict and one update, shared by the root and update tests, with
    their float64 / float32 restatement results (computed once, never modified)."""
    g = torch.Generator().manual_seed(1000 * n + 10 * dz + int(2 * abk[0] + abk[2]))
    gamma, wm0, wc0, wi = ukf_ref.merwe(n, *abk)
    f, h = _models(n, dz, g)
    m = 0.5 * torch.randn(N, n, generator=g)
    S, Q, R = _tril(N, n, g, 0.1, 0.3), _tril(N, n, g, 0.05, 0.05), _tril(N, dz, g, 0.05, 0.2)
    z = 0.5 * torch.randn(N, dz, generator=g)
    X = ukf_ref.sigma(m, S, gamma, groups)
    Y = f(X)  # float32: the same propagated points go to the kernel and both restatements
    c = dict(n=n, dz=dz, N=N, groups=groups, w=(gamma, wm0, wc0, wi), m=m, S=S, Q=Q, R=R, z=z,
             X=X, Y=Y)
    c["pred64"] = ukf_ref.root(Y.double(), Q.double(), n, wm0, wc0, wi, groups)
    c["pred32"] = ukf_ref.root(Y, Q, n, wm0, wc0, wi, groups)
    # the update's inputs: the float32 prior, its redrawn points and their measurement
    m1, S1, _ = c["pred32"]
    X2 = ukf_ref.sigma(m1, S1, gamma, groups)
    Z = h(X2)
    zm, zt, zf = ukf_ref.root(Z, R, n, wm0, wc0, wi, groups)
    c.update(m1=m1, S1=S1, X2=X2, Z=Z, zm=zm, zt=zt)
    c["z64"] = ukf_ref.root(Z.double(), R.double(), n, wm0, wc0, wi, groups)
    c["z32"] = (zm, zt, zf)
    args = (m1, S1, X2, Z, zm, zt, z)
    c["up64"] = ukf_ref.update(*(a.double() for a in args), wc0, wi, groups)
    c["up32"] = ukf_ref.update(*args, wc0, wi, groups)
    for k in ("pred64", "pred32", "z64", "up64", "up32"):
        assert not c[k][2].any(), f"restatement flagged a filter in {k}"
    return c


@pytest.mark.parametrize("groups,N", [(1, 4), (1, 5), (1, 12), (4, 4), (4, 12)])
@pytest.mark.parametrize("n", [4, 9, 16, 64])
def test_sigma_points_bit_exact(hip, n, groups, N):
    """(1, 0, 0): gamma = sqrt(n) = 2, 3, 4, 8; the kernel rounds gamma * S and then the sum, as
    torch's float32 `m +- gamma * S` does, so the points are equal bit for bit."""
    g = torch.Generator().manual_seed(n * 100 + N)
    gamma = K.merwe_weights(n)[0]
    m = torch.randn(N, n, generator=g)
    S = _tril(N, n, g, 0.1, 0.3)
    got = K.sigma_points(m.to(hip), S.to(hip), gamma, groups).cpu()
    idx = K.point_rows(N, n, groups)
    assert torch.equal(got[idx[:, 0]], m)
    gS = (gamma * S).transpose(1, 2)  # [N, column, :]
    assert torch.equal(got[idx[:, 1:n + 1]], m.unsqueeze(1) + gS)
    assert torch.equal(got[idx[:, n + 1:]], m.unsqueeze(1) - gS)
    assert torch.equal(got, ukf_ref.sigma(m, S, gamma, groups))


@pytest.mark.parametrize("abk", TRIPLES)
@pytest.mark.parametrize("n,dz", DIMS)
def test_unscented_root_vs_float64(hip, n, dz, abk):
    c = _case(n, dz, abk)
    _, wm0, wc0, wi = c["w"]
    # the predict root (d = n) and the measurement root (d = dz, sigma count from n)
    for tag, pts, noise, k64, k32 in (("pred", c["Y"], c["Q"], "pred64", "pred32"),
                                      ("meas", c["Z"], c["R"], "z64", "z32")):
        mean, S, status = K.unscented_root(pts.to(hip), noise.to(hip), n, wm0, wc0, wi,
                                           c["groups"])
        assert mean.shape == (c["N"], pts.shape[1]) and S.shape == noise.shape
        _structure(S, status)
        what = f"ukf.root[{tag}] n={n} d={pts.shape[1]} abk={abk}"
        _gate(what + " mean", mean, c[k64][0], c[k32][0])
        _gate(what + " cov", _cov(S), _cov(c[k64][1]), _cov(c[k32][1]))


@pytest.mark.parametrize("abk", TRIPLES)
@pytest.mark.parametrize("n,dz", DIMS)
def test_kalman_update_vs_float64(hip, n, dz, abk):
    c = _case(n, dz, abk)
    _, _, wc0, wi = c["w"]
    args = [c[k].to(hip) for k in ("m1", "S1", "X2", "Z", "zm", "zt", "z")]
    mean, S, status = K.kalman_update(*args, wc0, wi, c["groups"])
    assert mean.shape == (c["N"], n) and S.shape == (c["N"], n, n)
    _structure(S, status)
    what = f"ukf.update n={n} dz={dz} abk={abk}"
    _gate(what + " mean", mean, c["up64"][0], c["up32"][0])
    _gate(what + " cov", _cov(S), _cov(c["up64"][1]), _cov(c["up32"][1]))


def _chain_setup(hip, abk):
    n, N = 16, 3
    g = torch.Generator().manual_seed(77)
    f, h = _models(n, n, g)
    m, S = 0.5 * torch.randn(N, n, generator=g), _tril(N, n, g, 0.1, 0.3)
    Q, R = _tril(N, n, g, 0.05, 0.05), _tril(N, n, g, 0.05, 0.2)
    zs = 0.5 * torch.randn(3, N, n, generator=g)
    from pinn_kalman.ukf import SquareRootUKF
    Qd, Rd = Q.to(hip), R.to(hip)
    filt = SquareRootUKF(lambda x, u: (f(x), Qd), lambda x: (h(x), Rd), *abk)
    return n, f, h, m, S, Q, R, zs, filt, Qd, Rd


@pytest.mark.parametrize("abk", TRIPLES)
def test_three_chained_steps(hip, abk):
    n, f, h, m, S, Q, R, zs, filt, Qd, Rd = _chain_setup(hip, abk)
    runs = []
    for _ in range(2):
        filt.initialize_beliefs(m.to(hip), scale_tril=S.to(hip))
        outs = [filt(zs[t].to(hip)).clone() for t in range(3)]
        runs.append((outs, filt.belief_scale_tril.clone(), filt.status.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b), "two identical runs differ"
    assert torch.equal(runs[0][1], runs[1][1])
    # the same sequence of op.ukf calls by hand
    gamma, wm0, wc0, wi = K.merwe_weights(n, *abk)
    mh, Sh = m.to(hip), S.to(hip)
    for t in range(3):
        mh, Sh, _ = K.unscented_root(f(K.sigma_points(mh, Sh, gamma)), Qd, n, wm0, wc0, wi)
        X = K.sigma_points(mh, Sh, gamma)
        Z = h(X)
        zm, zt, _ = K.unscented_root(Z, Rd, n, wm0, wc0, wi)
        mh, Sh, _ = K.kalman_update(mh, Sh, X, Z, zm, zt, zs[t].to(hip), wc0, wi)
        assert torch.equal(mh, runs[0][0][t]), f"forward != hand-made sequence at step {t}"
    assert torch.equal(Sh, runs[0][1])
    _structure(Sh, runs[0][2])
    # against the restatement chains
    ref = {}
    for dt in (torch.float64, torch.float32):
        mm, SS = m.to(dt), S.to(dt)
        for t in range(3):
            o = ukf_ref.step(mm, SS, lambda x: (f(x), Q.to(dt)), lambda x: (h(x), R.to(dt)),
                             zs[t].to(dt), abk)
            assert not o["flag"].any()
            mm, SS = o["m_post"], o["S_post"]
        ref[dt] = (mm, SS)
    _gate(f"ukf.chain3 abk={abk} mean", mh, ref[torch.float64][0], ref[torch.float32][0])
    _gate(f"ukf.chain3 abk={abk} cov", _cov(Sh), _cov(ref[torch.float64][1]),
          _cov(ref[torch.float32][1]))


def _pipeline(hip, m, S, Q, R, z, abk):
    """sigma -> element-wise dynamics -> root -> sigma -> element-wise measurement -> root ->
    update, all filters in one call of each kernel."""
    n = m.shape[1]
    gamma, wm0, wc0, wi = K.merwe_weights(n, *abk)
    m, S, Q, R, z = (t.to(hip) for t in (m, S, Q, R, z))
    X = K.sigma_points(m, S, gamma)
    m1, S1, s1 = K.unscented_root(X + 0.2 * torch.sin(3 * X), Q, n, wm0, wc0, wi)
    X2 = K.sigma_points(m1, S1, gamma)
    Z = X2 + 0.1 * torch.tanh(X2) ** 2
    zm, zt, s2 = K.unscented_root(Z, R, n, wm0, wc0, wi)
    m2, S2, s3 = K.kalman_update(m1, S1, X2, Z, zm, zt, z, wc0, wi)
    return [t.cpu() for t in (X, m1, S1, X2, zm, zt, m2, S2, s1 | s2 | s3)]


def test_a_nan_filter_leaves_the_others_bit_identical(hip):
    n, N, bad = 16, 4, 1
    g = torch.Generator().manual_seed(5)
    m, S = 0.5 * torch.randn(N, n, generator=g), _tril(N, n, g, 0.1, 0.3)
    Q, R = _tril(N, n, g, 0.05, 0.05), _tril(N, n, g, 0.05, 0.2)
    z = 0.5 * torch.randn(N, n, generator=g)
    good = _pipeline(hip, m, S, Q, R, z, (0.5, 2., 0.))
    m_nan = m.clone()
    m_nan[bad] = float("nan")
    got = _pipeline(hip, m_nan, S, Q, R, z, (0.5, 2., 0.))  # the call returns
    keep = torch.tensor([i for i in range(N) if i != bad])
    rows = K.point_rows(N, n)[keep].reshape(-1)
    for i, (a, b) in enumerate(zip(good, got)):
        sel = rows if a.shape[0] == (2 * n + 1) * N else keep
        assert torch.equal(a[sel], b[sel]), f"output {i} of a healthy filter changed"
    assert good[-1].tolist() == [0] * N and got[-1][keep].tolist() == [0] * (N - 1)
    assert torch.isnan(got[6][bad]).all()


def test_a_lost_downdate_is_flagged_finite_and_isolated(hip):
    """wc0 = -0.25 and filter 2's Y_0 displaced by 100: the point-0 downdate removes 2500 from
    a covariance of order 0.1 and loses positive definiteness.  The weights go to the kernel
    directly with wm0 = 0: with the Merwe-consistent wm0 = -3 of (0.5, 2, 0) the displaced
    point would drag the mean along and the weighted sum would stay positive definite (the
    shift d enters as 36 d d^T - 4 d d^T)."""
    n, N, bad = 16, 4, 2
    wm0, wc0, wi = 0., -0.25, 1. / (2 * n)
    g = torch.Generator().manual_seed(6)
    m, S, Q = 0.5 * torch.randn(N, n, generator=g), _tril(N, n, g, 0.1, 0.3), _tril(N, n, g, 0.05,
                                                                                  0.05)
    X = ukf_ref.sigma(m, S, 4., 1)
    Y = X + 0.2 * torch.sin(3 * X)
    Yb = Y.clone()
    Yb[K.point_rows(N, n)[bad, 0]] += 100.
    m0, S0, st0 = (t.cpu() for t in K.unscented_root(Y.to(hip), Q.to(hip), n, wm0, wc0, wi))
    m1, S1, st1 = (t.cpu() for t in K.unscented_root(Yb.to(hip), Q.to(hip), n, wm0, wc0, wi))
    keep = torch.tensor([i for i in range(N) if i != bad])
    assert torch.equal(m0[keep], m1[keep]) and torch.equal(S0[keep], S1[keep])
    assert st0.tolist() == [0] * N and st1.tolist() == [0, 0, 1, 0]
    assert torch.isfinite(m1).all() and torch.isfinite(S1).all()
    assert (S1.triu(1) == 0).all()
    for dt in (torch.float64, torch.float32):
        _, Sr, flag = ukf_ref.root(Yb.to(dt), Q.to(dt), n, wm0, wc0, wi)
        assert flag.tolist() == [False, False, True, False] and torch.isfinite(Sr).all()
    # the same through the update kernel: an innovation factor far too small for the gain
    gamma = 4.
    X2 = ukf_ref.sigma(m, S, gamma, 1)
    zt = _tril(N, n, g, 0.1, 0.8)  # S_z S_z^T well above P: the healthy downdates succeed
    zt_b = zt.clone()
    zt_b[bad] *= 1e-3
    z = 0.5 * torch.randn(N, n, generator=g)
    a = [t.to(hip) for t in (m, S, X2, X2, m)]
    u0 = [t.cpu() for t in K.kalman_update(*a, zt.to(hip), z.to(hip), 0., wi)]
    u1 = [t.cpu() for t in K.kalman_update(*a, zt_b.to(hip), z.to(hip), 0., wi)]
    assert torch.equal(u0[0][keep], u1[0][keep]) and torch.equal(u0[1][keep], u1[1][keep])
    assert u1[2][bad] == 1 and u1[2][keep].tolist() == [0] * (N - 1)
    assert torch.isfinite(u1[0]).all() and torch.isfinite(u1[1]).all()
    flag = ukf_ref.update(m, S, X2, X2, m, zt_b, z, 0., wi)[2]
    assert flag.tolist() == [False, False, True, False]


@pytest.mark.parametrize("compat", [True, False])
def test_ukf_on_ns_dynamics_stagewise(hip, compat):
    """UKF(config): image 16, patch 8, B = 1 -> 16 filters of n = 64, 129 sigma fields of 16^2
    through NSDynamics.  Stage by stage, so the stencil's sensitivity stays out of the
    tolerance.

    Under compat=True the stencil's unbind-stride quirk mixes neighbouring sigma fields, which
    inflates the predicted covariance from 1e-6 to O(1) (largest eigenvalue 2.5 measured);
    the velocity and pressure filters then meet a measurement factor of 1e-4 I, a posterior
    2.5e8 times smaller than the prior, which float32 inputs cannot carry: the float64
    restatement fed the kernel's float32 inputs flags exactly those 12 filters as not positive
    definite, and so do the float32 restatement and the kernel.  Flagged filters' outputs are
    unspecified by contract (finite is checked); the update is compared on the filters the
    float64 restatement does not flag, and the flags themselves must agree.  Under
    compat=False nothing is flagged and every filter is compared."""
    from configs.pinn import pinn_pde
    from pinn_kalman.ukf import UKF
    from pinn_kalman.ukf_utils import patch
    c = pinn_pde.get_config()
    c.data.image_size = 16
    c.device = hip
    rng = np.random.default_rng(4)
    B, size, n, N = 1, 16, 64, 16
    fields = torch.from_numpy(np.concatenate([
        rng.uniform(0.1, 1.0, (B, 1, size, size)),
        rng.uniform(0.05, 0.5, (B, 2, size, size)) * rng.choice([-1, 1], (B, 2, size, size)),
        rng.normal(0, 0.01, (B, 1, size, size))], 1).astype(np.float32))
    obs = fields + torch.from_numpy(rng.normal(0, 1e-3, fields.shape).astype(np.float32))
    x0 = patch(fields, 8)
    filt = UKF(c, compat=compat)
    assert filt.dynamic.compat is compat
    seen = {}
    filt.dynamic.register_forward_hook(
        lambda mod, args, out: seen.update(dyn_in=args[0].clone(), dyn_out=out[0].clone(),
                                           dyn_q=out[1]))
    filt.initialize(x0, var=1e-6)
    S0 = filt.ukf.belief_scale_tril.clone()
    out = filt(obs.to(hip))
    assert out.shape == (1, 4, 16, 16) and torch.isfinite(out).all()
    gamma, wm0, wc0, wi = K.merwe_weights(n)
    # 1. the rows NSDynamics received: torch's float32 sigma points in (g, s, r) order
    assert torch.equal(seen["dyn_in"].cpu(), ukf_ref.sigma(x0, S0.cpu(), gamma, 4))
    assert torch.isfinite(seen["dyn_out"]).all()
    # 2. the root of NSDynamics' own output
    Y = seen["dyn_out"]
    Qf = seen["dyn_q"][K.point_rows(N, n, 4)[:, 0].to(hip)]
    m1, S1, st = K.unscented_root(Y, Qf, n, wm0, wc0, wi, 4)
    _structure(S1, st)
    r64 = ukf_ref.root(Y.cpu().double(), Qf.cpu().double(), n, wm0, wc0, wi, 4)
    r32 = ukf_ref.root(Y.cpu(), Qf.cpu(), n, wm0, wc0, wi, 4)
    _gate(f"ukf.ns compat={compat} root mean", m1, r64[0], r32[0])
    _gate(f"ukf.ns compat={compat} root cov", _cov(S1), _cov(r64[1]), _cov(r32[1]))
    # 3. the update on the same inputs
    X2 = K.sigma_points(m1, S1, gamma, 4)
    Z, R = filt.measurement(X2)
    Rf = R[K.point_rows(N, n, 4)[:, 0].to(hip)]
    zm, zt, st = K.unscented_root(Z, Rf, n, wm0, wc0, wi, 4)
    _structure(zt, st)
    z = patch(obs, 8).to(hip)
    m2, S2, st = K.kalman_update(m1, S1, X2, Z, zm, zt, z, wc0, wi, 4)
    assert torch.isfinite(m2).all() and torch.isfinite(S2).all()
    assert (S2.triu(1) == 0).all()
    args = [t.cpu() for t in (m1, S1, X2, Z, zm, zt, z)]
    u64 = ukf_ref.update(*(a.double() for a in args), wc0, wi, 4)
    u32 = ukf_ref.update(*args, wc0, wi, 4)
    assert st.cpu().bool().tolist() == u64[2].tolist() == u32[2].tolist()
    ok = ~u64[2]
    assert ok[:4].all() and (compat or ok.all())  # density filters always; all without the quirk
    assert (torch.diagonal(S2, dim1=1, dim2=2).cpu()[ok] > 0).all()
    _gate(f"ukf.ns compat={compat} update mean", m2.cpu()[ok], u64[0][ok], u32[0][ok])
    _gate(f"ukf.ns compat={compat} update cov", _cov(S2)[ok], _cov(u64[1])[ok], _cov(u32[1])[ok])
    # 4. UKF.forward is exactly that composition
    from pinn_kalman.ukf_utils import unpatch
    assert torch.equal(out, unpatch(m2, 8, 16, 4))
    assert torch.equal(filt.ukf.belief_scale_tril, S2)
    assert torch.equal(filt.ukf.status, st)
