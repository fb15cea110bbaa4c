"""CPU: the host side of the square-root UKF -- Merwe weights, the (g, s, r) row layout, the
C-ABI argument checks without a device, the measurement model's shapes -- and the anchor of
the restatement tests/ukf_ref.py (the yardstick of the GPU tests) to the closed-form Kalman
filter."""
import math

import pytest
import torch

import ukf_ref
from op import ukf as K

TRIPLES = [(1., 0., 0.), (0.5, 2., 0.), (1., 2., 1.)]  # no point-0 term / downdate / update


@pytest.mark.parametrize("n,gamma", [(4, 2.), (16, 4.), (64, 8.)])
def test_merwe_weights_reference_parameters(n, gamma):
    g, wm0, wc0, wi = K.merwe_weights(n)
    assert (g, wm0, wc0) == (gamma, 0., 0.) and wi == 1 / (2 * n)
    assert K.merwe_weights(n) == pytest.approx(ukf_ref.merwe(n), abs=0)


def test_merwe_weights_scaled():
    assert K.merwe_weights(16, 0.5, 2., 0.) == (2., -3., -0.25, 0.125)
    for n in (1, 4, 9, 64):
        for abk in TRIPLES + [(0.1, 2., 3.)]:
            _, wm0, _, wi = K.merwe_weights(n, *abk)
            assert wm0 + 2 * n * wi == pytest.approx(1., abs=1e-9)
    with pytest.raises(ValueError):
        K.merwe_weights(4, 1., 0., -4.)  # n + lam = 0
    with pytest.raises(ValueError):
        K.merwe_weights(4, 1., 0., -5.)
    with pytest.raises(ValueError):
        K.merwe_weights(4, 0., 0., 0.)


def _linear_case(n, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    N, sq = 3, math.sqrt(n)
    F = torch.eye(n, dtype=torch.float64) + 0.3 * rn(N, n, n) / sq
    H = torch.eye(n, dtype=torch.float64) + 0.3 * rn(N, n, n) / sq
    eye = torch.eye(n, dtype=torch.float64)
    S0 = (0.1 * rn(N, n, n) / sq).tril() + 0.3 * eye
    Q = (0.05 * rn(N, n, n) / sq).tril() + 0.05 * eye
    R = (0.05 * rn(N, n, n) / sq).tril() + 0.2 * eye
    return N, F, H, S0, Q, R, rn(N, n), rn(3, N, n)


@pytest.mark.parametrize("abk", TRIPLES)
@pytest.mark.parametrize("n", [4, 16, 64])
def test_restatement_equals_textbook_kalman_filter_on_linear_models(n, abk):
    """Linear f(x) = F x, h(x) = H x: the unscented transform is exact, so three predict +
    update steps of the float64 restatement equal P = F P F^T + Q Q^T, K = P H^T (H P H^T +
    R R^T)^-1, m += K (z - H m), P -= K S K^T to rounding (<= 1e-12), for all three branches of
    the point-0 term."""
    N, F, H, S0, Q, R, m0, zs = _linear_case(n, 10 * n + int(abk[0] * 2 + abk[2]))
    idx = ukf_ref.rows(N, n)

    def per_row(M):  # [N, n, n] -> the matrix of each point row's filter
        out = torch.empty((2 * n + 1) * N, n, n, dtype=M.dtype)
        out[idx.reshape(-1)] = M.unsqueeze(1).expand(-1, 2 * n + 1, -1, -1).reshape(-1, n, n)
        return out
    Fr, Hr = per_row(F), per_row(H)
    dyn = lambda X: ((Fr @ X.unsqueeze(2)).squeeze(2), Q)
    meas = lambda X: ((Hr @ X.unsqueeze(2)).squeeze(2), R)
    m, S = m0, S0
    mk, P = m0, S0 @ S0.transpose(1, 2)
    for t in range(3):
        out = ukf_ref.step(m, S, dyn, meas, zs[t], abk)
        assert not out["flag"].any()
        m, S = out["m_post"], out["S_post"]
        mk = (F @ mk.unsqueeze(2)).squeeze(2)
        P = F @ P @ F.transpose(1, 2) + Q @ Q.transpose(1, 2)
        Sk = H @ P @ H.transpose(1, 2) + R @ R.transpose(1, 2)
        Kg = P @ H.transpose(1, 2) @ torch.linalg.inv(Sk)
        mk = mk + (Kg @ (zs[t] - (H @ mk.unsqueeze(2)).squeeze(2)).unsqueeze(2)).squeeze(2)
        P = P - Kg @ Sk @ Kg.transpose(1, 2)
        assert (m - mk).abs().max() <= 1e-12
        assert (S @ S.transpose(1, 2) - P).abs().max() <= 1e-12
        assert (S.triu(1) == 0).all() and (torch.diagonal(S, dim1=1, dim2=2) > 0).all()


def test_restatement_flags_a_lost_downdate_and_stays_finite():
    S = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    x = torch.tensor([[0.1, 0.2, 0.3], [0.5, 2.0, 0.3]], dtype=torch.float64)
    S1, flag = ukf_ref.rank1(S, x, -1)
    assert flag.tolist() == [False, True] and torch.isfinite(S1).all()
    assert (S1[0] @ S1[0].T - (torch.eye(3) - torch.outer(x[0], x[0]))).abs().max() < 1e-15


@pytest.mark.parametrize("groups", [1, 4])
def test_point_row_layout(groups):
    N, n = 8, 3
    got = K.point_rows(N, n, groups)
    ng = N // groups
    for i in range(N):
        for s in range(2 * n + 1):
            assert got[i, s] == ((i // ng) * (2 * n + 1) + s) * ng + i % ng
    assert torch.equal(got, ukf_ref.rows(N, n, groups))
    assert sorted(got.reshape(-1).tolist()) == list(range(N * (2 * n + 1)))  # a permutation
    with pytest.raises(ValueError):
        K.point_rows(6, 3, 4)


def test_unpatch_of_grouped_rows_gives_one_field_per_sigma_point():
    """groups = 4, p = 2, 4 x 4 image, B = 2: unpatch of rows in (g, s, r) order yields, for
    each (s, b), the field made of every patch's s-th sigma point."""
    from pinn_kalman.ukf_utils import patch, unpatch
    B, p, size, n = 2, 2, 4, 4
    ns = 2 * n + 1
    g = torch.Generator().manual_seed(0)
    fields = torch.randn(ns, B, 4, size, size, generator=g)  # field (s, b): sigma point s
    N = 4 * B * (size // p) ** 2
    idx = K.point_rows(N, n, 4)
    pts = torch.empty(ns * N, p * p)
    for s in range(ns):
        pts[idx[:, s]] = patch(fields[s], p)  # filter rows (c, b, patch) of sigma point s
    un = unpatch(pts, p, size, 4)
    assert un.shape == (ns * B, 4, size, size)
    assert torch.equal(un.reshape(ns, B, 4, size, size), fields)
    assert torch.equal(patch(un, p), pts)  # and patch() comes back in the same order


def test_abi_argument_errors_without_a_device():
    """Each entry point validates before any HIP call: n = 65, groups not dividing N and a null
    output return BPK_ERR_ARG with a message naming the argument (pointers are never
    dereferenced on the host; 8 stands for 'non-null')."""
    from op import _lib
    dll = _lib.lib.load()
    for name in ("sigma", "root", "update"):
        for kw, word in ((dict(N=4, n=65, d=4, groups=1, null_out=False), b"n = 65"),
                         (dict(N=4, n=4, d=4, groups=3, null_out=False), b"groups = 3"),
                         (dict(N=4, n=4, d=4, groups=1, null_out=True), b"NULL")):
            # one call at a time: bpk_last_error() holds the latest message
            o = None if kw["null_out"] else 8
            a = (kw["N"], kw["n"])
            if name == "sigma":
                rc = dll.bpk_ukf_sigma_points_f32(8, 8, o, *a, 2.0, kw["groups"], None)
            elif name == "root":
                rc = dll.bpk_ukf_root_f32(8, 8, o, 8, 8, *a, kw["d"], 0., 0., .125, kw["groups"],
                                          None)
            else:
                rc = dll.bpk_ukf_update_f32(8, 8, 8, 8, 8, 8, 8, o, 8, 8, *a, kw["d"], 0., .125,
                                            kw["groups"], None)
            msg = dll.bpk_last_error()
            assert rc == 1 and word in msg and b"ukf_" in msg, (name, kw, rc, msg)
    assert dll.bpk_ukf_root_f32(8, 8, 8, 8, 8, 4, 4, 65, 0., 0., .125, 1, None) == 1
    assert b"d = 65" in dll.bpk_last_error()
    assert dll.bpk_ukf_update_f32(8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 4, 4, 0, 0., .125, 1, None) == 1
    assert b"dz = 0" in dll.bpk_last_error()
    assert {"bpk_ukf_sigma_points_f32", "bpk_ukf_root_f32", "bpk_ukf_update_f32"} <= set(
        _lib.exported_symbols())


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    m, S = torch.zeros(4, 3), torch.eye(3).repeat(4, 1, 1)
    with pytest.raises(RuntimeError, match="HIP"):
        K.sigma_points(m, S, 2.0)
    with pytest.raises(RuntimeError, match="HIP"):
        K.unscented_root(torch.zeros(28, 3), S, 3, 0., 0., 1 / 6)
    with pytest.raises(RuntimeError, match="HIP"):
        K.kalman_update(m, S, torch.zeros(28, 3), torch.zeros(28, 3), m, S, m, 0., 1 / 6)


def _config(size=16):
    from configs.pinn import pinn_pde
    c = pinn_pde.get_config()
    c.data.image_size = size
    c.device = torch.device("cpu")
    return c


def test_identity_measure_shapes_and_uncertainty():
    from pinn_kalman.ukf_utils import IdentityKFMeasure, patch
    c = _config()
    h = IdentityKFMeasure(c)
    d, patches, nb = 64, 4, 3
    x = torch.randn(4 * nb * patches, d)
    z, f = h(x)
    assert z is x  # deterministic by default
    assert f.shape == (x.shape[0], d, d)
    v = c.inverse.variance
    assert torch.equal(f[0], torch.eye(d) * v) and torch.equal(f[-1], torch.eye(d) * v ** 2)
    with pytest.raises(AssertionError):
        h.update_uncertainty(torch.ones(1, 1, 16, 16), torch.ones(1, 1, 16, 16))
    with pytest.raises(AssertionError):
        h.update_uncertainty(torch.ones(1, 2, 16, 16), torch.ones(1, 2, 16, 16))
    with pytest.raises(AssertionError):
        h.update_uncertainty(torch.ones(2, 16, 16), torch.ones(1, 16, 16))
    uf = torch.rand(1, 2, 16, 16) + 0.1
    up = torch.rand(1, 1, 16, 16) + 0.1
    h.update_uncertainty(uf, up)
    z, f = h(x)
    q = nb * patches
    assert f.shape == (4 * q, d, d)
    assert torch.equal(f[:q], (torch.eye(d) * v).expand(q, -1, -1))
    assert torch.equal(f[q:3 * q], torch.diag_embed(patch(uf, 8).repeat(nb, 1)) ** 2)
    assert torch.equal(f[3 * q:], torch.diag_embed(patch(up, 8).repeat(nb, 1)) ** 2)
    zf, ff = h(x[:q], f_only=True)
    assert zf is x[:q] or torch.equal(zf, x[:q])
    assert ff.shape == (q, d, d) and torch.equal(ff[1], torch.eye(d) * v)
    torch.manual_seed(0)
    zn, _ = IdentityKFMeasure(c, noisy=True)(x)
    assert zn.shape == x.shape and not torch.equal(zn, x)


def test_filter_classes_import_and_validate_on_the_host():
    from pinn_kalman.ukf import UKF, SquareRootUKF
    from pinn_kalman.ukf_utils import NSDynamics
    c = _config()
    assert NSDynamics(c).compat is True and NSDynamics(c, compat=False).compat is False
    f = SquareRootUKF(lambda x, u: (x, None), lambda x: (x, None), groups=4)
    with pytest.raises(ValueError):
        f.initialize_beliefs(torch.zeros(6, 4), scale_tril=torch.eye(4).repeat(6, 1, 1))
    with pytest.raises(ValueError):
        f.initialize_beliefs(torch.zeros(8, 4))
    P = torch.tensor([[4., 2.], [2., 3.]]).repeat(4, 1, 1)
    f.initialize_beliefs(torch.zeros(4, 2), covariance=P)
    S = f.belief_scale_tril
    assert S.dtype == torch.float32 and torch.allclose(S @ S.transpose(1, 2), P, atol=1e-6)
    assert f.status.dtype == torch.int32 and f.status.tolist() == [0] * 4
    u = UKF(c)
    u.initialize(var=0.04)
    assert u.ukf.belief_mean.shape == (16, 64) and (u.ukf.belief_mean == 0.1).all()
    assert torch.equal(u.ukf.belief_scale_tril[3], torch.eye(64) * 0.1)  # default var = 0.01
    u.initialize(torch.zeros(16, 64), var=0.04)
    assert torch.allclose(u.ukf.belief_scale_tril[0], torch.eye(64) * 0.2)
    with pytest.raises(RuntimeError, match="HIP"):
        u(torch.zeros(1, 4, 16, 16))
