"""CPU: the innovation restatement tests/ukf_innov_ref.py against a direct evaluation of the
Gaussian density (explicit inverse and determinant, float64), the argument checks of
op.ukf.innovation and the ABI entry point, and the backward-compatible FilterHistory."""
import math

import numpy as np
import pytest
import torch

import ukf_innov_ref as R
from op import ukf as K


@pytest.mark.parametrize("dz", [1, 2, 5])
def test_restatement_equals_the_gaussian_density(dz):
    rng = np.random.default_rng(dz)
    N = 6
    S = np.tril(0.3 * rng.standard_normal((N, dz, dz))) + 1.5 * np.eye(dz)
    S[:, np.arange(dz), np.arange(dz)] = np.abs(np.diagonal(S, axis1=1, axis2=2)) + 0.2
    garbage = S + np.triu(rng.standard_normal((N, dz, dz)), 1)  # above the diagonal: ignored
    zm, z = rng.standard_normal((N, dz)), rng.standard_normal((N, dz))
    e, nis, ll, st = R.innovation(zm, garbage, z)
    assert st.tolist() == [0] * N and e.shape == (N, dz) and nis.shape == ll.shape == (N,)
    for i in range(N):
        P = S[i] @ S[i].T
        r = z[i] - zm[i]
        q = r @ np.linalg.inv(P) @ r
        dens = math.exp(-0.5 * q) / math.sqrt((2 * math.pi) ** dz * np.linalg.det(P))
        assert nis[i] == pytest.approx(q, rel=1e-12)
        assert ll[i] == pytest.approx(math.log(dens), rel=1e-12, abs=1e-12)
        assert e[i] == pytest.approx(np.linalg.inv(S[i]) @ r, rel=1e-12, abs=1e-14)


def test_restatement_status_contract():
    S = np.eye(3)[None].repeat(4, 0)
    S[1, 1, 1], S[2, 0, 0], S[3, 2, 2] = 0., -1., np.nan
    e, nis, ll, st = R.innovation(np.zeros((4, 3)), S, np.ones((4, 3)))
    assert st.tolist() == [0, 1, 1, 1]
    assert np.isnan(e[1:]).all() and np.isnan(nis[1:]).all() and np.isnan(ll[1:]).all()
    assert nis[0] == 3. and ll[0] == pytest.approx(-0.5 * (3 + 3 * math.log(2 * math.pi)))


def test_kalman_evidence_is_the_joint_density_of_the_observations():
    """Two steps of a scalar model: sum_t loglik_t = log N([z_1, z_2]; 0, C) with the joint
    covariance C written out by hand."""
    f, q, r, p0 = 0.8, 0.3, 0.5, 2.0
    zs = np.array([[[0.7]], [[-1.1]]])
    ll, nis, _ = R.kalman_evidence([[f]], [[1.]], [[q]], [[r]], np.zeros((1, 1)), [[p0]], zs)
    v1 = f * f * p0 + q           # var x_1
    v2 = f * f * v1 + q           # var x_2
    C = np.array([[v1 + r, f * v1], [f * v1, v2 + r]])
    z = zs[:, 0, 0]
    want = -0.5 * (z @ np.linalg.inv(C) @ z + math.log(np.linalg.det(C)) + 2 * math.log(2 * math.pi))
    assert ll.sum() == pytest.approx(want, rel=1e-12)
    assert nis.shape == (2, 1)


def test_innovation_argument_checks(monkeypatch):
    zm, S = torch.zeros(4, 3), torch.eye(3).repeat(4, 1, 1)
    with pytest.raises(RuntimeError, match="HIP"):
        K.innovation(zm, S, zm)
    # the checks behind the device check (none of these reaches the library)
    monkeypatch.setattr(K, "require_hip", lambda *a, **k: None)
    with pytest.raises(RuntimeError, match="float32"):
        K.innovation(zm.double(), S, zm)
    with pytest.raises(RuntimeError, match="z_tril"):
        K.innovation(zm, torch.eye(4).repeat(4, 1, 1), zm)
    with pytest.raises(RuntimeError, match="obs"):
        K.innovation(zm, S, torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="z_mean"):
        K.innovation(torch.zeros(3), S, zm)
    big = torch.zeros(2, 65)
    with pytest.raises(RuntimeError, match="dz = 65"):
        K.innovation(big, torch.eye(65).repeat(2, 1, 1), big)


def test_abi_innovation_argument_errors_without_a_device():
    from op import _lib
    dll = _lib.lib.load()
    assert "bpk_ukf_innovation_f32" in _lib.exported_symbols()
    p = 8  # stands for "non-null"; nothing is dereferenced on the host
    assert dll.bpk_ukf_innovation_f32(p, p, p, None, p, p, p, 4, 65, None) == 1
    assert b"dz = 65" in dll.bpk_last_error()
    assert dll.bpk_ukf_innovation_f32(p, p, p, None, p, p, p, 4, 0, None) == 1
    assert dll.bpk_ukf_innovation_f32(p, p, p, p, None, p, p, 4, 8, None) == 1
    assert b"nis" in dll.bpk_last_error()
    assert dll.bpk_ukf_innovation_f32(p, p, p, None, p, p, p, 0, 8, None) == 0  # N = 0, white NULL


def test_filter_history_positional_signature_is_unchanged():
    from pinn_kalman.ukf import FilterHistory
    T, N, n = 2, 3, 4
    h = FilterHistory(torch.zeros(T + 1, N, n), torch.zeros(T + 1, N, n, n), torch.zeros(T, N, n),
                      torch.zeros(T, N, n, n), [None] * T)
    assert len(h) == T and h.nis is None and h.logliks is None and h.accepted is None
    h = FilterHistory(torch.zeros(T + 1, N, n), torch.zeros(T + 1, N, n, n), torch.zeros(T, N, n),
                      torch.zeros(T, N, n, n), [None] * T, nis=torch.zeros(T, N))
    assert h.nis.shape == (T, N)


def test_filter_arguments_validate_on_the_host():
    from pinn_kalman.ukf import SquareRootUKF
    f = SquareRootUKF(lambda x, u: (x, None), lambda x: (x, None))
    assert f.diagnostics is False and f.gate is None and f.nis is None and f.accepted is None
    f = SquareRootUKF(lambda x, u: (x, None), lambda x: (x, None), diagnostics=True, gate=9)
    assert f.diagnostics is True and f.gate == 9.0
    steps = SquareRootUKF._valid_steps
    assert steps(None, 3, 4) == [True] * 3
    assert steps([True, False, None], 3, 4) == [True, False, False]
    assert steps(torch.tensor([True, False]), 2, 4) == [True, False]
    m = torch.ones(2, 4, dtype=torch.bool)
    got = steps(m, 2, 4)
    assert len(got) == 2 and torch.equal(got[0], m[0])
    with pytest.raises(ValueError):
        steps([True], 2, 4)
    with pytest.raises(ValueError):
        steps(torch.ones(2, 4), 2, 4)  # not bool


def test_ukf_statistics_need_diagnostics_and_valid_rows_follow_patch_order():
    from configs.pinn import pinn_pde
    from pinn_kalman.ukf import PINN_KF, UKF
    from pinn_kalman.ukf_utils import patch
    c = pinn_pde.get_config()
    c.data.image_size = 16
    c.kf.patch_size = 4
    c.device = torch.device("cpu")
    u = UKF(c)
    assert u.ukf.diagnostics is False and u.ukf.gate is None
    for fn in (u.nis_maps, u.log_likelihood):
        with pytest.raises(RuntimeError, match="diagnostics"):
            fn()
    u = UKF(c, diagnostics=True, gate=40.)
    assert u.ukf.diagnostics is True and u.ukf.gate == 40.
    # a frame mask over B = 3 samples marks exactly the rows patch() makes of those samples
    B = 3
    valid = torch.tensor([True, False, True])
    fields = valid.float().view(B, 1, 1, 1).expand(B, 4, 16, 16)
    assert torch.equal(u._valid_rows(valid), patch(fields, 4)[:, 0] == 1)
    both = u._valid_rows(torch.stack([valid, ~valid]))
    assert both.shape == (2, 4 * B * 16) and torch.equal(both[1], ~both[0])
    with pytest.raises(ValueError):
        u._valid_rows(torch.ones(3))
    c.model.feature_nums = [4, 8, 8]
    kf = PINN_KF(c, diagnostics=True, gate=7.5)
    assert kf.ukf.ukf.diagnostics is True and kf.ukf.ukf.gate == 7.5
