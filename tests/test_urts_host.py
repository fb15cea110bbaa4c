"""CPU: the host side of the unscented RTS smoother -- the anchor of the restatement
tests/urts_ref.py (the yardstick of tests/test_gpu_urts.py) to the closed-form
Rauch-Tung-Striebel recursion, the C-ABI argument checks of bpk_ukf_smooth_f32 without a
device, `SquareRootUKF.smooth`'s preconditions and the masked measurement model."""
import math

import pytest
import torch

import ukf_ref
import urts_ref

TRIPLES = [(1., 0., 0.), (0.5, 2., 0.), (1., 2., 1.)]


def _linear_case(n, seed, T=3):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    N, sq = 3, math.sqrt(n)
    eye = torch.eye(n, dtype=torch.float64)
    F = eye + 0.3 * rn(N, n, n) / sq
    H = eye + 0.3 * rn(N, n, n) / sq
    S0 = (0.1 * rn(N, n, n) / sq).tril() + 0.3 * eye
    Q = (0.05 * rn(N, n, n) / sq).tril() + 0.05 * eye
    R = (0.05 * rn(N, n, n) / sq).tril() + 0.2 * eye
    return N, F, H, S0, Q, R, rn(N, n), rn(T, N, n)


@pytest.mark.parametrize("abk", TRIPLES)
@pytest.mark.parametrize("n", [4, 16, 64])
def test_restatement_equals_closed_form_rts_on_linear_models(n, abk):
    """Linear f(x) = F x, h(x) = H x: the unscented transform is exact, so C = P F^T and three
    forward steps followed by three backward steps of the float64 restatement equal the
    textbook recursion G = P F^T P-^-1, m^s = m + G (m^s_+ - m-), P^s = P + G (P^s_+ - P-) G^T
    to rounding (<= 1e-12), for all three branches of the point-0 term."""
    T = 3
    N, F, H, S0, Q, R, m0, zs = _linear_case(n, 20 * n + int(abk[0] * 2 + abk[2]), T)
    idx = ukf_ref.rows(N, n)

    def per_row(M):  # [N, n, n] -> the matrix of each point row's filter
        out = torch.empty((2 * n + 1) * N, n, n, dtype=M.dtype)
        out[idx.reshape(-1)] = M.unsqueeze(1).expand(-1, 2 * n + 1, -1, -1).reshape(-1, n, n)
        return out
    Fr, Hr = per_row(F), per_row(H)
    dyn = lambda X: ((Fr @ X.unsqueeze(2)).squeeze(2), Q)
    meas = lambda X: ((Hr @ X.unsqueeze(2)).squeeze(2), R)
    ms, Ss, flag, _ = urts_ref.chain(m0, S0, dyn, meas, zs, abk)
    assert not flag.any()
    # closed form: the Kalman filter forward, keeping posteriors and predictions
    mv = lambda A, x: (A @ x.unsqueeze(2)).squeeze(2)
    Ft, Ht = F.transpose(1, 2), H.transpose(1, 2)
    mk, Pk, mp, Pp = [m0], [S0 @ S0.transpose(1, 2)], [], []
    for t in range(T):
        m1, P1 = mv(F, mk[-1]), F @ Pk[-1] @ Ft + Q @ Q.transpose(1, 2)
        mp.append(m1)
        Pp.append(P1)
        Sk = H @ P1 @ Ht + R @ R.transpose(1, 2)
        Kg = P1 @ Ht @ torch.linalg.inv(Sk)
        mk.append(m1 + mv(Kg, zs[t] - mv(H, m1)))
        Pk.append(P1 - Kg @ Sk @ Kg.transpose(1, 2))
    msk, Psk = mk[T], Pk[T]
    assert (ms[T] - msk).abs().max() <= 1e-12
    for t in range(T - 1, -1, -1):
        G = Pk[t] @ Ft @ torch.linalg.inv(Pp[t])
        msk = mk[t] + mv(G, msk - mp[t])
        Psk = Pk[t] + G @ (Psk - Pp[t]) @ G.transpose(1, 2)
        err_m = float((ms[t] - msk).abs().max())
        err_p = float((Ss[t] @ Ss[t].transpose(1, 2) - Psk).abs().max())
        print(f"n={n} abk={abk} t={t}: mean {err_m:.2e} cov {err_p:.2e}")
        assert err_m <= 1e-12 and err_p <= 1e-12
        assert (Ss[t].triu(1) == 0).all()
        assert (torch.diagonal(Ss[t], dim1=1, dim2=2) > 0).all()
    # smoothing never loses information: P^s <= P (here: on the diagonal)
    assert (torch.diagonal(Psk, dim1=1, dim2=2)
            <= torch.diagonal(Pk[0], dim1=1, dim2=2) + 1e-12).all()


_PTRS = ["mean", "scale_tril", "x_points", "y_points", "pred_mean", "pred_tril", "next_mean",
         "next_tril", "mean_out", "scale_tril_out", "status"]


def _call(dll, N=4, n=4, groups=1, null=None):
    """bpk_ukf_smooth_f32 with 8 standing for 'non-null' (never dereferenced on the host)."""
    ptrs = [None if i == null else 8 for i in range(len(_PTRS))]
    return dll.bpk_ukf_smooth_f32(*ptrs, N, n, 0., .125, groups, None)


def test_abi_argument_errors_without_a_device():
    from op import _lib
    dll = _lib.lib.load()
    assert "bpk_ukf_smooth_f32" in _lib.exported_symbols()
    for kw, word in ((dict(n=0), b"n = 0"), (dict(n=65), b"n = 65"),
                     (dict(N=4, groups=3), b"groups = 3"), (dict(N=-1), b"N = -1")):
        assert _call(dll, **kw) == 1
        msg = dll.bpk_last_error()
        assert word in msg and b"ukf_smooth" in msg, (kw, msg)
    for i, name in enumerate(_PTRS):
        assert _call(dll, null=i) == 1, name
        msg = dll.bpk_last_error()
        assert b"ukf_smooth" in msg and name.encode() + b" is NULL" in msg, (name, msg)
    assert _call(dll, N=0) == 0  # nothing to do: OK without a launch


def test_op_refuses_cpu_tensors_and_bad_shapes():
    from op import ukf as K
    m, S, X = torch.zeros(4, 3), torch.eye(3).repeat(4, 1, 1), torch.zeros(28, 3)
    with pytest.raises(RuntimeError, match="HIP"):
        K.rts_smooth(m, S, X, X, m, S, m, S, 0., 1 / 6)


def test_smooth_needs_a_filter_history():
    from pinn_kalman.ukf import FilterHistory, SquareRootUKF
    f = SquareRootUKF(lambda x, u: (x, None), lambda x: (x, None))
    with pytest.raises(RuntimeError, match="filter"):
        f.smooth(None)
    f.initialize_beliefs(torch.zeros(4, 2), scale_tril=torch.eye(2).repeat(4, 1, 1))
    with pytest.raises(RuntimeError, match="filter"):
        f.smooth(None)
    with pytest.raises(ValueError, match="controls"):
        f.filter(torch.zeros(2, 4, 2), controls=[None])
    h = f.filter(torch.zeros(0, 4, 2))  # no step: no kernel runs
    assert isinstance(h, FilterHistory) and len(h) == 0
    assert h.means.shape == (1, 4, 2) and h.scale_trils.shape == (1, 4, 2, 2)
    assert h.pred_means.shape == (0, 4, 2) and h.pred_trils.shape == (0, 4, 2, 2)
    ms, Ss = f.smooth(h)  # T = 0: the filtered belief itself
    assert torch.equal(ms[0], f.belief_mean) and torch.equal(Ss[0], f.belief_scale_tril)
    with pytest.raises(ValueError):
        f.smooth("history")
    other = FilterHistory(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3, 3), torch.zeros(0, 4, 3),
                          torch.zeros(0, 4, 3, 3), [])
    with pytest.raises(ValueError, match="4 filters of dimension 2"):
        f.smooth(other)


def _config(size=16):
    from configs.pinn import pinn_pde
    c = pinn_pde.get_config()
    c.data.image_size = size
    c.device = torch.device("cpu")
    return c


@pytest.mark.parametrize("fields", [1, 3])
@pytest.mark.parametrize("mask_shape", ["hw", "11hw"])
def test_inpaint_measure(fields, mask_shape):
    """fields = B (2n+1) whole fields in the batch: density rows are states * patched mask tiled
    over the batch, the other rows and the factor are the parent's."""
    from pinn_kalman.ukf_utils import IdentityKFMeasure, InpaintKFMeasure, patch
    c = _config()
    d, patches = 64, 4
    g = torch.Generator().manual_seed(3)
    mask = (torch.rand(16, 16, generator=g) < 0.5).float()
    assert 0 < mask.sum() < mask.numel()
    h = InpaintKFMeasure(c, mask if mask_shape == "hw" else mask[None, None])
    parent = IdentityKFMeasure(c)
    assert isinstance(h, IdentityKFMeasure) and h.supports_factor_rows
    uf, up = torch.rand(1, 2, 16, 16, generator=g) + 0.1, torch.rand(1, 1, 16, 16, generator=g) + 0.1
    h.update_uncertainty(uf, up)
    parent.update_uncertainty(uf, up)
    q = fields * patches
    fld = torch.randn(fields, 4, 16, 16, generator=g)
    x = patch(fld, 8)  # rows (channel, field, patch)
    assert x.shape == (4 * q, d)
    z, f = h(x)
    zp, fp = parent(x)
    assert z.shape == x.shape and f.shape == (4 * q, d, d) and torch.equal(f, fp)
    pm = patch(mask[None, None], 8)
    assert torch.equal(z[:q], x[:q] * pm.repeat(fields, 1))
    assert torch.equal(z[:q], patch(fld[:, :1] * mask, 8))  # = masking the density fields
    assert torch.equal(z[q:], x[q:])
    rows = torch.tensor([0, q, 2 * q + 1, 4 * q - 1])
    z2, f2 = h(x, factor_rows=rows)
    assert torch.equal(z2, z) and f2.shape == (4, d, d) and torch.equal(f2, fp[rows])
    zf, ff = h(x[:q], f_only=True)
    zpf, fpf = parent(x[:q], f_only=True)
    assert torch.equal(zf, z[:q]) and ff.shape == (q, d, d) and torch.equal(ff, fpf)
    zf, ff = h(x[:q], f_only=True, factor_rows=rows[:2])
    assert torch.equal(zf, z[:q]) and ff.shape == (2, d, d)
    with pytest.raises(ValueError, match="mask"):
        InpaintKFMeasure(c, torch.ones(8, 8))


def test_ukf_takes_a_mask_on_the_host():
    from pinn_kalman.ukf import UKF
    from pinn_kalman.ukf_utils import IdentityKFMeasure, InpaintKFMeasure, patch
    c = _config()
    assert type(UKF(c).measurement) is IdentityKFMeasure and UKF(c).mask is None
    mask = torch.zeros(16, 16)
    mask[::2] = 1.
    u = UKF(c, compat=False, mask=mask)
    assert isinstance(u.measurement, InpaintKFMeasure) and u.ukf.measurement_model is u.measurement
    obs = torch.randn(2, 4, 16, 16)
    z = u._observation(obs)
    want = obs.clone()
    want[:, 0] *= mask
    assert torch.equal(z, patch(want, 8))
    u.initialize(torch.zeros(16, 64), var=0.04)
    with pytest.raises(RuntimeError, match="HIP"):
        u.smooth(torch.zeros(1, 1, 4, 16, 16))
