"""CPU: the Bayesian layers (models/bayesian.py), B_PINN, its checkpoint / training plumbing and
the argument checks of the bayes C entry points.  The KL formula of tests/bayes_ref.py (the
truth of test_gpu_bayes.py) is anchored here to torch.distributions."""
import math

import pytest
import torch
import torch.nn as nn

import bayes_ref
from conftest import full_pinn_config

SIZES = [1, 3, 32, 56448, 2, 149760, 5]


def _segments(sizes):
    out, at = [], 0
    for n in sizes:
        out.append((at, n))
        at += n
    return out


def test_kl_restatement_matches_torch_distributions():
    from torch.distributions import Normal, kl_divergence
    g = torch.Generator().manual_seed(3)
    P = sum(SIZES)
    mu = torch.randn(P, generator=g, dtype=torch.float64) * 0.3
    rho = torch.randn(P, generator=g, dtype=torch.float64) * 2 - 2
    rho[::7] = -30.0
    rho[3::11] = 25.0
    segs = _segments(SIZES)
    pms = [0.0, 0.05, -0.1, 0.0, 0.2, 0.0, 0.01]
    pss = [0.1, 0.01, 1.0, 0.1, 0.5, 0.01, 0.3]
    want = 0.0
    # not F.softplus: its linear branch above 20 is off by 1.4e-11 at rho = 25
    sigma = bayes_ref.softplus(rho)
    for (off, n), pm, ps in zip(segs, pms, pss):
        q = Normal(mu[off:off + n], sigma[off:off + n])
        p = Normal(torch.full((n,), pm, dtype=torch.float64),
                   torch.full((n,), ps, dtype=torch.float64))
        want = want + kl_divergence(q, p).mean()
    got = bayes_ref.kl(mu, rho, pms, pss, segs)
    assert abs(float(got - want)) <= 1e-12 * abs(float(want))
    # one prior for all segments: the scalar form
    want1 = sum(kl_divergence(Normal(mu[o:o + n], sigma[o:o + n]),
                              Normal(torch.zeros(n, dtype=torch.float64),
                                     torch.full((n,), 0.1, dtype=torch.float64))).mean()
                for o, n in segs)
    got1 = bayes_ref.kl(mu, rho, 0.0, 0.1, segs)
    assert abs(float(got1 - want1)) <= 1e-12 * abs(float(want1))


def test_restatement_softplus_is_stable():
    rho = torch.tensor([-100.0, -30.0, 0.0, 25.0, 30.0], dtype=torch.float64)
    s = bayes_ref.softplus(rho)
    assert torch.isfinite(s).all() and (s > 0).all()
    assert abs(float(s[0]) / math.exp(-100.0) - 1) < 1e-12
    assert abs(float(s[2]) - math.log(2.0)) < 1e-15


@pytest.fixture(scope="module")
def cfg():
    from configs.pinn import pinn_pde
    return full_pinn_config(pinn_pde.get_config)


@pytest.fixture(scope="module")
def bpinn(cfg):
    from pinn_kalman.pinn import B_PINN
    torch.manual_seed(11)
    return B_PINN(cfg)


def test_bpinn_builds_with_flat_parameters(cfg, bpinn):
    from models.bayesian import BayesConv2d, BayesConvTranspose2d
    from pinn_kalman.pinn import PINN
    assert not any(isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) for m in bpinn.modules())
    kinds = {type(m) for m in bpinn.modules()}
    assert BayesConv2d in kinds and BayesConvTranspose2d in kinds
    det = PINN(cfg)
    for net, dnet, ps in ((bpinn.flownet, det.flownet, 0.1),
                          (bpinn.pressurenet, det.pressurenet, 0.01)):
        b = net.bayes
        assert b.numel == sum(p.numel() for p in dnet.parameters())
        assert [tuple(p.shape) for p in net.parameters()] == [(b.numel,), (b.numel,)]
        assert [(n, s) for n, s in b.segments] == [(n, tuple(p.shape))
                                                   for n, p in dnet.named_parameters()]
        at = 0
        for off, n, pm, sg in b.table.tolist():
            assert off == at and n >= 1 and pm == 0.0 and sg == ps
            at += int(n)
        assert at == b.numel
    up = bpinn.flownet.inference_units[1].match.flow_upsample
    assert up.groups == 2 and up._ib is None and up.kernel_size == (4, 4)


def test_default_init_moments(bpinn):
    for net, rho0 in ((bpinn.flownet, -3.0), (bpinn.pressurenet, -0.5)):
        b = net.bayes
        n = b.numel
        for v, mean in ((b.mu.detach().double(), 0.0), (b.rho.detach().double(), rho0)):
            assert abs(float(v.mean()) - mean) <= 5 * 0.1 / math.sqrt(n)
            assert abs(float(v.std()) - 0.1) <= 5 * 0.1 / math.sqrt(2 * n)


def test_moped_init(cfg):
    from pinn_kalman.pinn import B_PINN, PINN
    torch.manual_seed(5)
    det = PINN(cfg)
    with torch.no_grad():
        for p in det.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    w = {k: torch.cat([p.detach().reshape(-1) for p in n.parameters()])
         for k, n in (("f", det.flownet), ("p", det.pressurenet))}
    b = B_PINN(cfg, det)
    delta = cfg.model.bpinn_moped_delta
    for key, net in (("f", b.flownet), ("p", b.pressurenet)):
        mu, rho = net.bayes.mu.detach(), net.bayes.rho.detach()
        assert torch.equal(mu, w[key])
        big = w[key].abs() > 1e-3
        assert int(big.sum()) > 1000
        sigma = bayes_ref.softplus(rho.double())[big]
        want = delta * w[key].double().abs()[big]
        assert float(((sigma - want).abs() / want).max()) <= 1e-5
        ref = bayes_ref.moped_rho(w[key].double(), delta)
        assert torch.allclose(rho.double(), ref, rtol=1e-6, atol=1e-6)


def test_layerwise_state_dict_round_trip(cfg, bpinn):
    from models.bayesian import load_layerwise_state_dict, to_layerwise_state_dict
    from pinn_kalman.pinn import B_PINN
    other = B_PINN(cfg)
    for a, b in ((bpinn.flownet, other.flownet), (bpinn.pressurenet, other.pressurenet)):
        sd = to_layerwise_state_dict(a)
        assert len(sd) == 2 * len(a.bayes.segments)
        first = a.bayes.segments[0][0].rsplit(".", 1)[0]
        assert tuple(sd[first + ".mu_kernel"].shape) == a.bayes.segments[0][1]
        assert first + ".rho_kernel" in sd and first + ".mu_bias" in sd
        assert all(k.rsplit(".", 1)[1] in ("mu_kernel", "rho_kernel", "mu_bias", "rho_bias")
                   for k in sd)
        assert not torch.equal(a.bayes.mu, b.bayes.mu)
        load_layerwise_state_dict(b, sd)
        assert torch.equal(a.bayes.mu, b.bayes.mu) and torch.equal(a.bayes.rho, b.bayes.rho)
        sd.pop(next(iter(sd)))
        with pytest.raises(KeyError):
            load_layerwise_state_dict(b, sd)


def test_other_parametrised_layers_raise():
    from models.bayesian import dnn_to_bnn
    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.body = nn.Sequential(nn.Conv2d(2, 2, 3), nn.Linear(4, 4))

    with pytest.raises(NotImplementedError, match="Linear"):
        dnn_to_bnn(Net(), {"prior_sigma": 0.1})
    with pytest.raises(TypeError, match="Sequential"):
        dnn_to_bnn(nn.Sequential(nn.Conv2d(2, 2, 3)), {"prior_sigma": 0.1})


def _state(cfg, model):
    import losses
    from models.ema import ExponentialMovingAverage
    return dict(optimizer=(losses.get_optimizer(cfg, model.flownet.parameters(), is_bpinn=True),
                           losses.get_optimizer(cfg, model.pressurenet.parameters(), 0.05,
                                                is_bpinn=True)),
                model=model, ema=ExponentialMovingAverage(model.parameters(), 0.9), step=0)


def test_restore_bpinn_checkpoint_round_trip(cfg, bpinn, tmp_path):
    import utils
    from pinn_kalman.pinn import B_PINN, PINN
    nothing = str(tmp_path / "none.pth")
    st = _state(cfg, bpinn)
    st["step"] = 7
    assert utils.restore_bpinn_checkpoint(nothing, nothing, st, cfg) is st and st["step"] == 7
    # a B-PINN checkpoint resumes in place
    path = str(tmp_path / "bpinn.pth")
    utils.save_checkpoint(path, st)
    st2 = _state(cfg, B_PINN(cfg))
    utils.restore_bpinn_checkpoint(nothing, path, st2, cfg)
    assert st2["step"] == 7
    for a, b in zip(bpinn.state_dict().values(), st2["model"].state_dict().values()):
        assert torch.equal(a, b)
    # only a deterministic PINN checkpoint: MOPED from it, new optimizers
    torch.manual_seed(2)
    det = PINN(cfg)
    dpath = str(tmp_path / "pinn.pth")
    torch.save({"model": det.state_dict()}, dpath)
    st3 = _state(cfg, B_PINN(cfg))
    old = st3["model"]
    utils.restore_bpinn_checkpoint(dpath, nothing, st3, cfg)
    assert st3["model"] is not old and st3["model"].using_pretrained
    flat = torch.cat([p.detach().reshape(-1) for p in det.flownet.parameters()])
    assert torch.equal(st3["model"].flownet.bayes.mu.detach(), flat)
    assert st3["optimizer"][0].param_groups[0]["params"][0] is st3["model"].flownet.bayes.mu
    assert st3["optimizer"][1].param_groups[0]["lr"] == pytest.approx(cfg.optim.bpinn_lr * 0.05)


def test_prelim_step_fn_accepts_bpinn(cfg):
    import losses
    fn = losses.get_prelim_step_fn(cfg, True, losses.optimization_manager(cfg, is_bpinn=True),
                                   is_bpinn=True)
    assert callable(fn)


def test_stream_is_host_state(bpinn):
    bpinn.reseed(9, step=4)
    assert (bpinn.flownet.bayes.seed, bpinn.pressurenet.bayes.seed) == (18, 19)
    assert bpinn.flownet.bayes.step == bpinn.pressurenet.bayes.step == 4
    with pytest.raises(RuntimeError, match="HIP"):
        bpinn.flownet.bayes.draw()  # no CPU fallback
    assert bpinn.flownet.bayes.step == 4
    with pytest.raises(RuntimeError, match="no forward"):
        bpinn.pressurenet.kl_loss()


def test_make_table_checks_the_tiling():
    from op import bayes
    t = bayes.make_table([(0, 3, 0.0, 0.1), (3, 5, 0.0, 0.2)], "cpu")
    assert t.dtype == torch.float64 and t.tolist() == [[0, 3, 0, 0.1], [3, 5, 0, 0.2]]
    for bad in ([(0, 3, 0.0, 0.1), (4, 5, 0.0, 0.1)], [(0, 0, 0.0, 0.1)], [(0, 2, 0.0, 0.0)], []):
        with pytest.raises(ValueError):
            bayes.make_table(bad, "cpu")
    with pytest.raises(RuntimeError, match="HIP"):
        bayes.sample_kl(torch.zeros(8), torch.zeros(8), t, 0, 0)


def test_bayes_entry_points_report_argument_errors_without_a_device():
    from op import _lib
    dll = _lib.lib.load()
    assert dll.bpk_bayes_workspace_bytes(0) == 0
    assert dll.bpk_bayes_workspace_bytes(5) == 8
    assert dll.bpk_bayes_workspace_bytes(10 ** 9) == 1024 * 8
    rc = dll.bpk_bayes_sample_kl_f32(None, None, None, 1, 0, 0, 0, None, None, None, None)
    assert rc == 1 and b"elements" in dll.bpk_last_error()
    rc = dll.bpk_bayes_sample_kl_f32(None, None, None, 9, 8, 0, 0, None, None, None, None)
    assert rc == 1 and b"segments" in dll.bpk_last_error()
    rc = dll.bpk_bayes_sample_kl_f32(None, None, None, 2, 8, 0, 0, None, None, None, None)
    assert rc == 1 and b"null pointer" in dll.bpk_last_error()
    rc = dll.bpk_bayes_sample_kl_bwd_f32(None, None, None, 0, 8, 0, 0, None, None, None, None,
                                         None)
    assert rc == 1 and b"segments" in dll.bpk_last_error()
    rc = dll.bpk_bayes_sample_kl_bwd_f32(None, None, None, 2, 8, 0, 0, None, None, None, None,
                                         None)
    assert rc == 1 and b"null pointer" in dll.bpk_last_error()
