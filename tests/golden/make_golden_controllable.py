"""Generate the conditional-sampling fixtures by running the REFERENCE's
controllable_generation.py on CPU (development container only: the reference does not travel).

    python tests/golden/make_golden_controllable.py

Same import recipe as make_golden.py (its stubs are reused).  Every torch.randn_like draw of
get_pc_inpainter / get_pc_colorizer is recorded in order; per PC iteration the reference draws
[corrector update x n_steps] [data noise] [predictor update] [data noise], update draws absent
for a None corrector / predictor.  They are stored as two ordered lists:

  draws   the update draws, full shape
  draws2  the data-noise draws of the projections.  Only what the reference's arithmetic can
          see is kept, the rest multiplies a zero mask: for inpainting the draw times the
          mask, for colorization channel 0 ([n, B, 1, H, W]).

Fixtures (N = 25, the smallest grid with every DDPM beta below 1, make_golden.py:323):
  ctrl_inpaint_em_langevin.npz  net ncsnpp_a, 32^2 x 1, B = 2, VP continuous, snr 0.075
  ctrl_inpaint_anc_none.npz     net ddpm_a, discrete: the None-corrector projection
  ctrl_colorize_rd_ald.npz      3-channel ncsnpp_c (16^2, nf 8; weights in the file), n_steps 2
Each holds prior, data (the gray image for colorize), mask, draws, draws2, out and the settings:
recorded inputs and outputs only.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

N, EPS = 25, 1e-3


def main():
    if not os.path.isdir(mg.REF):
        print(f"reference not found at {mg.REF}; nothing to do")
        return
    sys.dont_write_bytecode = True
    ConfigDict = mg._install_stubs()
    sys.path.insert(0, mg.REF)
    import torch

    torch.set_num_threads(4)
    import controllable_generation as cg
    import sampling
    import sde_lib
    from models import ddpm, ncsnpp  # noqa: F401  (registers models)
    from models import utils as mutils

    def to_cfg(o):
        if isinstance(o, dict):
            return ConfigDict({k: to_cfg(v) for k, v in o.items()})
        if isinstance(o, list):
            return tuple(to_cfg(v) for v in o)
        return o

    def net_config(name):
        d = np.load(os.path.join(HERE, f"net_{name}.npz"))
        cfg = to_cfg(json.loads(str(d["config_json"])))
        cfg.model.fir_kernel = list(cfg.model.fir_kernel)
        cfg.device = torch.device("cpu")
        return cfg, {k[2:]: torch.tensor(d[k]) for k in d.files if k.startswith("p:")}

    def stored_net(name):
        cfg, sd = net_config(name)
        model = mutils.get_model(cfg.model.name)(cfg)
        model.load_state_dict(sd, strict=True)
        return cfg, model.eval()

    def color_net():
        cfg, _ = net_config("ncsnpp_c")
        cfg.data.num_channels = 3
        torch.manual_seed(0)
        model = mutils.get_model(cfg.model.name)(cfg)
        with torch.no_grad():  # the reference zero-inits Conv_1 / NIN_3, as in make_golden.py
            for p in model.parameters():
                if p.requires_grad:
                    p.add_(torch.randn_like(p) * 0.02)
        return cfg, model.eval()

    def record(name, kind, cfg, model, predictor, corrector, B, snr, n_steps, continuous,
               extra=None):
        sde = sde_lib.VPSDE(beta_min=cfg.model.beta_min, beta_max=cfg.model.beta_max, N=N)
        C, S = cfg.data.num_channels, cfg.data.image_size
        shape = (B, C, S, S)
        g = torch.Generator().manual_seed(23)
        if kind == "inpaint":
            data = torch.rand(shape, generator=g)
            mask = (torch.rand(shape, generator=g) < 0.5).float()
            mask[:, :, 3, :] = 1.   # one all-known row
            mask[:, :, 7, :] = 0.   # one all-unknown row
        else:
            data = torch.rand((B, 1, S, S), generator=g).repeat(1, 3, 1, 1)
            mask = torch.cat([torch.ones(B, 1, S, S), torch.zeros(B, 2, S, S)], dim=1)
        log = []
        real = torch.randn_like

        def rec(t, *a, **k):
            z = real(t, *a, **k)
            log.append(z.clone())
            return z

        get = cg.get_pc_inpainter if kind == "inpaint" else cg.get_pc_colorizer
        fn = get(sde, sampling.get_predictor(predictor), sampling.get_corrector(corrector),
                 lambda v: v, snr, n_steps=n_steps, probability_flow=False,
                 continuous=continuous, denoise=True, eps=EPS)
        torch.manual_seed(11)
        prior = sde.prior_sampling(shape)
        torch.manual_seed(11)
        torch.randn_like = rec
        try:
            out = fn(model, data, mask) if kind == "inpaint" else fn(model, data)
        finally:
            torch.randn_like = real
        n_corr = n_steps if corrector != "none" else 0
        n_pred = 1 if predictor != "none" else 0
        per = n_corr + 1 + n_pred + 1
        assert len(log) == N * per, (len(log), N, per)
        draws, draws2 = [], []
        for i in range(N):
            it = log[i * per:(i + 1) * per]
            draws += it[:n_corr] + it[n_corr + 1:n_corr + 1 + n_pred]
            draws2 += [it[n_corr], it[per - 1]]
        draws2 = torch.stack(draws2)
        draws2 = draws2 * mask if kind == "inpaint" else draws2[:, :, :1]
        arr = {"prior": prior.numpy(), "data": data.numpy(), "mask": mask.numpy(),
               "out": out.numpy(), "draws": torch.stack(draws).numpy(),
               "draws2": draws2.numpy(), "N": np.array(N), "eps": np.array(EPS),
               "snr": np.array(snr), "n_steps": np.array(n_steps),
               "continuous": np.array(continuous), "predictor": np.array(predictor),
               "corrector": np.array(corrector), "condition": np.array(kind)}
        arr.update(extra or {})
        mg._save(f"ctrl_{name}.npz", **arr)

    cfg, model = stored_net("ncsnpp_a")
    record("inpaint_em_langevin", "inpaint", cfg, model, "euler_maruyama", "langevin", 2, 0.075, 1,
           True, {"net": np.array("ncsnpp_a")})
    cfg, model = stored_net("ddpm_a")
    record("inpaint_anc_none", "inpaint", cfg, model, "ancestral_sampling", "none", 2, 0.16, 1,
           False, {"net": np.array("ddpm_a")})
    cfg, model = color_net()
    weights = {"p:" + k: v.detach().numpy() for k, v in model.state_dict().items()}
    weights["config_json"] = np.array(mg._config_json(cfg))
    record("colorize_rd_ald", "colorize", cfg, model, "reverse_diffusion", "ald", 2, 0.16, 2, True,
           weights)


if __name__ == "__main__":
    main()
