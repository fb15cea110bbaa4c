"""B-PINN preliminary train step (configs/pinn/pinn_pde.py, 64 x 64): the fused weight sampler
(op.bayes, BPK_BAYES_FUSED=1) against its aten composition (=0), interleaved in one process --
per repetition a window of --steps steps of each, host clock around a device synchronise --
at each batch size of --batches.  Then one step of each form under torch.profiler: kernels per
step, and the device time of the bayes kernels with their achieved bytes/s (12 B per element
forward: mu, rho read, W written; 20 B backward: mu, rho, gW read, gmu, grho written).
Prints one JSON line per batch size.

    python tools/bench_bpinn.py [--batches 64 8] [--steps 10] [--reps 3] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-pinn-kalman-filter_amd"), os.path.join(REPO, "tests"), REPO]
import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

import losses  # noqa: E402
from configs.pinn import pinn_pde  # noqa: E402
from conftest import build_pinn_weights, full_pinn_config, make_pinn_inputs  # noqa: E402
from inverse.operators import InpaintOperator  # noqa: E402
from models.ema import ExponentialMovingAverage  # noqa: E402
from op import bayes  # noqa: E402
from pinn_kalman.pinn import B_PINN, PINN  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in a.batches:
        c = full_pinn_config(pinn_pde.get_config, batch=B)
        batch = tuple(v.to(dev) for v in make_pinn_inputs(c, 1))
        c.device = dev
        model = B_PINN(c, build_pinn_weights(PINN, c))
        state = dict(optimizer=(losses.get_optimizer(c, model.flownet.parameters(), is_bpinn=True),
                                losses.get_optimizer(c, model.pressurenet.parameters(), 0.05,
                                                     is_bpinn=True)),
                     model=model, ema=ExponentialMovingAverage(model.parameters(), c.model.ema_rate),
                     step=0)
        g = torch.Generator().manual_seed(0)
        op = InpaintOperator(mask=[(torch.rand(batch[0].shape, generator=g) < 0.1).float().to(dev)])
        step_fn = losses.get_prelim_step_fn(c, True, losses.optimization_manager(c, is_bpinn=True),
                                            is_bpinn=True)

        def run(fused, n):
            bayes._FUSED = fused
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                out = step_fn(state, op, batch)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n, out

        for fused in (True, False):
            run(fused, a.warmup)
        rate = {True: [], False: []}
        for _ in range(a.reps):
            for fused in (True, False):  # interleaved: both forms see the same clocks
                rate[fused].append(1.0 / run(fused, a.steps)[0])
        res = {"what": "B-PINN prelim train step, fused sampler vs aten composition", "batch": B,
               "steps": a.steps, "reps": a.reps,
               "P": [model.flownet.bayes.numel, model.pressurenet.bayes.numel]}
        for fused, key in ((True, "fused"), (False, "aten")):
            res[key + "_steps_per_s"] = round(statistics.median(rate[fused]), 3)
            res[key + "_steps_per_s_min_max"] = [round(min(rate[fused]), 3),
                                                 round(max(rate[fused]), 3)]
        res["fused_over_aten"] = round(res["fused_steps_per_s"] / res["aten_steps_per_s"], 4)
        for fused, key in ((True, "fused"), (False, "aten")):
            bayes._FUSED = fused
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                out = step_fn(state, op, batch)
                torch.cuda.synchronize()
            kern = [e for e in prof.events()
                    if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
                    and "Memset" not in e.name]
            res[key + "_kernels_per_step"] = len(kern)
            res[key + "_finite"] = bool(torch.isfinite(out[0]))
            if fused:
                ks = {}
                for e in kern:
                    for tag in ("k_bayes_fwd", "k_bayes_kl", "k_bayes_bwd"):
                        if tag in e.name:
                            ks.setdefault(tag, []).append(e.device_time)
                # launches in step order: FlowNet, then PressureNet
                res["bayes_kernel_us"] = {k: [round(v, 2) for v in vs] for k, vs in ks.items()}
                P = res["P"]
                for tag, per in (("k_bayes_fwd", 12), ("k_bayes_bwd", 20)):
                    if len(ks.get(tag, [])) == 2:
                        res[tag + "_GBps"] = [round(per * p / (us * 1e-6) / 1e9, 1)
                                              for p, us in zip(P, ks[tag])]
        bayes._FUSED = True
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
