"""What the innovation statistics cost: one `UKF.forward` at the shipped `pinn_pde` geometry
(192 x 192 fields, patch_size 8, B = 1 -> 2304 filters of dimension 64) with diagnostics off
and on, and `op.ukf.innovation` alone on that step's (z_mean, z_tril).

  step_ms   : HIP events around one `forward`, median over --reps steps after --warmup; the
              filter is re-initialised before every step (outside the timed window) so each
              step does the same work; the two filters alternate inside every repetition.
  kernel_us : HIP events around --inner back-to-back calls of the op, per call, median over
              --reps; hbm_fraction = the bytes it must read (N dz (dz + 1) / 2 + 2 N dz floats)
              over that time, over the 8 TB/s peak.

Prints two JSON lines (diagnostics off, diagnostics on).

    python tools/bench_ukf_innovation.py [--size 192] [--reps 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-pinn-kalman-filter_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from configs.pinn import pinn_pde  # noqa: E402
from op import ukf as K  # noqa: E402
from pinn_kalman.ukf import UKF  # noqa: E402
from pinn_kalman.ukf_utils import patch  # noqa: E402

HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--compat", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    c = pinn_pde.get_config()
    c.data.image_size = a.size
    c.device = dev
    p = c.kf.patch_size
    rng = np.random.default_rng(0)
    shape = (1, 1, a.size, a.size)
    fields = torch.from_numpy(np.concatenate([
        rng.uniform(0.1, 1.0, shape),
        rng.uniform(0.05, 0.5, shape) * rng.choice([-1, 1], shape),
        rng.uniform(0.05, 0.5, shape) * rng.choice([-1, 1], shape),
        rng.normal(0, 0.01, shape)], 1).astype(np.float32))
    obs = (fields + torch.from_numpy(rng.normal(0, 1e-3, fields.shape).astype(np.float32))).to(dev)
    x0 = patch(fields, p).to(dev)
    N, dz = x0.shape
    filts = {False: UKF(c, compat=bool(a.compat)),
             True: UKF(c, compat=bool(a.compat), diagnostics=True)}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    times, outs = {False: [], True: []}, {}
    for it in range(a.warmup + a.reps):
        for on, filt in filts.items():
            filt.initialize(x0, var=1e-6)
            e0, e1 = ev(), ev()
            torch.cuda.synchronize()
            e0.record()
            outs[on] = filt(obs)
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[on].append(e0.elapsed_time(e1))
    same = bool(torch.equal(outs[False], outs[True]))
    # the op alone, on the (z_mean, z_tril) of that step
    u = filts[True].ukf
    gamma, wm0, wc0, wi = K.merwe_weights(dz)
    filts[True].initialize(x0, var=1e-6)
    u.predict()
    X = K.sigma_points(u.belief_mean, u.belief_scale_tril, gamma, 4)
    Z, Rf = filts[True].measurement(X, factor_rows=u._rows0)
    zm, zt, _ = K.unscented_root(Z, Rf, dz, wm0, wc0, wi, 4)
    z = patch(obs, p)
    per_call = []
    for _ in range(a.warmup):
        K.innovation(zm, zt, z, white=False)
    for _ in range(a.reps):
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(a.inner):
            K.innovation(zm, zt, z, white=False)
        e1.record()
        e1.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e3 / a.inner)
    kus = statistics.median(per_call)
    nbytes = 4 * (N * dz * (dz + 1) // 2 + 2 * N * dz)
    med = {on: statistics.median(v) for on, v in times.items()}
    lines = []
    for on in (False, True):
        res = {"what": "UKF.forward", "diagnostics": on, "size": a.size, "filters": N, "n": dz,
               "compat": a.compat, "reps": a.reps, "step_ms": round(med[on], 4),
               "step_ms_min_max": [round(min(times[on]), 4), round(max(times[on]), 4)],
               "device": torch.cuda.get_device_name(0)}
        if on:
            res.update({"ratio_on_over_off": round(med[True] / med[False], 4),
                        "outputs_bit_identical": same,
                        "mean_nis": float(u.nis.double().mean()),
                        "innovation_kernel_us": round(kus, 2),
                        "innovation_kernel_us_min_max": [round(min(per_call), 2),
                                                         round(max(per_call), 2)],
                        "innovation_algorithmic_bytes": nbytes,
                        "innovation_hbm_fraction": round(nbytes / (kus * 1e-6) / HBM_PEAK, 4)})
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
