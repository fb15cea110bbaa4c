"""One backward (Rauch-Tung-Striebel) step of the UKF smoother at the reference's shape (192 x 192
fields, patch_size 8, B = 1 -> 2304 filters of state dimension 64, 129 sigma points each):
HIP-event time of the whole step of `SquareRootUKF.smooth` (sigma points redrawn, NSDynamics,
`rts_smooth`) and of `op.ukf.rts_smooth` alone, against `op.ukf.kalman_update` at the same
shape -- the three timed in turn inside every repetition, median over --reps after --warmup.
The stage inputs come from one `filter` step of the device's own filter.

Comparison basis: the same backward step by tests/urts_ref.py in float32 on the CPU (16
threads), fed the device's stage inputs, dynamics excluded.  Prints one JSON line.

    python tools/bench_urts.py [--size 192] [--reps 10] [--warmup 3] [--no-basis]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-pinn-kalman-filter_amd"), os.path.join(REPO, "tests"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from configs.pinn import pinn_pde  # noqa: E402
from op import ukf as K  # noqa: E402
from pinn_kalman.ukf import UKF  # noqa: E402
from pinn_kalman.ukf_utils import patch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-basis", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    c = pinn_pde.get_config()
    c.data.image_size = a.size
    c.device = dev
    p, n = c.kf.patch_size, c.kf.patch_size ** 2
    rng = np.random.default_rng(0)
    shape = (1, 1, a.size, a.size)
    fields = torch.from_numpy(np.concatenate([
        rng.uniform(0.1, 1.0, shape),
        rng.uniform(0.05, 0.5, shape) * rng.choice([-1, 1], shape),
        rng.uniform(0.05, 0.5, shape) * rng.choice([-1, 1], shape),
        rng.normal(0, 0.01, shape)], 1).astype(np.float32))
    obs = (fields + torch.from_numpy(rng.normal(0, 1e-3, fields.shape).astype(np.float32))).to(dev)
    x0 = patch(fields, p).to(dev)
    N = x0.shape[0]
    filt = UKF(c, compat=False)
    u = filt.ukf
    gamma, wm0, wc0, wi = K.merwe_weights(n)
    rows0 = K.point_rows(N, n, 4, device=dev)[:, 0].contiguous()
    filt.initialize(x0, var=1e-6)
    z = patch(obs, p)
    hist = u.filter([z])
    m0, S0, mp, Sp = hist.means[0], hist.scale_trils[0], hist.pred_means[0], hist.pred_trils[0]
    m1, S1 = hist.means[1], hist.scale_trils[1]
    # the inputs of the forward update of that step, and of the backward stage
    X2 = K.sigma_points(mp, Sp, gamma, 4)
    Z, Rf = filt.measurement(X2, factor_rows=rows0)
    zm, zt, _ = K.unscented_root(Z, Rf, n, wm0, wc0, wi, 4)
    X = K.sigma_points(m0, S0, gamma, 4)
    Y = filt.dynamic(X)[0]

    def backward_step():
        x = K.sigma_points(m0, S0, gamma, 4)
        y = filt.dynamic(x)[0]
        return K.rts_smooth(m0, S0, x, y, mp, Sp, m1, S1, wc0, wi, 4)

    work = {"backward_step": backward_step,
            "rts_smooth": lambda: K.rts_smooth(m0, S0, X, Y, mp, Sp, m1, S1, wc0, wi, 4),
            "kalman_update": lambda: K.kalman_update(mp, Sp, X2, Z, zm, zt, z, wc0, wi, 4)}
    ms = {k: [] for k in work}
    out = {}
    for it in range(a.warmup + a.reps):
        for k, fn in work.items():  # interleaved: the three see the same clocks
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out[k] = fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    res = {"what": "UKF smoother, one backward step", "size": a.size, "filters": N, "n": n,
           "reps": a.reps, "warmup": a.warmup}
    for k, v in ms.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    res["rts_smooth_over_kalman_update"] = round(res["rts_smooth_ms"] / res["kalman_update_ms"], 3)
    ms_s, Ss_s, st = out["rts_smooth"]
    res["flagged"] = int(st.sum()) + int(u.status.sum())
    res["finite"] = bool(torch.isfinite(ms_s).all() and torch.isfinite(Ss_s).all())
    res["step_equals_op"] = bool(torch.equal(out["backward_step"][0], ms_s)
                                 and torch.equal(out["backward_step"][1], Ss_s))
    if not a.no_basis:
        import ukf_ref
        import urts_ref
        torch.set_num_threads(16)
        cpu = [t.cpu() for t in (m0, S0, X, Y, mp, Sp, m1, S1)]
        urts_ref.smooth(*(t[:64] if t.shape[0] == N else t[:129 * 64] for t in cpu), wc0, wi, 4)
        ukf_ref.rows(N, n, 4)  # index table, cached: kept out of the arithmetic time
        t0 = time.perf_counter()
        r = urts_ref.smooth(*cpu, wc0, wi, 4)
        t1 = time.perf_counter()
        res["basis"] = {"what": "tests/urts_ref.py float32, CPU, 16 threads, dynamics excluded",
                        "ms": round((t1 - t0) * 1e3, 1), "flagged": int(r[2].sum())}
        res["basis_over_rts_smooth"] = round(res["basis"]["ms"] / res["rts_smooth_ms"], 1)
        ok = ~(r[2] | st.cpu().bool())
        res["max_rel_diff_vs_basis"] = (float((r[0][ok] - ms_s.cpu()[ok]).abs().max())
                                        / float(r[0][ok].abs().max()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
