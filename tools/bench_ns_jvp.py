"""ns_step tangent-linear model: the HIP JVP (csrc/ns_step_jvp.hip) against the forward, the
functional HIP adjoint and `torch.func.jvp` of the plain-torch restatement
(tests/ns_step_torch_ref.py) on the same device, float32, at the shapes of
tools/bench_ns_vjp.py (B = 256 and B = 129 fields of 192 x 192) with its field generator; then
Adam 4D-Var against incremental Gauss-Newton 4D-Var on the twin experiment.  Needs a GPU.

Section 1, per shape: four variants alternate inside every repetition (all see the same
clocks), timed with device events around --inner back-to-back calls, median over --reps
repetitions:

  fwd      : ns_step.full_step(compat=False) under no_grad -- the simulator line, for scale
  hip_jvp  : ns_step.full_step_jvp at a stored base state (v1 given): one application of M
  hip_vjp  : ns_step.full_step_vjp at the same state: one application of M^T
  aten_jvp : torch.func.jvp of the restatement through aten (computes the primal as well)

Gsite/s = B * H * W / time.  A JVP call needs at least 14 planes x 4 B per site (6 base planes
including v1, 4 tangents in, 4 out); `min_bytes_rate_TBps` is that minimum over the measured
time and `copy_fraction` its ratio to the 6.29 TB/s measured copy rate.  `jvp_kernels` lists
the device time of each kernel of one JVP call (torch.profiler, a run of its own).

Section 2: `FourDVar.fit(iters=40)` against `IncrementalFourDVar.fit(outer=3, inner=10)` on
`twin_fields(B=4, n=192)`, T = 4 frames of one step, density observed: wall time of one fit
(host clock around the call and a device synchronisation, after one warm-up fit, median over
--fit-reps) and the final J of each.

    python tools/bench_ns_jvp.py [--reps 10] [--inner 5] [--warmup 3] [--fit-reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-pinn-kalman-filter_amd"), REPO, os.path.join(REPO, "tests"),
                os.path.join(REPO, "tools")]
import torch  # noqa: E402

import ns_step_torch_ref as R  # noqa: E402
from bench_ns_vjp import COPY_RATE, event_us, fields, kernel_table  # noqa: E402
from op import ns_step  # noqa: E402
from pinn_kalman.fourdvar import FourDVar, IncrementalFourDVar  # noqa: E402


def op_section(a, dev):
    lines = []
    for what, B, n in (("simulator", 256, 192), ("ukf", 129, 192)):
        (d, v, p), tans = fields(B, n, dev)  # its cotangents serve as tangents
        with torch.no_grad():
            v1 = ns_step.full_step(d, v, p, R.DT, R.DX, compat=False)[1]

        def fwd():
            with torch.no_grad():
                return ns_step.full_step(d, v, p, R.DT, R.DX, compat=False)

        def hip_jvp():
            return ns_step.full_step_jvp(d, v, p, *tans, R.DT, R.DX, v1=v1)

        def hip_vjp():
            return ns_step.full_step_vjp(d, v, p, v1, *tans, R.DT, R.DX)

        def aten_jvp():
            return torch.func.jvp(lambda x, y, z: R.full_step(x, y, z, R.DT, R.DX), (d, v, p),
                                  tuple(tans))[1]

        forms = {"fwd": fwd, "hip_jvp": hip_jvp, "hip_vjp": hip_vjp, "aten_jvp": aten_jvp}
        th, ta = hip_jvp(), aten_jvp()
        diff = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(th, ta)]
        del th, ta
        for fn in forms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():
                times[k].append(event_us(fn, a.inner))
        sites = B * n * n
        res = {"what": f"ns_step tangent-linear model, {what} shape", "shape": [B, n, n],
               "reps": a.reps, "inner": a.inner, "device": torch.cuda.get_device_name(0),
               "tangent_rel_diff_hip_vs_aten": [float(f"{x:.3e}") for x in diff]}
        for k in forms:
            us = statistics.median(times[k])
            res[k] = {"us": round(us, 1), "us_min_max": [round(min(times[k]), 1),
                                                         round(max(times[k]), 1)],
                      "gsite_per_s": round(sites / us * 1e-3, 3)}
        us = res["hip_jvp"]["us"]
        min_bytes = 14 * 4 * sites
        res["hip_jvp"]["min_bytes"] = min_bytes
        res["hip_jvp"]["min_bytes_rate_TBps"] = round(min_bytes / (us * 1e-6) / 1e12, 3)
        res["hip_jvp"]["copy_fraction"] = round(min_bytes / (us * 1e-6) / COPY_RATE, 4)
        res["hip_jvp_faster_than_aten_jvp"] = us < res["aten_jvp"]["us"]
        res["speedup_vs_aten_jvp"] = round(res["aten_jvp"]["us"] / us, 2)
        res["hip_jvp_over_fwd"] = round(us / res["fwd"]["us"], 2)
        res["hip_jvp_over_hip_vjp"] = round(us / res["hip_vjp"]["us"], 2)
        res["jvp_kernels"] = kernel_table(hip_jvp)
        print(json.dumps(res), flush=True)
        lines.append(res)
        torch.cuda.empty_cache()
    return lines


def twin_problem(B, n, T, dev):
    """R.twin_problem at another size, float32 on the device: the observations are the HIP
    step's own rollout of the truth."""
    (d, v, p), (db, vb) = [[t.float().to(dev) for t in ts] for ts in R.twin_fields(B=B, n=n)]
    fd = FourDVar(steps_per_frame=1, dt=R.DT, dx=R.DX)
    with torch.no_grad():
        obs = fd.rollout(torch.cat([d, v, p], 1), T)
    weights = torch.zeros(1, 1, 4, 1, 1, device=dev)
    weights[:, :, 0] = 1.0 / R.TWIN_OBS_VAR
    bw = torch.full((1, 4, 1, 1), 1.0 / R.TWIN_BG_VAR, device=dev)
    return obs, weights, torch.cat([db, vb, p], 1), bw


def fit_section(a, dev):
    B, n, T = 4, 192, R.TWIN_T
    prob = twin_problem(B, n, T, dev)
    adam = FourDVar(steps_per_frame=1, dt=R.DT, dx=R.DX)
    gn = IncrementalFourDVar(steps_per_frame=1, dt=R.DT, dx=R.DX)
    forms = {"adam_iters40": lambda: adam.fit(*prob, iters=R.TWIN_ITERS, lr=R.TWIN_LR),
             "gauss_newton_outer3_inner10": lambda: gn.fit(*prob, outer=3, inner=10)}
    res = {"what": "4D-Var fit on the twin experiment", "shape": [B, n, n], "frames": T,
           "fit_reps": a.fit_reps, "device": torch.cuda.get_device_name(0)}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.fit_reps):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
            hist = out.history.double().cpu()
            res[k] = {"J0": float(hist[0, 0]), "J": float(hist[-1, 0])}
    for k in forms:
        res[k]["wall_ms"] = round(statistics.median(times[k]), 2)
        res[k]["wall_ms_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
    res["sweeps"] = {"adam_iters40": "41 forward + 40 adjoint",
                     "gauss_newton_outer3_inner10": "4 forward + 33 adjoint + 30 tangent-linear"}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ns_jvp: no HIP device")
    dev = torch.device("cuda:0")
    ops, fit = op_section(a, dev), fit_section(a, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"ops": ops, "fit": fit}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
