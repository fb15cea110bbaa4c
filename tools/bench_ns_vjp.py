"""ns_step forward + backward: the HIP adjoint (csrc/ns_step_vjp.hip) against aten autograd of
the plain-torch restatement (tests/ns_step_torch_ref.py) on the same device, float32, at the
simulator's shape (B = 256, 192 x 192) and the UKF's (129 fields of 192 x 192).

Per shape, three variants alternate inside every repetition (all see the same clocks), timed
with device events around --inner back-to-back calls, median over --reps repetitions:

  fwd       : ns_step.full_step(compat=False) under no_grad -- the simulator line, for scale
  hip_fwbw  : full_step with a graph + backward of all three outputs (HIP adjoint)
  aten_fwbw : the restatement forward + backward through aten

Gsite/s = B * H * W / time.  For hip_fwbw the algorithm needs at least 14 planes x 4 B per
site for the backward (6 inputs / saved outputs, 4 cotangents, 4 gradients) on top of the
forward's 8 (4 read, 4 written); `min_bytes_rate` is that minimum over the measured time and
`copy_fraction` its ratio to the 6.29 TB/s measured copy rate.  `backward_kernels` lists the
device time of each backward kernel of one call (torch.profiler, a run of its own).

    python tools/bench_ns_vjp.py [--reps 10] [--inner 5] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-pinn-kalman-filter_amd"), REPO, os.path.join(REPO, "tests")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

import ns_step_torch_ref as R  # noqa: E402
from op import ns_step  # noqa: E402

COPY_RATE = 6.29e12  # measured device copy rate, B/s


def fields(B, n, dev):
    """Smooth fields of the twin experiment's kind, velocity (0.6, -0.5) + 0.1 x pooled noise:
    no component comes near 0, so the two variants take the same upwind branches."""
    g = torch.Generator(device=dev).manual_seed(0)

    def smooth(c):
        x = torch.randn(B, c, n, n, device=dev, generator=g)
        for _ in range(3):
            x = F.avg_pool2d(x, 3, stride=1, padding=1)
        return x / x.abs().max()

    dens = 0.5 + 0.2 * smooth(1)
    vel = torch.tensor([0.6, -0.5], device=dev).view(1, 2, 1, 1) + 0.1 * smooth(2)
    pres = 0.002 * smooth(1)
    cots = [torch.randn(B, c, n, n, device=dev, generator=g) for c in (1, 2, 1)]
    return (dens, vel, pres), cots


def event_us(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def kernel_table(fn):
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            name = e.name.replace("(anonymous namespace)::", "").replace("void ", "")
            name = name.split("(")[0][:48]
            us, n = rows.get(name, (0.0, 0))
            rows[name] = (us + e.device_time, n + 1)
    return {k: {"us": round(us, 1), "launches": n} for k, (us, n) in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for what, B, n in (("simulator", 256, 192), ("ukf", 129, 192)):
        (d, v, p), cots = fields(B, n, dev)
        leaves = [t.clone().requires_grad_(True) for t in (d, v, p)]

        def fwd():
            with torch.no_grad():
                return ns_step.full_step(d, v, p, R.DT, R.DX, compat=False)

        def hip_fwbw():
            out = ns_step.full_step(*leaves, R.DT, R.DX, compat=False)
            return torch.autograd.grad(out, leaves, cots)

        def aten_fwbw():
            out = R.full_step(*leaves, R.DT, R.DX)
            return torch.autograd.grad(out, leaves, cots)

        forms = {"fwd": fwd, "hip_fwbw": hip_fwbw, "aten_fwbw": aten_fwbw}
        gh, ga = hip_fwbw(), aten_fwbw()
        diff = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(gh, ga)]
        del gh, ga
        for fn in forms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():
                times[k].append(event_us(fn, a.inner))
        sites = B * n * n
        res = {"what": f"ns_step forward+backward, {what} shape", "shape": [B, n, n],
               "reps": a.reps, "inner": a.inner, "device": torch.cuda.get_device_name(0),
               "grad_rel_diff_hip_vs_aten": [float(f"{x:.3e}") for x in diff]}
        for k in forms:
            us = statistics.median(times[k])
            res[k] = {"us": round(us, 1), "us_min_max": [round(min(times[k]), 1),
                                                         round(max(times[k]), 1)],
                      "gsite_per_s": round(sites / us * 1e-3, 3)}
        us = res["hip_fwbw"]["us"]
        min_bytes = (8 + 14) * 4 * sites
        res["hip_fwbw"]["min_bytes"] = min_bytes
        res["hip_fwbw"]["min_bytes_rate_TBps"] = round(min_bytes / (us * 1e-6) / 1e12, 3)
        res["hip_fwbw"]["copy_fraction"] = round(min_bytes / (us * 1e-6) / COPY_RATE, 4)
        res["hip_faster_than_aten"] = res["hip_fwbw"]["us"] < res["aten_fwbw"]["us"]
        res["speedup_vs_aten"] = round(res["aten_fwbw"]["us"] / res["hip_fwbw"]["us"], 2)
        out = ns_step.full_step(*leaves, R.DT, R.DX, compat=False)
        res["backward_kernels"] = kernel_table(lambda: torch.autograd.grad(out, leaves, cots))
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
        del out, leaves
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
