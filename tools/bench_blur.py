"""Blur measurement operator (op.blur, csrc/blur.hip) against its aten composition on the same
device: A and A^T at [16, 1, 256, 256], K = 13, stride 1 and 4.

The aten form is what a user would write without the op: an index-gather symmetric pad,
F.conv2d with the taps as a column then as a row, the strided slice; its A^T is autograd's
backward of that composition.  Two figures per form and direction:

  call_us   : HIP events around --inner back-to-back calls, per call, median over --reps
              repetitions; native and aten alternate inside every repetition.  Includes the
              host's launch gaps where the host is the slower side.
  kernel_us : device time of the kernels of one call under torch.profiler (a run of its own,
              after the timed loops), summed.

hbm_fraction = algorithmic bytes (the input read once, the output written once) over
kernel_us, over the 8 TB/s peak.  Prints one JSON line per stride.

    python tools/bench_blur.py [--reps 20] [--inner 50] [--warmup 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-pinn-kalman-filter_amd"), REPO]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

from op import blur  # noqa: E402

HBM_PEAK = 8e12


def symm_index(n, p, device):
    i = torch.arange(-p, n + p, device=device)
    return torch.where(i < 0, -1 - i, torch.where(i >= n, 2 * n - 1 - i, i))


def aten_blur(x, col, row, ih, iw, s):
    B, C, H, W = x.shape
    xp = x[:, :, ih][:, :, :, iw]
    t = F.conv2d(F.conv2d(xp.reshape(B * C, 1, ih.numel(), iw.numel()), col), row)
    o = (s - 1) // 2
    t = t[:, :, o::s, o::s]
    return t.reshape(B, C, t.shape[2], t.shape[3])


def event_us(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def kernel_us(fn):
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kern = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and "Memcpy" not in e.name and "Memset" not in e.name]
    return sum(e.device_time for e in kern), len(kern)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, C, H, W, K = 16, 1, 256, 256, 13
    taps = blur.gaussian_taps(4.0, K)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    lines = []
    for s in (1, 4):
        Ho, Wo = blur.out_size(H, W, K, s)
        gy = torch.randn(B, C, Ho, Wo, generator=g).to(dev)
        gt = taps.flip(0).to(dev, torch.float32)
        col, row = gt.view(1, 1, K, 1), gt.view(1, 1, 1, K)
        ih, iw = symm_index(H, K // 2, dev), symm_index(W, K // 2, dev)
        xg = x.clone().requires_grad_()
        ya = aten_blur(xg, col, row, ih, iw, s)
        forms = {
            "native_A": lambda: blur.blur2d(x, taps, s),
            "aten_A": lambda: aten_blur(x, col, row, ih, iw, s),
            "native_AT": lambda: blur.blur2d_adjoint(gy, taps, s, (H, W)),
            "aten_AT": lambda: torch.autograd.grad(ya, xg, gy, retain_graph=True)[0],
        }
        # the two forms compute the same thing (float32 summation order apart)
        scale = float(x.abs().max())
        dA = float((forms["native_A"]() - forms["aten_A"]()).abs().max()) / scale
        dAT = float((forms["native_AT"]() - forms["aten_AT"]()).abs().max()) / float(gy.abs().max())
        for fn in forms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():  # interleaved: every form sees the same clocks
                times[k].append(event_us(fn, a.inner))
        nbytes = 4 * B * C * (H * W + Ho * Wo)
        res = {"what": "blur2d A / A^T vs aten composition", "shape": [B, C, H, W], "K": K,
               "stride": s, "reps": a.reps, "inner": a.inner, "algorithmic_bytes": nbytes,
               "device": torch.cuda.get_device_name(0), "max_diff_A": dA, "max_diff_AT": dAT}
        for k, fn in forms.items():
            us, n = kernel_us(fn)
            res[k] = {"call_us": round(statistics.median(times[k]), 2),
                      "call_us_min_max": [round(min(times[k]), 2), round(max(times[k]), 2)],
                      "kernel_us": round(us, 2), "kernels": n,
                      "hbm_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4) if us else None}
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
