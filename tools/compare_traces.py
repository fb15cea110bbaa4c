"""Verdict over the outputs of trace_launches.py:

    python tools/compare_traces.py parent1.pt branch1.pt parent2.pt branch2.pt ...

Traces are compared per workload (the first word of each line); where two differ, every line
that is in one and not in the other is printed.  Tensors: how many are torch.equal, and the
largest difference per workload."""
import collections
import difflib
import itertools
import sys

import torch

runs = {p.rsplit("/", 1)[-1].removesuffix(".pt"): torch.load(p) for p in sys.argv[1:]}
names = list(runs)  # parent1 branch1 parent2 branch2 ...


def by_section(trace):
    d = collections.OrderedDict()
    for line in trace:
        d.setdefault(line.split(" ", 1)[0], []).append(line)
    return d


def launches(lines):
    return [ln for ln in lines if "supported(" not in ln and "_bytes(" not in ln]


def traces(a, b):
    ta, tb = by_section(runs[a]["trace"]), by_section(runs[b]["trace"])
    for sec in ta:
        la, lb = ta[sec], tb.get(sec, [])
        same = "IDENTICAL" if la == lb else "DIFFERENT"
        print(f"trace {a} vs {b} [{sec}]: {same} ({len(la)} / {len(lb)} lines; launches only: "
              f"{len(launches(la))} / {len(launches(lb))})")
        if la != lb:
            for ln in difflib.unified_diff(la, lb, a, b, n=0, lineterm=""):
                if not ln.startswith(("---", "+++", "@@")):
                    print("    " + ln)


def tensors(a, b):
    ta, tb = runs[a]["tensors"], runs[b]["tensors"]
    assert ta.keys() == tb.keys()
    equal = sum(torch.equal(ta[k], tb[k]) for k in ta)
    print(f"tensors {a} vs {b}: {equal} of {len(ta)} torch.equal")
    worst = {}
    for k in ta:
        if not torch.equal(ta[k], tb[k]):
            sec = k.split("/", 1)[0]
            d = float((ta[k].double() - tb[k].double()).abs().max())
            n, w = worst.get(sec, (0, (-1.0, None, 0.0)))
            worst[sec] = (n + 1, max(w, (d, k, float(ta[k].abs().max()))))
    for sec, (n, (d, k, mag)) in worst.items():
        print(f"  {sec}: {n} differ; largest |diff| {d:.3e} in {k} (max |value| {mag:.3e})")


parents, branches = names[0::2], names[1::2]
for a, b in list(zip(parents, branches)) + [(t[0], u) for t in (parents, branches) for u in t[1:]]:
    traces(a, b)
for a, b in itertools.chain(itertools.product(parents, branches),
                            itertools.combinations(parents, 2), itertools.combinations(branches, 2)):
    tensors(a, b)
