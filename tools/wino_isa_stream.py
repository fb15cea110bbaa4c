"""Instruction-class stream of the F(2x4) Winograd kernels, from the compiler's assembly.

A developer tool, not a test: the stream depends on the compiler version.  Make the assembly
with the Makefile's flags for conv_winograd.o plus `--cuda-device-only -S`, from csrc/:

    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function \
        -I../../include -munsafe-fp-atomics -fno-slp-vectorize --cuda-device-only -S \
        conv_winograd.hip -o conv_winograd.s
    python tools/wino_isa_stream.py conv_winograd.s [--kernel NAME] [--no-stream]

For each `wino_f24_k16_kernel<PRE, TAILK>` form (or every kernel whose name holds NAME) it
prints the VGPR count and scratch bytes the compiler reports, the number of exec-mask loops
(`s_cbranch_execnz`: a per-lane "waterfall" around an operand the compiler could not prove
uniform), the instruction-class stream of every basic block, and the longest MFMA-free run of
vector arithmetic inside the steps.

Classes, by opcode prefix only:
    M  MFMA (v_mfma)            v  other VALU (v_)         T  transcendental (v_exp, v_rcp, ...)
    r  LDS read (ds_read/load)  w  LDS write (ds_write/store; other ds_ count as r)
    G  VMEM load                S  VMEM store or atomic    X  scratch_
    |  wait (s_waitcnt, s_nop)  B  s_barrier               >  branch (s_branch, s_cbranch, s_endpgm)
Other scalar instructions are counted per block but left out of the stream.

The steps are the basic blocks that hold an MFMA, each up to its last MFMA (what follows the
last step's is the epilogue).  A run is a sequence of M-free instructions from the block's start
or an MFMA to the next MFMA; its length is its number of v and T instructions, whatever else
stands among them.  Scratch instructions inside the steps are those between a block's first
and last MFMA.
"""
import argparse
import re
import sys

TRANS = ("v_exp", "v_rcp", "v_log", "v_sqrt", "v_rsq", "v_sin", "v_cos")
VMEM = ("buffer_", "global_", "flat_", "tbuffer_")


def classify(op):
    if op.startswith("v_mfma"):
        return "M"
    if op.startswith(TRANS):
        return "T"
    if op.startswith("v_"):
        return "v"
    if op.startswith("ds_"):
        return "w" if ("write" in op or "store" in op) else "r"
    if op.startswith("scratch_"):
        return "X"
    if op.startswith(VMEM):
        return "G" if "_load" in op else "S"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "|"
    if op.startswith("s_barrier"):
        return "B"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
        return ">"
    return None  # other scalar


def kernels(text):
    """name -> (list of (block label, [opcodes]), metadata dict)"""
    out = {}
    name, blocks, meta = None, None, None
    label_re = re.compile(r"^([A-Za-z_.$][\w.$]*):")
    for line in text.splitlines():
        m = re.match(r"^\s*\.type\s+([\w.$]+),@function", line)
        if m:
            name, blocks, meta = m.group(1), [("entry", [])], {}
            out[name] = (blocks, meta)
            continue
        if name is None:
            continue
        m = re.match(r"^;\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy):\s*(\d+)", line)
        if m:
            meta[m.group(1)] = int(m.group(2))
            continue
        if re.match(r"^\s*\.amdhsa_kernel\s", line):
            continue
        m = label_re.match(line)
        if m:
            if m.group(1) != name and "NumVgprs" not in meta:
                blocks.append((m.group(1), []))
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") or "NumVgprs" in meta:
            continue
        blocks[-1][1].append(s.split()[0])
    return out


def demangled_form(name):
    m = re.search(r"wino_f24_k16_kernelILb([01])ELb([01])E", name)
    if not m:
        return name
    tf = {"0": "false", "1": "true"}
    return f"wino_f24_k16_kernel<PRE={tf[m.group(1)]}, TAILK={tf[m.group(2)]}>"


def report(name, blocks, meta, stream=True, width=100):
    ops = [o for _, b in blocks for o in b]
    print(f"== {demangled_form(name)}")
    print(f"   VGPRs {meta.get('NumVgprs', '?')}  AGPRs {meta.get('NumAgprs', '?')}  "
          f"scratch {meta.get('ScratchSize', '?')} B  instructions {len(ops)}")
    print(f"   exec-mask loops (s_cbranch_execnz): "
          f"{sum(o.startswith('s_cbranch_execnz') for o in ops)}")
    scratch_in_steps, longest = 0, (0, None)
    for label, b in blocks:
        cls = [classify(o) for o in b]
        if "M" not in cls:
            continue
        last = len(cls) - cls[::-1].index("M")
        scratch_in_steps += cls[cls.index("M"):last].count("X")
        run = 0
        for c in cls[:last]:
            if c == "M":
                if run > longest[0]:
                    longest = (run, label)
                run = 0
            elif c in ("v", "T"):
                run += 1
    nm = sum(classify(o) == "M" for o in ops)
    print(f"   MFMAs {nm}; scratch instructions inside the steps: {scratch_in_steps}")
    print(f"   longest MFMA-free vector run inside the steps: {longest[0]} (block {longest[1]})")
    if not stream:
        return
    for label, b in blocks:
        cls = [classify(o) for o in b]
        s = "".join(c for c in cls if c)
        n_s = sum(c is None for c in cls)
        print(f"   [{label}] {len(b)} instr: M {s.count('M')} v {s.count('v')} T {s.count('T')} "
              f"r {s.count('r')} w {s.count('w')} G {s.count('G')} S {s.count('S')} "
              f"X {s.count('X')} scalar {n_s}")
        for i in range(0, len(s), width):
            print("      " + s[i:i + width])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="wino_f24_k16_kernel")
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    with open(a.asm) as f:
        ks = kernels(f.read())
    sel = sorted(n for n in ks if a.kernel in n)
    if not sel:
        sys.exit(f"no kernel matching {a.kernel!r} in {a.asm}")
    for n in sel:
        report(n, *ks[n], stream=not a.no_stream)


if __name__ == "__main__":
    main()
