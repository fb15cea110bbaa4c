#!/usr/bin/env python3
"""Per-kernel comparison of two gfx950 device assembly files (no GPU needed):

    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only -S x.hip -o A.s
    tools/kernel_isa_diff.py A.s B.s

prints `same`, `DIFF`, `gone` or `new` per kernel, comparing the whole instruction list and the
kernel descriptor (registers, accumulation offset, scratch, LDS); exit status 1 on any DIFF.
Kernels pair up by demangled name without template arguments; several instances of one template
pair by argument values, where one side may lack arguments the other has (a template parameter
that had a single value was removed).
"""
import re
import subprocess
import sys

META = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size",
        "group_segment_fixed_size")


def kernels(path):
    """[(base name, template args, pretty name, lines, descriptor summary)]"""
    text = re.sub(r"[ \t]*(;|//).*", "", open(path).read())       # comments
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)                     # labels carry a function index
    out = []
    for name, body in re.findall(r"^(_Z\w+):\n(.*?)^\.Lfunc_end", text, re.M | re.S):
        lines = [ln.strip().replace(name, "KERNEL") for ln in body.split("\n")]
        lines = [ln for ln in lines if ln and not re.match(r"\.(loc\b|file\b|Ltmp\d+)", ln)
                 and "__hip_cuid_" not in ln]
        if not any(ln.startswith(".amdhsa_kernel") for ln in lines):
            continue  # a device function, not a kernel
        pretty = subprocess.run(["c++filt", name], capture_output=True, text=True,
                                check=True).stdout.strip()
        pretty = re.sub(r"^void |\(anonymous namespace\)::", "", pretty).split("(")[0]
        base, _, args = pretty.partition("<")
        meta = " ".join(ln[len(".amdhsa_"):].replace(" ", "=") for ln in lines
                        if ln.startswith(".amdhsa_") and ln.split()[0][len(".amdhsa_"):] in META)
        out.append((base, args.rstrip(">").split(", ") if args else [], pretty, lines, meta))
    return out


def within(short, long):
    """short is long with some elements left out"""
    it = iter(long)
    return all(x in it for x in short)


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    bad = 0
    for ka in a:
        match = [kb for kb in b if kb[0] == ka[0]
                 and (within(kb[1], ka[1]) or within(ka[1], kb[1]))]
        if len(match) != 1:
            print(f"gone  {ka[2]}")
            continue
        kb = match[0]
        b.remove(kb)
        same = ka[3] == kb[3]
        bad += not same
        renamed = "" if ka[2] == kb[2] else f" -> {kb[2]}"
        meta = ka[4] if ka[4] == kb[4] else f"{ka[4]} -> {kb[4]}"
        print(f"{'same' if same else 'DIFF'}  {ka[2]}{renamed}  [{len(ka[3])} lines; {meta}]")
    for kb in b:
        print(f"new   {kb[2]}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
