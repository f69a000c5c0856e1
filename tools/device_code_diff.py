#!/usr/bin/env python3
"""Compare the device code of two builds of one translation unit, kernel by kernel (what a host-only refactor must leave alone).

    hipcc <_lib.HIPCC_FLAGS> --cuda-device-only -S -o before.s pioneer_amd/csrc/pnr_api.hip      # at the old commit
    hipcc <_lib.HIPCC_FLAGS> --cuda-device-only -S -o after.s pioneer_amd/csrc/pnr_api.hip       # at the new one
    python tools/device_code_diff.py before.s after.s

Order is ignored: each listing is split at the kernel symbols into the function body (label .. its .Lfunc_end) and the
.amdhsa_kernel descriptor block, compared as text.  For a body that differs the per-opcode count delta (after - before) is printed
with it: "reordered only" when the instruction mix is the same.  Masked: the function's index in the listing, which numbers its local labels
(.LBB<i>_<k>, .Lfunc_end<i>), and the assembler comments, which quote those labels.  Exit status 0: same kernel names, no body
or descriptor differs."""
import collections
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel\n", text, re.M | re.S):
        name = m.group(1)
        body = re.search(r"^%s:.*?^(\.Lfunc_end(\d+)):\n" % re.escape(name), text, re.M | re.S)
        idx = body.group(2)
        code = re.sub(r"[ \t]*;.*$", "", body.group(0), flags=re.M)
        out[name] = (re.sub(r"(\.L[A-Za-z_]+)%s(?!\d)" % idx, r"\1#", code), m.group(0))
    return out


def opcode_delta(x, y):
    """after - before counts of every opcode whose count differs between two function bodies"""
    ops = lambda body: collections.Counter(ln.split()[0] for ln in body.splitlines() if ln.startswith("\t") and not ln.startswith("\t."))
    cx, cy = ops(x), ops(y)
    return {o: cy[o] - cx[o] for o in sorted(set(cx) | set(cy)) if cx[o] != cy[o]}


def main(before, after):
    a, b = kernels(before), kernels(after)
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    bodies = [k for k in a if k in b and a[k][0] != b[k][0]]
    descs = [k for k in a if k in b and a[k][1] != b[k][1]]
    for what, names in (("only before", gone), ("only after", new), ("body differs", bodies), ("descriptor differs", descs)):
        for k in names:
            delta = opcode_delta(a[k][0], b[k][0]) if names is bodies else None
            print(f"{what}: {k}" + ("" if delta is None else f"  {delta or 'reordered only'}"))
    print(f"{len(a)} kernels before, {len(b)} after; names {'equal' if not gone and not new else 'DIFFER'}; "
          f"{len(bodies)} bodies differ, {len(descs)} descriptors differ")
    return 1 if gone or new or bodies or descs else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
