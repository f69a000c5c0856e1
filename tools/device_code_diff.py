#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (what a host-only refactor must leave alone).  Each side is one or
more listings: the library's kernels are spread over its translation units (_lib.UNITS: pnr_api.hip and pnr_queries.hip for the
env engine, pnr_learn.hip for the learner), and a kernel may move between them.

    for u in pnr_api pnr_queries; do                 # at the old commit: into before/, at the new one: into after/
        hipcc <_lib.HIPCC_FLAGS> --cuda-device-only -S -o before/$u.s pioneer_amd/csrc/$u.hip
    done
    python tools/device_code_diff.py --before before/*.s --after after/*.s

Order is ignored: each listing is split at the kernel symbols into the function body (label .. its .Lfunc_end) and the
.amdhsa_kernel descriptor block, compared as text.  For a body that differs the per-opcode count delta (after - before) is printed
with it: "reordered only" when the instruction mix is the same.  Masked: the function's index in the listing, which numbers its local labels
(.LBB<i>_<k>, .Lfunc_end<i>), and the assembler comments, which quote those labels.  A kernel that two listings of one side hold
is an error (two units would compile, and the library would hold, the same kernel).  --by-template-arguments pairs the kernels by
their mangled name up to the end of the template argument list, without the parameter types (a kernel whose parameter types are
written in terms of a role enum or a type list, dyn_world_kernel, is renamed by an addition to either; its code need not change),
and masks the name inside body and descriptor.  Exit status 0: no such kernel, same kernel
names, no body or descriptor differs; then the number of kernels each listing holds is printed too."""
import argparse
import collections
import re
import sys


def short_name(name):
    """the mangled name up to the end of its template argument list (the whole name of a kernel that is no template)"""
    cut = name.find("EEv")
    return name if cut < 0 else name[:cut + 2]


def kernels(path, by_template_arguments=False):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel\n", text, re.M | re.S):
        name = m.group(1)
        body = re.search(r"^%s:.*?^(\.Lfunc_end(\d+)):\n" % re.escape(name), text, re.M | re.S)
        idx = body.group(2)
        code = re.sub(r"[ \t]*;.*$", "", body.group(0), flags=re.M)
        k = (re.sub(r"(\.L[A-Za-z_]+)%s(?!\d)" % idx, r"\1#", code), m.group(0))
        if by_template_arguments:
            short = short_name(name)
            assert short not in out, f"{path}: two kernels shorten to {short}"
            out[short] = tuple(t.replace(name, short) for t in k)
        else:
            out[name] = k
    return out


def side(paths, by_template_arguments=False):
    """({kernel: (body, descriptor)}, {kernel: its listing}, [(kernel, listing, listing) held twice]) of one side's listings"""
    merged, where, twice = {}, {}, []
    for path in paths:
        for name, k in kernels(path, by_template_arguments).items():
            if name in merged:
                twice.append((name, where[name], path))
            merged[name], where[name] = k, path
    return merged, where, twice


def opcode_delta(x, y):
    """after - before counts of every opcode whose count differs between two function bodies"""
    ops = lambda body: collections.Counter(ln.split()[0] for ln in body.splitlines() if ln.startswith("\t") and not ln.startswith("\t."))
    cx, cy = ops(x), ops(y)
    return {o: cy[o] - cx[o] for o in sorted(set(cx) | set(cy)) if cx[o] != cy[o]}


def main(before, after, by_template_arguments=False, new_allowed=False):
    (a, a_where, a_twice), (b, b_where, b_twice) = side(before, by_template_arguments), side(after, by_template_arguments)
    for when, twice in (("before", a_twice), ("after", b_twice)):
        for name, p, q in twice:
            print(f"twice {when}: {name}  ({p}, {q})")
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    bodies = [k for k in a if k in b and a[k][0] != b[k][0]]
    descs = [k for k in a if k in b and a[k][1] != b[k][1]]
    for what, names in (("only before", gone), ("only after", new), ("body differs", bodies), ("descriptor differs", descs)):
        for k in names:
            delta = opcode_delta(a[k][0], b[k][0]) if names is bodies else None
            print(f"{what}: {k}" + ("" if delta is None else f"  {delta or 'reordered only'}"))
    bad = bool(a_twice or b_twice or gone or (new and not new_allowed) or bodies or descs)
    if not bad:
        for when, where in (("before", a_where), ("after", b_where)):
            for path, count in collections.Counter(where.values()).items():
                print(f"{when}: {count:4d} kernels from {path}")
    print(f"{len(a)} kernels before, {len(b)} after; names {'equal' if not gone and not new else 'DIFFER'}; "
          f"{len(a_twice) + len(b_twice)} kernels twice on a side; {len(bodies)} bodies differ, {len(descs)} descriptors differ")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--before", nargs="+", required=True, metavar="LISTING")
    ap.add_argument("--after", nargs="+", required=True, metavar="LISTING")
    ap.add_argument("--by-template-arguments", action="store_true", help="pair kernels by name and template arguments, not parameter types")
    ap.add_argument("--new-allowed", action="store_true", help="kernels only the after side holds are listed but are no failure (a feature adds kernels)")
    args = ap.parse_args()
    sys.exit(main(args.before, args.after, args.by_template_arguments, args.new_allowed))
