#!/usr/bin/env python3
"""Compare two device listings kernel by kernel: `pair_isa_diff.py <parent listing> <branch listing>`.

A listing is what the Makefile's flags plus `-S --cuda-device-only` give for one translation unit (tests/test_spill_gate.py compiles
variant 0 that way).  For every kernel -- matched by its mangled name -- the two sides are compared in

  * the count of each opcode (the first token of every instruction line): order and operands inside a kernel may differ,
  * the figures the compiler prints behind the kernel (`; codeLenInByte = ...`, `; NumVgprs: ...`, `; ScratchSize: ...`,
    `; Occupancy: ...`, `; LDSByteSize: ...` and the rest of that block).

Prints the kernels that differ and how, whether the whole listings are equal apart from the `__hip_cuid_` symbol, and a summary line;
exit status 1 if any kernel differs.  Two directories instead of two files: every `*.s` present in both is compared.
A refactoring of the pair kernel should run this first and see no kernel listed."""
import collections
import os
import re
import sys

FUNC = re.compile(r"^\t\.type\t(\S+),@function")
INFO = re.compile(r"^; (\w[\w .\[\]/]*?)\s*[:=]\s*(\S+)")


def kernels(path):
    """{name: (Counter of opcodes, {figure: value})} of a listing."""
    out, name, in_code = {}, None, False
    for ln in open(path, errors="replace"):
        m = FUNC.match(ln)
        if m:
            name, in_code = m.group(1), True
            out[name] = (collections.Counter(), {})
            continue
        if name is None:
            continue
        if in_code:
            if ln.startswith(".Lfunc_end"):
                in_code = False
            elif ln.startswith("\t") and not ln.startswith("\t."):
                out[name][0][ln.split()[0]] += 1
        else:
            m = INFO.match(ln)
            if m:
                out[name][1].setdefault(m.group(1), m.group(2))
    return out


def same_text(a, b):
    strip = lambda p: [re.sub(r"__hip_cuid_\w+", "__hip_cuid_", ln) for ln in open(p, errors="replace")]      # noqa: E731
    return strip(a) == strip(b)


def compare(a, b):
    ka, kb = kernels(a), kernels(b)
    bad = 0
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print(f"{name}\n    only in the {'parent' if name in ka else 'branch'} listing")
            bad += 1
            continue
        (ha, fa), (hb, fb) = ka[name], kb[name]
        lines = [f"    {op}: {ha[op]} -> {hb[op]}" for op in sorted(set(ha) | set(hb)) if ha[op] != hb[op]]
        lines += [f"    {k}: {fa.get(k)} -> {fb.get(k)}" for k in sorted(set(fa) | set(fb)) if fa.get(k) != fb.get(k)]
        if lines:
            print(name + "\n" + "\n".join(lines))
            bad += 1
    text = "equal apart from the __hip_cuid_ symbol" if same_text(a, b) else "texts differ"
    print(f"{os.path.basename(b)}: {len(set(ka) | set(kb))} kernels, {bad} differ; listings: {text}")
    return bad


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = sys.argv[1:]
    if os.path.isdir(a):
        names = sorted(n for n in os.listdir(a) if n.endswith(".s") and os.path.exists(os.path.join(b, n)))
        bad = sum(compare(os.path.join(a, n), os.path.join(b, n)) for n in names)
    else:
        bad = compare(a, b)
    sys.exit(1 if bad else 0)
