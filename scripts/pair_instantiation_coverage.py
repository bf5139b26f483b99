"""Which of the 264 instantiations of the two-sub-steps kernel (csrc/evp_fused2.hip, k_pair) a test run executed.

Input: the kernel-name statistics of kernel-trace runs of the GPU tests, e.g.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m pytest tests/test_gpu_evp.py ... -m gpu -q

(kernel trace only -- no counters --, the program after `--`, under a time limit of its own).  Every process of the run writes a
`*kernel_stats.csv` of its own; this script takes files or directories (searched recursively), maps each k_pair<...> name -- demangled
or mangled -- onto the keys of tests/golden/spill_table.json and prints which keys ran, with their call counts, and which did not,
grouped by the template argument that no traced case selects and with what the same statistics say of each one's twins.

    python scripts/pair_instantiation_coverage.py OUT_BEFORE                       # one run
    python scripts/pair_instantiation_coverage.py OUT_BEFORE --with OUT_NEW        # a second set of runs on top of the first
    ... --markdown                                                                  # tables for profiles/*.md
    ... --expected                                                                  # tests/pair_matrix.py against the LAST set of runs

--expected: every key the selection rule of tests/pair_matrix.py (expected_key over MATRIX x transports x first sub-step, as
tests/test_gpu_pair_matrix.py runs them) names, against the keys the last set of statistics executed.  Expected but not executed: a
mistake in the mirror rule or a fall-back of the library -- to be explained or fixed; executed but not expected: launches the rule
does not describe (the trailing single sub-step of an odd count has the other order; other test files).

A measurement, not a gate: no test reads its result.
"""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "spill_table.json")
# (WALLS, MASK, FORCE, FD, EXTRA) -> the translation unit (CSI_PAIR_VARIANT) that instantiates it
VARIANT = {(0, 0, 0, 0, 0): 0, (1, 0, 0, 0, 0): 1, (1, 1, 0, 0, 0): 2, (1, 0, 1, 0, 0): 3, (1, 1, 1, 0, 0): 4, (1, 0, 1, 1, 0): 5, (1, 1, 1, 1, 0): 6,
           (1, 0, 1, 0, 1): 7, (1, 1, 1, 0, 1): 8, (1, 0, 1, 0, 2): 9, (1, 1, 1, 0, 2): 10}
FAMILY = {0: "plain", 1: "walls", 2: "mask", 3: "array forcing", 4: "mask + array forcing", 5: "free drift", 6: "mask + free drift",
          7: "model.forcing / immersed flux", 8: "mask + model.forcing / immersed flux", 9: "wind-drag / bottom-stress arrays",
          10: "mask + wind-drag / bottom-stress arrays"}


def key_of(name):
    """spill-table key of a kernel name, None if it is not a k_pair instantiation
    template <bool UNI, bool AUF, bool WALLS, bool MASK, bool FORCE, bool FD, int CF, bool FULL, bool PEER, int EXTRA, bool DLD>"""
    m = re.search(r"k_pair<([^>]*)>", name)
    if m:
        a = [{"true": 1, "false": 0}.get(x.strip(), x.strip()) for x in m.group(1).split(",")]
        a = [int(re.sub(r"[^0-9-]", "", str(x))) for x in a]
    else:
        m = re.search(r"k_pairI(.*?)EEv", name)
        if not m:
            return None
        a = [int(x) for x in re.findall(r"L[bi](\d+)E", m.group(1))]
    a += [0] * (11 - len(a))
    uni, auf, walls, mask, force, fd, cf, full, peer, extra, dld = a[:11]
    v = VARIANT[(walls, mask, force, fd, extra)]
    return f"v{v} UNI{uni} AUF{auf} CF{cf} FULL{full} PEER{peer} X{extra} DLD{dld}"


def read(paths):
    """{key: calls} over every *kernel_stats.csv under the paths"""
    files = []
    for p in paths:
        files += sorted(glob.glob(os.path.join(p, "**", "*kernel_stats.csv"), recursive=True)) if os.path.isdir(p) else [p]
    calls = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                k = key_of(row.get("Name", ""))
                if k:
                    calls[k] = calls.get(k, 0) + int(row.get("Calls", 0) or 0)
    return calls, len(files)


def describe(key):
    f = dict(x for x in re.findall(r"([A-Z]+)(\d+)", key))
    v = int(re.match(r"v(\d+)", key).group(1))
    return (f"{FAMILY[v]}, {'uniform' if f['UNI'] == '1' else ('per-point' if f['FULL'] == '1' else 'per-row')} coefficients, "
            f"{'u' if f['AUF'] == '1' else 'v'}-first" + (f", forcing kinds fixed ({f['CF']})" if f["CF"] != "0" else "") +
            (", peer flags" if f["PEER"] == "1" else "") + (", neighbours with other row strides" if f["DLD"] == "1" else ""))


# what selects the argument that keeps an instantiation from running (launch_fused_pair and its callers in csi_launch.hip)
WHY = {"untiled": "PEER0: no untiled case of the traced tests has this family with these coefficients (UNI / per-row / FULL) and "
                  "compile-time forcing kinds (CF), from this parity of the first sub-step",
       "peer": "PEER1 DLD0: selected only for a tile with a peer-connected side (non-zero launch sequence number); no tiled case of the "
               "traced tests has this family with these coefficients and forcing kinds, from this parity of the first sub-step",
       "dld": "DLD1: selected only when a peer-connected neighbour's arrays have another row stride than the tile's own (bit 63 of the "
              "launch sequence number, from peer.dld): two local tiles of different widths; a self-connected tile is its own neighbour"}


def twin(key, **changed):
    for name, value in changed.items():
        key = re.sub(rf"\b{name}\d+", f"{name}{value}", key)
    return key


def never_executed(calls, table):
    """[(group, [(key, which of its twins -- the other order, DLD0, untiled -- were executed)])], groups as in WHY"""
    groups = {"untiled": [], "peer": [], "dld": []}
    said = lambda k: "ran" if calls.get(k) else "did not run"
    for k in table:
        if calls.get(k):
            continue
        f = dict(re.findall(r"([A-Z]+)(\d+)", k))
        group = "dld" if f["DLD"] == "1" else ("peer" if f["PEER"] == "1" else "untiled")
        beside = [f"its {'v' if f['AUF'] == '1' else 'u'}-first twin {said(twin(k, AUF=1 - int(f['AUF'])))}"]
        if group == "dld":
            beside.append(f"its DLD0 twin {said(twin(k, DLD=0))}")
        if group != "untiled":
            beside.append(f"its untiled twin {said(twin(k, PEER=0, DLD=0))}")
        groups[group].append((k, "; ".join(beside)))
    return [(g, rows) for g, rows in groups.items() if rows]


def summary(title, calls, table, md):
    ran = [k for k in table if calls.get(k)]
    auf1 = [k for k in ran if " AUF1 " in k]
    print(f"{title}: {len(ran)} of {len(table)} instantiations executed ({len(ran) - len(auf1)} v-first, {len(auf1)} u-first)")
    unknown = sorted(set(calls) - set(table))
    if unknown:
        print("  names that are not in the table:", unknown)
    return ran


def expected_by_the_table():
    """{key: [(case, transport, first sub-step)]} of tests/pair_matrix.py, and its UNREACHABLE dict"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pair_matrix as pm
    return pm.selected(), pm.UNREACHABLE, set(pm.TARGETS)


def compare_expected(calls, table, md):
    expected, unreachable, targets = expected_by_the_table()
    ran = {k for k in table if calls.get(k)}
    print(f"\nexpected by the table: {len(expected)} keys; executed in the trace: {len(ran)}; both: {len(ran & set(expected))}; "
          f"targets (never executed before) executed: {len(ran & targets)} of {len(targets)}")
    missing = sorted(set(expected) - ran)
    print(f"expected but NOT executed: {len(missing)}")
    for k in missing:
        who = ", ".join(f"{n} ({t}, first = {f})" for n, t, f in expected[k][:3])
        print(f"| `{k}` | {who} |" if md else f"  {k:44s} {who}")
    beyond = sorted(ran - set(expected))
    print(f"executed but not expected: {len(beyond)}")
    for k in beyond:
        print(f"| `{k}` | {calls[k]} |" if md else f"  {k:44s} {calls[k]:8d}")
    print(f"listed as unreachable (the library refuses the configuration on tiles): {len(unreachable)}")
    for k, why in unreachable.items():
        print(f"| `{k}` | {why} | {'EXECUTED' if k in ran else 'not executed'} |" if md else f"  {k:44s} {why}")
    return 1 if missing else 0


def main(argv):
    md = "--markdown" in argv
    want_expected = "--expected" in argv
    argv = [a for a in argv if a not in ("--markdown", "--expected")]
    extra = []
    if "--with" in argv:
        i = argv.index("--with")
        argv, extra = argv[:i], argv[i + 1:]
    if not argv:
        print(__doc__)
        return 2
    table = sorted(json.load(open(TABLE)))
    before, nb = read(argv)
    print(f"{nb} statistics file(s) in the first set, {sum(before.values())} k_pair launches")
    ran_before = summary("first set", before, table, md)
    both = dict(before)
    if extra:
        more, nm = read(extra)
        print(f"{nm} statistics file(s) in the second set, {sum(more.values())} k_pair launches")
        summary("second set alone", more, table, md)
        for k, n in more.items():
            both[k] = both.get(k, 0) + n
        ran = summary("both sets", both, table, md)
        print("\ninstantiations only the second set executed:")
        for k in ran:
            if k not in ran_before:
                print(f"| `{k}` | {both[k]} | {describe(k)} |" if md else f"  {k:44s} {both[k]:8d}  {describe(k)}")
    print("\nexecuted (key, launches):")
    for k in table:
        if both.get(k):
            print(f"| `{k}` | {before.get(k, 0)} | {both[k]} |" if md else f"  {k:44s} {before.get(k, 0):8d} {both[k]:8d}")
    print("\nnever executed:")
    for group, rows in never_executed(both, table):
        print(f"\n{len(rows)} instantiations -- {WHY[group]}\n" + ("\n| instantiation | | measured beside it |\n|---|---|---|" if md else ""))
        for k, beside in rows:
            print(f"| `{k}` | {describe(k)} | {beside} |" if md else f"  {k:44s} {describe(k)}; {beside}")
    if want_expected:
        return compare_expected(more if extra else before, table, md)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
