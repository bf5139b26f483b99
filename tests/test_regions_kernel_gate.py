"""Generated code of the regional reduction (csrc/regions.hip; hipcc cross-compiles, nothing runs): from the compiler's resource-usage
remarks the build keeps beside the object (csrc/regions.res) -- no scratch and no spills in any instantiation.  Nothing else is read
from the generated code."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaseaice.jl_amd", "csrc")


def remarks():
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC], stdout=subprocess.DEVNULL)      # (no-op when the library is up to date)
    blocks = open(os.path.join(CSRC, "regions.res")).read().split("remark: Function Name: ")[1:]
    out = {}
    for b in blocks:
        g = lambda k: int(re.search(k + r"[^:]*: (\d+)", b).group(1))      # noqa: E731
        out[b.split()[0]] = dict(scratch=g("ScratchSize"), vspill=g("VGPRs Spill"), sspill=g("SGPRs Spill"), vgprs=g(r"\bVGPRs"), agprs=g("AGPRs"))
    return out


def test_seven_instantiations_without_scratch_or_spills():
    r = remarks()
    names = sorted(r)
    assert len(names) == 7, names
    # k_regions_partial<MK, MASK>: three metric kinds, with and without a land mask; the finishing kernel's regional instantiation
    for mk in (0, 1, 2):
        for mask in (0, 1):
            assert sum(f"k_regions_partialILi{mk}ELb{mask}E" in n for n in names) == 1, (mk, mask, names)
    assert sum("finish_records" in n and "RegionKinds" in n for n in names) == 1
    for n, v in r.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vspill"] == 0 and v["sspill"] == 0, n
        # sixteen cells held in registers, not in the accumulation registers that stand in for spills: a block of 256 threads has 512
        # registers per thread, half of them vector registers proper
        assert v["agprs"] == 0 and v["vgprs"] <= 256, n
