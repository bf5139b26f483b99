"""Generated code of the tracer kernels (csrc/tracers.hip; hipcc cross-compiles, nothing runs): from the compiler's resource-usage
remarks the build keeps beside the object (csrc/tracers.res) -- no scratch and no spills in any instantiation, and the instantiations
the launch rule of tracers.hip implies.  Nothing else is read from the generated code."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaseaice.jl_amd", "csrc")


def remarks():
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC], stdout=subprocess.DEVNULL)      # (no-op when the library is up to date)
    blocks = open(os.path.join(CSRC, "tracers.res")).read().split("remark: Function Name: ")[1:]
    out = {}
    for b in blocks:
        g = lambda k: int(re.search(k + r"[^:]*: (\d+)", b).group(1))      # noqa: E731
        out[b.split()[0]] = dict(scratch=g("ScratchSize"), vspill=g("VGPRs Spill"), sspill=g("SGPRs Spill"), vgprs=g(r"\bVGPRs"), agprs=g("AGPRs"),
                                 lds=g("LDS Size"))
    return out


def test_instantiations_without_scratch_or_spills():
    r = remarks()
    names = sorted(r)
    # k_tracer_tendencies<SCHEME, FAST, W32, NTR>: six schemes, of which the three WENO ones also with f32 weights (9 forms), STRICT and
    # FAST, 1 / 2 / 4 tracers per thread: 54; the two point-wise kernels: 56 in all
    stencil = [n for n in names if "k_tracer_tendencies" in n]
    assert len(stencil) == 54 and len(names) == 56, (len(stencil), len(names))
    code = lambda s: f"Li{s}E" if s > 0 else f"Lin{-s}E"      # noqa: E731
    for scheme in (1, 3, -3, 5, -5, 7):
        for fast in (0, 1):
            for w32 in ((0, 1) if scheme in (3, 5, 7) else (0,)):
                for ntr in (1, 2, 4):
                    tag = f"k_tracer_tendenciesI{code(scheme)}Lb{fast}ELb{w32}ELi{ntr}EE"
                    assert sum(tag in n for n in stencil) == 1, tag
    assert sum("k_tracer_star_noadv" in n for n in names) == 1 and sum("k_tracer_finish" in n for n in names) == 1
    for n, v in r.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vspill"] == 0 and v["sspill"] == 0, n
        # a block of 512 threads has 256 registers per thread, half of them vector registers proper: nothing in the accumulation registers
        assert v["agprs"] == 0 and v["vgprs"] <= 128, n
        # the flux tiles: 2 x NTR x 8 x 65 doubles
        if "k_tracer_tendencies" in n:
            ntr = int(re.search(r"Li(\d)EEEv", n).group(1))
            assert v["lds"] == 2 * ntr * 8 * 65 * 8, n
