"""Generated code of the enthalpy-method column model's kernels (csrc/enthalpy.hip; hipcc cross-compiles, nothing runs): from the
compiler's resource-usage remarks the build keeps beside the object (csrc/enthalpy.res) -- no scratch and no spills in any
instantiation, no static LDS (the on-chip form's image is dynamic: (2 Nz + 2) * 512 bytes per block of one wave), and the register
occupancy include/csi.h states: 8 waves per SIMD for every kernel, so that on chip the LDS image alone sets the residency."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaseaice.jl_amd", "csrc")


def remarks():
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC], stdout=subprocess.DEVNULL)      # (no-op when the library is up to date)
    blocks = open(os.path.join(CSRC, "enthalpy.res")).read().split("remark: Function Name: ")[1:]
    out = {}
    for b in blocks:
        g = lambda k: int(re.search(k + r"[^:]*: (\d+)", b).group(1))      # noqa: E731
        out[b.split()[0]] = dict(vgprs=g(r"    VGPRs"), scratch=g("ScratchSize"), vspill=g("VGPRs Spill"), sspill=g("SGPRs Spill"),
                                 lds=g("LDS Size"), occupancy=g("Occupancy"))
    return out


def test_six_instantiations_without_scratch_or_spills_at_full_register_occupancy():
    r = remarks()
    names = sorted(r)
    assert len(names) == 6, names
    assert sum("k_enthalpy_stepsILb1" in n for n in names) == 1 and sum("k_enthalpy_stepsILb0" in n for n in names) == 1      # on chip, per step
    assert sum("k_enthalpy_stateILi" in n for n in names) == 3 and sum("k_enthalpy_thickness" in n for n in names) == 1
    for n, v in r.items():
        print(n, v)
        assert v["scratch"] == 0 and v["vspill"] == 0 and v["sspill"] == 0 and v["lds"] == 0, n
        assert v["occupancy"] == 8 and v["vgprs"] <= 64, n


def test_header_states_that_occupancy_and_the_on_chip_residency():
    text = open(os.path.join(ROOT, "include", "csi.h"), encoding="utf-8").read()
    assert "register count allows 8 waves per SIMD for every kernel of the unit" in text
    assert "waves per CU as above (Nz = 20: 7)" in text
    import enthalpy_layouts as lay
    assert lay.plan(20)["waves_per_cu"] == 7 and lay.plan(lay.LARGEST_ON_CHIP_NZ)["waves_per_cu"] == 2
