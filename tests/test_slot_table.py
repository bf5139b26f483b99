"""The field slots are stated once per language -- csrc/csi_slots.h, _lib.SLOTS, the Julia stub's named tuples -- on top of the enums
of include/csi.h.  These tests hold the four together: ids and names against what gcc makes of the header, every column of the C table
against the Python one, each role against the list of slots that had it before there was a table, the Julia constants against the
Python ids, and every name _lib derives from the table against the value it had when it was written out by hand."""
import os
import re
import subprocess

import pytest

import climaseaice_jl_amd as csi

L = csi._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "csi.h")
LOC = {csi.Center: 0, csi.Face: 1}      # csi_slots.h: LOC_C, LOC_F

# ---- typed in, not computed from either table ---------------------------------------------------------------------------------------
FIELD_IDS = ("U V H A S11 S22 S12 UN VN P ALPHA DELTA ZETA_F ZETA_C GH GA HM AM UM VM TOP_U TOP_V BOT_U BOT_V MASS_FLUX HS GHS HSM "
             "MASS_FLUX_SNOW SNOWFALL_INTERCEPTED TU TUS FORCING_U FORCING_V GU GV").split()
THERMO_FIELD_IDS = ["TOP_HEAT_FLUX", "BOTTOM_HEAT_FLUX", "SNOWFALL"]
FREE_DRIFT_FIELD_IDS = ["FREE_DRIFT_U", "FREE_DRIFT_V"]
DERIVED_FIELD_IDS = ["D_DIVERGENCE", "D_SHEAR", "D_DEFORMATION", "D_SPEED", "D_SIGMA_I", "D_SIGMA_II", "D_STRESS_POWER"]
MOMENTUM_TERM_FIELD_IDS = ["M_CORIOLIS_X", "M_CORIOLIS_Y", "M_TOP_X", "M_TOP_Y", "M_BOTTOM_X", "M_BOTTOM_Y", "M_INTERNAL_X", "M_INTERNAL_Y",
                           "M_FORCING_X", "M_FORCING_Y"]
THERMO_LINEAR_FIELD_IDS = ["FLUX_COEFFICIENT", "FLUX_REFERENCE_TEMPERATURE", "BOTTOM_SALINITY", "TOP_HEAT_FLUX_USED", "BOTTOM_HEAT_FLUX_USED"]
MIXED_LAYER_FIELD_IDS = ["ML_TEMPERATURE", "ML_TEMPERATURE_M", "ML_SURFACE_HEAT_FLUX", "ML_COEFFICIENT", "ML_REFERENCE_TEMPERATURE",
                         "ML_DEEP_HEAT_FLUX", "ML_SURFACE_FLUX_USED"]
SHORTWAVE_FIELD_IDS = ["SHORTWAVE", "ALBEDO_USED"]
FORCING = ["TOP_U", "TOP_V", "BOT_U", "BOT_V", "FORCING_U", "FORCING_V", "FREE_DRIFT_U", "FREE_DRIFT_V"]      # kForcingFields' order
ROLE_MEMBERS = {
    "SLOT_HALO": FIELD_IDS + FREE_DRIFT_FIELD_IDS,                                                              # halo_slot()
    "SLOT_PEER": ["U", "V", "S11", "S22", "S12", "ALPHA", "ZETA_C", "ZETA_F", "DELTA"],                         # csi_field_bind's peer_field
    "SLOT_FORCING": FORCING,
    "SLOT_SERIES": FORCING + ["TOP_HEAT_FLUX", "BOTTOM_HEAT_FLUX", "SNOWFALL", "FLUX_COEFFICIENT", "FLUX_REFERENCE_TEMPERATURE",
                              "BOTTOM_SALINITY", "ML_SURFACE_HEAT_FLUX", "ML_COEFFICIENT", "ML_REFERENCE_TEMPERATURE",
                              "ML_DEEP_HEAT_FLUX", "SHORTWAVE"]}                                                 # series_slot()
# every name _lib derives from SLOTS, with the value it had as a literal
DERIVED_NAMES = dict(
    FIELD_IDS=FIELD_IDS, THERMO_FIELD_IDS=THERMO_FIELD_IDS, FREE_DRIFT_FIELD_IDS=FREE_DRIFT_FIELD_IDS, DERIVED_FIELD_IDS=DERIVED_FIELD_IDS,
    MOMENTUM_TERM_FIELD_IDS=MOMENTUM_TERM_FIELD_IDS, THERMO_LINEAR_FIELD_IDS=THERMO_LINEAR_FIELD_IDS,
    MIXED_LAYER_FIELD_IDS=MIXED_LAYER_FIELD_IDS, SHORTWAVE_FIELD_IDS=SHORTWAVE_FIELD_IDS,
    F=dict(zip(FIELD_IDS + THERMO_FIELD_IDS + FREE_DRIFT_FIELD_IDS, range(0, 41))), F_DERIVED=dict(zip(DERIVED_FIELD_IDS, range(41, 48))),
    F_MOMENTUM_TERMS=dict(zip(MOMENTUM_TERM_FIELD_IDS, range(48, 58))), F_THERMO_LINEAR=dict(zip(THERMO_LINEAR_FIELD_IDS, range(58, 63))),
    F_MIXED_LAYER=dict(zip(MIXED_LAYER_FIELD_IDS, range(63, 70))), F_SHORTWAVE=dict(zip(SHORTWAVE_FIELD_IDS, range(70, 72))),
    F_COUNT_BINDABLE=58, F_COUNT_THERMO=63, F_COUNT_MIXED_LAYER=70, F_COUNT_SHORTWAVE=72,
    SERIES_SLOTS=FORCING + ["TOP_HEAT_FLUX", "BOTTOM_HEAT_FLUX", "SNOWFALL"],
    THERMO_SERIES_SLOTS=["FLUX_COEFFICIENT", "FLUX_REFERENCE_TEMPERATURE", "BOTTOM_SALINITY"],
    MIXED_LAYER_SERIES_SLOTS=["ML_SURFACE_HEAT_FLUX", "ML_COEFFICIENT", "ML_REFERENCE_TEMPERATURE", "ML_DEEP_HEAT_FLUX"],
    SHORTWAVE_SERIES_SLOTS=["SHORTWAVE"])


def _run(tmp_path, compiler, source, *flags):
    exe = str(tmp_path / "a.out")
    subprocess.check_call([compiler, *flags, "-I", os.path.join(ROOT, "include"), source, "-o", exe])
    return subprocess.check_output([exe]).decode().splitlines()


def test_header_enumerators_are_the_python_rows(tmp_path):
    """Every CSI_F_* enumerator of the header, with the value gcc gives it: the ones that are not counts are ids 0 .. 71, once each, and
    _lib.SLOTS names them in that order.  The names come from the header text, so a new enumerator joins by itself."""
    text = open(HEADER).read()
    names = sorted(set(re.findall(r"^\s+(CSI_F_[A-Z0-9_]+)(?:\s*=\s*[A-Z0-9_]+)?,?\s*(?:/\*.*)?$", text, re.M)))
    assert "CSI_F_U" in names and "CSI_F_ALBEDO_USED" in names and "CSI_F_COUNT_SHORTWAVE" in names
    src = tmp_path / "enums.c"
    src.write_text('#include <stdio.h>\n#include "csi.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %d\\n", (int){n});\n' for n in names) + "    return 0;\n}\n")
    values = {n: int(v) for n, v in (line.split() for line in _run(tmp_path, "gcc", str(src)))}
    slots = sorted((v, n[len("CSI_F_"):]) for n, v in values.items() if not n.startswith("CSI_F_COUNT"))
    assert [v for v, _ in slots] == list(range(72))
    assert [n for _, n in slots] == [row[0] for row in L.SLOTS]
    assert max(v for n, v in values.items() if n.startswith("CSI_F_COUNT")) == len(L.SLOTS) == 72


def test_c_table_equals_the_python_table(tmp_path):
    out = _run(tmp_path, "g++", os.path.join(ROOT, "tests", "slots_host.cpp"), "-std=c++17", "-Wall", "-Werror")
    rows, tail = out[:-3], out[-3:]
    assert tail[0] == f"roles {L.SLOT_HALO} {L.SLOT_PEER} {L.SLOT_FORCING} {L.SLOT_SERIES}"
    assert tail[1].split() == ["forcing"] + [str(L.slot_id(n)) for n in FORCING]      # iteration over a role: table order
    assert tail[2] == "known 0 0"
    assert rows == [f"{k} {display} {LOC[lx]} {LOC[ly]} {roles}" for k, (_, display, (lx, ly), roles) in enumerate(L.SLOTS)]
    assert len(rows) == 72


@pytest.mark.parametrize("role", sorted(ROLE_MEMBERS))
def test_role_members_are_what_the_code_spelled_out(role):
    bit = getattr(L, role)
    members = [name for name, _, _, roles in L.SLOTS if roles & bit]
    assert sorted(members) == sorted(ROLE_MEMBERS[role]) and len(members) == {"SLOT_HALO": 38, "SLOT_PEER": 9, "SLOT_FORCING": 8, "SLOT_SERIES": 19}[role]
    if role == "SLOT_FORCING":
        assert members == FORCING
    assert all(roles < 16 for _, _, _, roles in L.SLOTS)


def test_julia_constants_agree_with_the_python_rows():
    """The six named tuples of the Julia stub: every entry's number is the id of a row whose NAME or display name it spells (in any
    letter case), and together they cover the 72 ids once each."""
    text = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "ClimaSeaIceHIP.jl")).read())      # (without the comments)
    seen = {}
    for tup in ("F", "DERIVED", "MOMENTUM_TERMS", "THERMO_LINEAR", "MIXED_LAYER", "SHORTWAVE"):
        body = re.search(rf"^const {tup} = \((.*?)\)\s*$", text, re.M | re.S).group(1)
        entries = re.findall(r"(\w+)\s*=\s*(\d+)", body)
        assert entries, tup
        for name, value in entries:
            assert int(value) not in seen, (tup, name)
            seen[int(value)] = name
    assert sorted(seen) == list(range(72))
    for k, name in seen.items():
        assert name.lower() in (L.SLOTS[k][0].lower(), L.SLOTS[k][1].lower()), (k, name, L.SLOTS[k][:2])


@pytest.mark.parametrize("name", sorted(DERIVED_NAMES))
def test_derived_names_keep_their_values(name):
    got, want = getattr(L, name), DERIVED_NAMES[name]
    assert type(got) is type(want) and got == want
    if isinstance(want, dict):
        assert list(got.items()) == list(want.items())


def test_lookups():
    assert [L.slot_id(row[0]) for row in L.SLOTS] == list(range(72))
    assert L.slot_location("S12") == (csi.Face, csi.Face) and L.slot_location("M_TOP_Y") == (csi.Center, csi.Face)
    assert L.slot_of_display_name("ocean_coefficient") == "ML_COEFFICIENT" and L.slot_of_display_name("bottom_u") == "BOT_U"
    assert len({row[1] for row in L.SLOTS}) == 72
    with pytest.raises(KeyError):
        L.slot_id("NOPE")
