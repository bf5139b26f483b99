"""The table of tests/pair_matrix.py, checked without a GPU: the mirror of the launch rule names only instantiations that exist, and
the matrix reaches every instantiation that no GPU test had executed before it (TARGETS) -- but for those the library refuses by name."""
import json
import os
import re

import pytest

import pair_matrix as pm

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spill_table.json")
KEY = re.compile(r"^v(\d+) UNI[01] AUF[01] CF[012] FULL[01] PEER[01] X[012] DLD[01]$")


selected_keys = pm.selected


def table_keys():
    with open(TABLE) as f:
        return set(json.load(f))


def test_every_expected_key_is_an_instantiation():
    table, selected = table_keys(), selected_keys()
    assert all(KEY.match(k) for k in selected), [k for k in selected if not KEY.match(k)]
    assert set(selected) <= table, sorted(set(selected) - table)


def test_targets_are_instantiations_and_written_out_once():
    table = table_keys()
    assert len(pm.TARGETS) == len(set(pm.TARGETS)) == 186
    assert set(pm.TARGETS) <= table
    assert sum(" PEER0 " in k for k in pm.TARGETS) == 37


def test_the_matrix_reaches_every_target():
    selected = set(selected_keys())
    missing = sorted(set(pm.TARGETS) - selected - set(pm.UNREACHABLE))
    assert not missing, missing
    # nothing is excused twice: a key the table does select is not listed as unreachable
    assert not set(pm.UNREACHABLE) & selected, sorted(set(pm.UNREACHABLE) & selected)


def test_unreachable_holds_tiled_keys_with_a_reason_only():
    for key, reason in pm.UNREACHABLE.items():
        assert key in pm.TARGETS and " PEER1 " in key, key            # every untiled target is reachable
        assert isinstance(reason, str) and reason.strip(), key


def test_every_family_coefficient_and_forcing_kind_is_crossed():
    """families x coefficient kinds (plain has no per-point instantiation), the three forcing kinds on plain, walls and mask, one
    multi-strip case per family; every case keeps the Coriolis force and seeded velocity noise"""
    for family in pm.FAMILIES:
        for coef in ("uni", "row", "pt"):
            if (family, coef) == ("plain", "pt"):
                continue
            cfs = ("cf2", "cf1", "cf0") if family in ("plain", "walls", "mask") else (None,)
            for cf in cfs:
                assert (family, coef, cf) in pm.COMBOS.values(), (family, coef, cf)
        assert any(n.startswith(family + "_") and n.endswith("_seams") and n[len(family) + 1:].split("_")[0] in ("uni", "row", "pt")
                   for n in pm.MATRIX), family
    for name, kw in pm.MATRIX.items():
        assert kw.get("coriolis", 1e-4) and kw["random_uv"] >= 0.03, name
        assert (40 <= kw["Nx"] <= 72) or name.endswith("_seams"), name
        fam = next(f for f in sorted(pm.FAMILIES, key=len, reverse=True) if name.startswith(f + "_"))
        v = int(KEY.match(pm.expected_key(kw)).group(1))
        # (plain on per-point coefficients does not exist: walls)
        assert pm.FAMILIES[v] == fam, (name, pm.expected_key(kw))


@pytest.mark.parametrize("kw", [dict(free_drift=True, user_forcing=True), dict(wind_drag="arrays", free_drift=True),
                                dict(bottom="arrays", user_forcing=True), dict(topo=("periodic", "folded"))])
def test_configurations_without_an_instantiation_are_named(kw):
    with pytest.raises(pm.NotPaired):
        pm.expected_key(kw)
