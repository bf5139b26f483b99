"""The table of tests/momentum_variant_shapes.py, checked without a GPU: from the table alone, every configuration meets every shape,
halo pair, metric kind and topology, the masked and no-slip physics and the unequal halos reach a multi-block launch, and no case is
one the entry point refuses.  The shapes are checked against the launch geometry the kernels' source states."""
import os
import re

import pytest

import momentum_variant_shapes as mv

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "climaseaice.jl_amd", "csrc")


def test_shapes_straddle_the_launch_block_the_sources_state():
    for name, n in (("momentum_viscous.hip", 2), ("momentum_explicit.hip", 3)):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        assert text.count("const dim3 b(64, 4);") == n and "dim3 b(" not in text.replace("const dim3 b(64, 4);", ""), name
        assert text.count("grid_for(r, b)") == 2 * n + (2 if n == 3 else 0), name        # every launch sized from the range
    bx, by = mv.BLOCK
    assert (bx, by) == (64, 4)
    assert mv.SHAPES == [(bx - 1, by - 1), (bx, by), (bx + 1, by + 1), (2 * bx + 2, 2 * by + 1)]
    for Nx, Ny in mv.MULTI_BLOCK:
        assert Nx > bx and Ny > by and Nx % bx and Ny % by                                # a second block and a partial last one, both ways
    assert -(-130 // bx) == 3 and -(-9 // by) == 3
    with open(os.path.join(CSRC, "csi_launch.hip")) as f:
        text = f.read()
    assert re.search(r"if \(c->Hx < 2 \|\| c->Hy < 2\) return fail\(c, CSI_ERR_INVALID_ARGUMENT, \"the momentum step needs halo >= 2\"\);", text)
    assert min(min(h) for h in mv.HALOS) == 2


def test_physics_are_the_sets_of_the_existing_cases():
    import test_gpu_momentum_variants as variants          # (its module-level mark concerns its own tests; importing needs no GPU)
    geometry = ("Nx", "Ny", "topo", "grid", "curvilinear")
    assert len(variants.CASES) == len(mv.PHYSICS) == 9
    for (_, kw), (_, phys) in zip(variants.CASES, mv.PHYSICS):
        assert {k: v for k, v in kw.items() if k not in geometry} == phys
    assert mv.IBC == variants.IBC and mv.NU == variants.NU


def test_no_case_is_refused_and_names_are_unique():
    assert 56 <= len(mv.TABLE) <= 68
    assert len({c["name"] for c in mv.TABLE}) == len(mv.TABLE)
    for c in mv.TABLE:
        (Nx, Ny), (Hx, Hy), kw = c["shape"], c["halo"], c["kw"]
        assert Hx >= 2 and Hy >= 2 and Nx >= Hx and Ny >= Hy, c["name"]
        assert (kw["Nx"], kw["Ny"], tuple(kw["H"]), kw["topo"]) == (Nx, Ny, (Hx, Hy), c["topo"])
        assert c["shape"] in mv.SHAPES and c["halo"] in mv.HALOS and c["topo"] in mv.TOPOLOGIES and c["metric"] in mv.METRICS
        assert kw.get("grid", "rectilinear") == ("latlon" if c["metric"] == "latlon" else "rectilinear")
        assert (kw.get("curvilinear") == 0.15) == (c["metric"] == "curvilinear")
        if c["metric"] == "curvilinear":
            assert kw.get("coriolis_points") or kw["coriolis"] is None
        else:
            assert not kw.get("coriolis_points")             # (refused by the library without full 2-D metrics)
        if kw.get("noslip"):
            assert c["topo"] == ("bounded", "bounded")


@pytest.mark.parametrize("configuration", mv.CONFIGURATIONS)
def test_each_configuration_meets_every_geometry(configuration):
    table = mv.cases_for(configuration)
    for shape in mv.SHAPES:
        here = [c for c in table if c["shape"] == shape]
        assert here, shape
        assert {c["halo"] for c in here} == set(mv.halos_for(shape)), shape              # each halo pair with Hx <= Nx, Hy <= Ny
        assert {c["topo"] for c in here} == set(mv.TOPOLOGIES), shape
        assert {c["metric"] for c in here} == set(mv.METRICS), shape
    assert mv.halos_for((63, 3)) == [(2, 2), (5, 3)] and mv.halos_for((64, 4)) == [(2, 2), (4, 4), (5, 3)]       # Hy <= Ny
    assert all(mv.halos_for(s) == mv.HALOS for s in mv.MULTI_BLOCK)
    for what, values in (("halo", mv.HALOS), ("metric", list(mv.METRICS)), ("topo", mv.TOPOLOGIES), ("physics", [n for n, _ in mv.PHYSICS])):
        assert {c[what] for c in table} == set(values), what
    # every metric kind on every topology (nothing omitted), every halo pair on every topology
    assert {(c["metric"], c["topo"]) for c in table} == {(m, t) for m in mv.METRICS for t in mv.TOPOLOGIES}
    assert {(c["halo"], c["topo"]) for c in table} == {(h, t) for h in mv.HALOS for t in mv.TOPOLOGIES}
    # every physics set on every metric kind and on every topology, and at a multi-block shape
    names = [n for n, _ in mv.PHYSICS]
    assert {(c["physics"], c["metric"]) for c in table} == {(p, m) for p in names for m in mv.METRICS}
    assert {(c["physics"], c["topo"]) for c in table} == {(p, t) for p in names for t in mv.TOPOLOGIES}
    assert {c["physics"] for c in table if c["shape"] in mv.MULTI_BLOCK} == set(names)


@pytest.mark.parametrize("configuration", mv.CONFIGURATIONS)
def test_masks_walls_and_unequal_halos_reach_a_multi_block_launch(configuration):
    multi = [c for c in mv.cases_for(configuration) if c["shape"] in mv.MULTI_BLOCK]
    assert any(c["kw"].get("land") and c["kw"].get("immersed_bc") for c in multi)
    assert any(c["kw"].get("noslip") for c in multi)
    big = {c["halo"] for c in mv.cases_for(configuration) if c["shape"] == (130, 9)}
    assert (5, 3) in big and (3, 5) in big
    # ... and the minimum halo, where the unconditional "safe address" loads have the least room, under walls and under a mask
    assert any(c["halo"] == (2, 2) and c["topo"] == ("bounded", "bounded") for c in multi)
    assert any(c["halo"] == (2, 2) and c["kw"].get("land") for c in mv.cases_for(configuration))


def test_exact_cases():
    assert len(mv.EXACT_CASES) == 8 and mv.K_FAST == 4.0
    for name, kw in mv.EXACT_CASES:
        assert (kw["Nx"], kw["Ny"]) in mv.MULTI_BLOCK and not kw.get("free_drift") and not kw.get("field_forcing"), name
