"""The case matrix of the two-sub-steps kernel (csrc/evp_fused2.hip, k_pair) and the rule that selects its instantiations, stated once.

k_pair is compiled in 264 instantiations: eleven families (translation units v0 .. v10), three coefficient kinds (uniform, per-row,
per-point), three compile-time forcing kinds (CF), the order of the first sub-step (AUF), the peer-flag protocol (PEER) and neighbours
with other row strides (DLD).  The launch code picks one from the model's configuration alone (forcing_scratch and the loop of
run_fused in csi_launch.hip choose the arguments, launch_fused_pair in evp_fused2.hip dispatches on them); expected_key() below is a
pure-Python mirror of that rule over the keywords of cases.make_case, and MATRIX crosses the ingredients that drive it:

    family ingredients   none | walls (topology) | land | field_forcing | free_drift | user_forcing / immersed_bc |
                         wind_drag = "arrays" / bottom = "arrays", each with and without land
    coefficient kind     rectilinear f-plane (uniform) | beta = / grid = "latlon" (per-row) | curvilinear = (per-point)
    forcing kind         (plain, walls, mask only)  default (CF2) | ue = 0.05, ve = -0.02 (CF1) | pressure = "ice_strength" (CF0)

Every case keeps the Coriolis force and seeded velocity noise of at least 0.03 (without them a case can be blind to the order of
the sub-steps: ice_strength_nocoriolis of tests/test_gpu_pair_ufirst.py).  Untiled cases are 40 .. 72 columns wide -- at the small
grids' six rows per tile every one of them has row-chunk seams, and all but the 40- and 48-column ones two strips --, one more case per
family is 120 columns wide (three 56-column strips).  peer_case() / dld_case() widen a case to what the tiled transports need.

No GPU import: tests/test_pair_matrix_table.py checks the table on the CPU, tests/test_gpu_pair_matrix.py runs it,
scripts/order_sensitivity.py shows that its cases can tell a wrong kernel from a right one, scripts/pair_instantiation_coverage.py
compares what the rule expects with what a kernel trace of the tests shows.
"""

FAMILIES = ("plain", "walls", "mask", "force", "mask_force", "force_fd", "mask_force_fd", "force_x", "mask_force_x", "force_w", "mask_force_w")
TRANSPORTS = ("untiled", "self_peer", "bounded_x_group")
IBC = ((0.02, -0.01, 0.015, 0.005), (-0.01, 0.02, 0.01, -0.015))


class NotPaired(ValueError):
    """the configuration is one the two-sub-steps kernel does not take (pair_forcing_kind < 0): three kernels"""


def expected_key(kw, transport="untiled", first=1):
    """The spill-table key ("v4 UNI0 AUF1 CF0 FULL1 PEER0 X0 DLD0") of the instantiation a sub-cycle that starts on sub-step `first`
    launches for make_case(**kw) on `transport`: "untiled", "self_peer" (a tile connected to itself on the peer transport) or
    "bounded_x_group" (peer-connected tiles of a Bounded x direction: unequal row strides)."""
    assert transport in TRANSPORTS, transport
    topo = kw.get("topo", ("periodic", "periodic"))
    grid = kw.get("grid", "rectilinear")
    if "folded" in topo or grid == "tripolar":
        raise NotPaired("north fold: the pair kernel runs below a three-kernel band; not a case of this matrix")
    mask = bool(kw.get("land"))
    wind = kw.get("wind_drag") == "arrays"                       # a SemiImplicitStress on top with array-valued air velocities
    b_tau = kw.get("bottom", "semi") == "arrays"                 # an explicit bottom stress given as arrays
    fd = bool(kw.get("free_drift"))
    extra = bool(kw.get("user_forcing")) or (bool(kw.get("immersed_bc")) and mask)      # csi_core.hip evp_dev: P.extra
    if (extra and fd) or ((wind or b_tau) and (fd or extra)):
        raise NotPaired("no instantiation with both")            # evp_fused.hip pair_forcing_kind
    force = bool(kw.get("field_forcing")) or wind or b_tau or fd or extra               # evp_array_forcing
    x = 1 if extra else (2 if (wind or b_tau) else 0)            # forcing_scratch: extra_kind
    # the kernels' compile-time forcing kinds: no array forcing, a number-valued top stress (or none), a bottom SemiImplicitStress with
    # number-valued ocean velocities, ReplacementPressure; 2 when that ocean is at rest
    cf = 0
    if not force and kw.get("wind_drag") is None and kw.get("bottom", "semi") == "semi" and kw.get("pressure", "replacement") == "replacement":
        cf = 2 if (kw.get("ue", 0.0) == 0.0 and kw.get("ve", 0.0) == 0.0) else 1
    full = kw.get("curvilinear") is not None                     # CSI_METRIC_FULL
    uni = not full and grid == "rectilinear" and kw.get("beta") is None
    dld = transport == "bounded_x_group"
    walls = "bounded" in topo or mask or force or dld or full    # run_fused: walls_variant; launch_fused_pair: per-point -> walls
    if x == 2:
        v = 10 if mask else 9
    elif x == 1:
        v = 8 if mask else 7
    elif fd:
        v = 6 if mask else 5
    elif force:
        v = 4 if mask else 3
    elif mask:
        v = 2
    else:
        v = 1 if walls else 0
    if full and cf == 1:
        cf = 0                                                   # per-point coefficients: CF2 or the run-time kinds only
    if v > 2:
        cf = 0                                                   # the array-forcing families have one instantiation
    return (f"v{v} UNI{int(uni)} AUF{int(first % 2 == 0)} CF{cf} FULL{int(full)} PEER{int(transport != 'untiled')} X{x} "
            f"DLD{int(dld)}")


# ---- the matrix -------------------------------------------------------------------------------------------------------------------
_PP, _PB, _BB = ("periodic", "periodic"), ("periodic", "bounded"), ("bounded", "bounded")
_FAMILY_KW = {
    # family: (ingredients, topology on uniform / per-row / per-point coefficients)
    "plain": (dict(), (_PP, _PP, None)),                                   # (per-point coefficients: the walls variant)
    "walls": (dict(), (_PB, _BB, _BB)),
    "mask": (dict(land=0.25), (_PP, _PB, _PB)),
    "force": (dict(field_forcing=True), (_PP, _BB, _PP)),
    "mask_force": (dict(field_forcing=True, land=0.25), (_PB, _PP, _BB)),
    "force_fd": (dict(free_drift=True, ue=0.05, ve=-0.02, top=(0.03, -0.02)), (_PP, _PB, _PB)),
    "mask_force_fd": (dict(free_drift=True, field_forcing=True, land=0.25), (_PB, _BB, _PP)),
    "force_x": (dict(user_forcing=True), (_PP, _PP, _BB)),
    "mask_force_x": (dict(land=0.25, immersed_bc=IBC, user_forcing=True), (_PB, _BB, _PP)),
    "force_w": (dict(wind_drag="arrays"), (_PP, _PB, _BB)),
    "mask_force_w": (dict(bottom="arrays", land=0.2), (_PB, _PP, _PB)),
}
# the array ingredient of the wind / bottom-stress families alternates over the coefficient kinds, and so does immersed_bc alone
_VARIED = {("force_w", "row"): dict(bottom="arrays"), ("mask_force_w", "row"): dict(wind_drag="arrays", field_forcing=True, land=0.2),
           ("mask_force_w", "pt"): dict(wind_drag="arrays", land=0.2), ("mask_force_x", "row"): dict(land=0.25, immersed_bc=IBC)}
_CF_KW = {"cf2": dict(), "cf1": dict(ue=0.05, ve=-0.02), "cf0": dict(pressure="ice_strength")}
_SIZES = ((64, 48), (40, 56), (72, 40), (56, 44), (48, 52), (60, 36))


def _coef_kw(coef, topo, i):
    if coef == "uni":
        return dict()
    if coef == "row":            # a lat-lon grid needs a bounded y direction; BetaPlane elsewhere and on every other bounded one
        return dict(grid="latlon") if (topo[1] == "bounded" and i % 2 == 0) else dict(beta=2e-10 if i % 4 < 2 else -1.5e-10)
    return dict(grid="latlon", curvilinear=0.04) if (topo == _BB and i % 2 == 0) else dict(curvilinear=0.05)


def _build():
    matrix, combos, i = {}, {}, 0
    for family in FAMILIES:
        ingredients, topos = _FAMILY_KW[family]
        for ci, coef in enumerate(("uni", "row", "pt")):
            topo = topos[ci]
            if topo is None:
                continue
            for cf in (("cf2", "cf1", "cf0") if family in ("plain", "walls", "mask") else (None,)):
                kw = dict(_VARIED.get((family, coef), ingredients))
                kw.update(_coef_kw(coef, topo, i))
                if cf:
                    kw.update(_CF_KW[cf])
                nx, ny = _SIZES[i % len(_SIZES)]
                kw.update(Nx=nx, Ny=ny, topo=topo, patches=True, random_uv=0.03 + 0.01 * (i % 3))
                name = "_".join(x for x in (family, coef, cf) if x)
                matrix[name] = kw
                combos[name] = (family, coef, cf)
                i += 1
        # one multi-strip case per family: three 56-column strips, the coefficient kind rotating over the families
        coef = ("row", "pt", "uni")[FAMILIES.index(family) % 3]
        if family == "plain" and coef == "pt":
            coef = "row"
        topo = topos[("uni", "row", "pt").index(coef)]
        kw = dict(_VARIED.get((family, coef), ingredients))
        kw.update(_coef_kw(coef, topo, i))
        kw.update(Nx=120, Ny=38, topo=topo, patches=True, random_uv=0.04)
        matrix[f"{family}_{coef}_seams"] = kw
        i += 1
    return matrix, combos


MATRIX, COMBOS = _build()          # COMBOS: name -> (family, coefficient kind, forcing kind) of the cases the tiled tests widen


def peer_case(name):
    """(make_case keywords, connected directions) of MATRIX[name] on one tile connected to itself: 128 .. 160 columns (the peer
    transport's minimum is 128), 48 .. 96 rows, connected in x and, where y is periodic, in y"""
    kw = dict(MATRIX[name])
    i = sorted(COMBOS).index(name)
    kw.update(Nx=(128, 136, 144, 160)[i % 4], Ny=(48, 64, 80, 96)[(i // 4) % 4], topo=("periodic", kw["topo"][1]))
    return kw, (True, kw["topo"][1] == "periodic")


def dld_case(name):
    """make_case keywords of MATRIX[name] on a Bounded x direction cut into two 128-column tiles (the eastern tile's Face fields are one
    column wider: unequal row strides); None for the plain family, which has no walls"""
    family = COMBOS[name][0]
    if family == "plain":
        return None
    kw = dict(MATRIX[name])
    i = sorted(COMBOS).index(name)
    kw.update(Nx=256, Ny=(48, 64, 80, 96)[i % 4], topo=("bounded", kw["topo"][1]))
    return kw


def selected():
    """{key: [(case, transport, first sub-step)]}: what the rule selects over MATRIX x transports x first in {1, 2}, on the shapes the
    GPU tests run"""
    out = {}
    for name, kw in MATRIX.items():
        runs = [("untiled", kw)]
        if name in COMBOS:
            runs.append(("self_peer", peer_case(name)[0]))
            if dld_case(name) is not None:
                runs.append(("bounded_x_group", dld_case(name)))
        for transport, k in runs:
            for first in (1, 2):
                out.setdefault(expected_key(k, transport, first), []).append((name, transport, first))
    return out


def ingredient_removed(kw):
    """(what, keywords): the case without the ingredient that tells its instantiation from its neighbours' -- free drift off, model.forcing
    / immersed fluxes off, arrays -> numbers, ice_strength -> replacement, ocean velocity -> 0; for the default forcing kinds the
    land, the coefficients' variation, and last the number-valued top stress itself.  Array shapes stay as they are."""
    kw = dict(kw)
    if kw.get("free_drift"):
        kw["free_drift"] = False
        return "free drift off", kw
    if kw.get("user_forcing") or kw.get("immersed_bc"):
        kw["user_forcing"], kw["immersed_bc"] = False, None
        return "model.forcing / immersed fluxes off", kw
    if kw.get("wind_drag") == "arrays":
        kw["wind_drag"] = "numbers"
        return "air velocities: arrays -> numbers", kw
    if kw.get("bottom") == "arrays":
        kw["bottom"] = "semi"
        return "bottom stress arrays -> SemiImplicitStress", kw
    if kw.get("field_forcing"):
        kw["field_forcing"] = False
        return "stress / ocean-velocity arrays -> numbers", kw
    if kw.get("pressure", "replacement") != "replacement":
        kw["pressure"] = "replacement"
        return "ice_strength -> replacement", kw
    if kw.get("ue") or kw.get("ve"):
        kw["ue"], kw["ve"] = 0.0, 0.0
        return "ocean velocity -> 0", kw
    if kw.get("land"):
        kw["land"] = 0.0
        return "land off", kw
    if kw.get("beta") is not None:
        kw["beta"] = None
        return "BetaPlane -> FPlane", kw
    if kw.get("curvilinear") is not None:
        kw["curvilinear"] = 0.0
        return "distortion of the metrics off", kw
    if kw.get("grid") == "latlon":
        kw["grid"] = "rectilinear"
        return "lat-lon -> rectilinear", kw
    kw["top"] = None
    return "top stress off", kw


# The library refuses these on tiles, by name (csi.CsiError); tests/test_gpu_pair_matrix.py asserts each refusal.  No PEER0 key may
# appear here: every untiled target is reachable.
UNREACHABLE = {}

# ---- the 186 instantiations no GPU test had executed before this matrix (profiles/r11_pair_coverage.md, "Never executed") -----------
TARGETS = (
    "v0 UNI0 AUF0 CF0 FULL0 PEER0 X0 DLD0", "v0 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD0", "v0 UNI0 AUF0 CF1 FULL0 PEER0 X0 DLD0",
    "v0 UNI0 AUF0 CF1 FULL0 PEER1 X0 DLD0", "v0 UNI0 AUF1 CF0 FULL0 PEER0 X0 DLD0", "v0 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD0",
    "v0 UNI0 AUF1 CF1 FULL0 PEER0 X0 DLD0", "v0 UNI0 AUF1 CF1 FULL0 PEER1 X0 DLD0", "v0 UNI0 AUF1 CF2 FULL0 PEER1 X0 DLD0",
    "v0 UNI1 AUF0 CF0 FULL0 PEER1 X0 DLD0", "v0 UNI1 AUF0 CF1 FULL0 PEER1 X0 DLD0", "v0 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD0",
    "v0 UNI1 AUF1 CF1 FULL0 PEER0 X0 DLD0", "v0 UNI1 AUF1 CF1 FULL0 PEER1 X0 DLD0", "v1 UNI0 AUF0 CF0 FULL0 PEER0 X0 DLD0",
    "v1 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD0", "v1 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD1", "v1 UNI0 AUF0 CF0 FULL1 PEER0 X0 DLD0",
    "v1 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD0", "v1 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD1", "v1 UNI0 AUF0 CF1 FULL0 PEER0 X0 DLD0",
    "v1 UNI0 AUF0 CF1 FULL0 PEER1 X0 DLD0", "v1 UNI0 AUF0 CF1 FULL0 PEER1 X0 DLD1", "v1 UNI0 AUF0 CF2 FULL0 PEER1 X0 DLD1",
    "v1 UNI0 AUF0 CF2 FULL1 PEER1 X0 DLD1", "v1 UNI0 AUF1 CF0 FULL0 PEER0 X0 DLD0", "v1 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD0",
    "v1 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD1", "v1 UNI0 AUF1 CF0 FULL1 PEER0 X0 DLD0", "v1 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD0",
    "v1 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD1", "v1 UNI0 AUF1 CF1 FULL0 PEER0 X0 DLD0", "v1 UNI0 AUF1 CF1 FULL0 PEER1 X0 DLD0",
    "v1 UNI0 AUF1 CF1 FULL0 PEER1 X0 DLD1", "v1 UNI0 AUF1 CF2 FULL0 PEER1 X0 DLD1", "v1 UNI0 AUF1 CF2 FULL1 PEER1 X0 DLD1",
    "v1 UNI1 AUF0 CF0 FULL0 PEER1 X0 DLD0", "v1 UNI1 AUF0 CF0 FULL0 PEER1 X0 DLD1", "v1 UNI1 AUF0 CF1 FULL0 PEER0 X0 DLD0",
    "v1 UNI1 AUF0 CF1 FULL0 PEER1 X0 DLD0", "v1 UNI1 AUF0 CF1 FULL0 PEER1 X0 DLD1", "v1 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD0",
    "v1 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD1", "v1 UNI1 AUF1 CF1 FULL0 PEER0 X0 DLD0", "v1 UNI1 AUF1 CF1 FULL0 PEER1 X0 DLD0",
    "v1 UNI1 AUF1 CF1 FULL0 PEER1 X0 DLD1", "v1 UNI1 AUF1 CF2 FULL0 PEER1 X0 DLD1", "v2 UNI0 AUF0 CF0 FULL0 PEER0 X0 DLD0",
    "v2 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD0", "v2 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD1", "v2 UNI0 AUF0 CF0 FULL1 PEER0 X0 DLD0",
    "v2 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD0", "v2 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD1", "v2 UNI0 AUF0 CF1 FULL0 PEER0 X0 DLD0",
    "v2 UNI0 AUF0 CF1 FULL0 PEER1 X0 DLD0", "v2 UNI0 AUF0 CF1 FULL0 PEER1 X0 DLD1", "v2 UNI0 AUF0 CF2 FULL0 PEER1 X0 DLD0",
    "v2 UNI0 AUF0 CF2 FULL0 PEER1 X0 DLD1", "v2 UNI0 AUF0 CF2 FULL1 PEER1 X0 DLD0", "v2 UNI0 AUF0 CF2 FULL1 PEER1 X0 DLD1",
    "v2 UNI0 AUF1 CF0 FULL0 PEER0 X0 DLD0", "v2 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD0", "v2 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD1",
    "v2 UNI0 AUF1 CF0 FULL1 PEER0 X0 DLD0", "v2 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD0", "v2 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD1",
    "v2 UNI0 AUF1 CF1 FULL0 PEER0 X0 DLD0", "v2 UNI0 AUF1 CF1 FULL0 PEER1 X0 DLD0", "v2 UNI0 AUF1 CF1 FULL0 PEER1 X0 DLD1",
    "v2 UNI0 AUF1 CF2 FULL0 PEER1 X0 DLD0", "v2 UNI0 AUF1 CF2 FULL0 PEER1 X0 DLD1", "v2 UNI0 AUF1 CF2 FULL1 PEER1 X0 DLD0",
    "v2 UNI0 AUF1 CF2 FULL1 PEER1 X0 DLD1", "v2 UNI1 AUF0 CF0 FULL0 PEER1 X0 DLD0", "v2 UNI1 AUF0 CF0 FULL0 PEER1 X0 DLD1",
    "v2 UNI1 AUF0 CF1 FULL0 PEER0 X0 DLD0", "v2 UNI1 AUF0 CF1 FULL0 PEER1 X0 DLD0", "v2 UNI1 AUF0 CF1 FULL0 PEER1 X0 DLD1",
    "v2 UNI1 AUF0 CF2 FULL0 PEER1 X0 DLD1", "v2 UNI1 AUF1 CF0 FULL0 PEER0 X0 DLD0", "v2 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD0",
    "v2 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD1", "v2 UNI1 AUF1 CF1 FULL0 PEER0 X0 DLD0", "v2 UNI1 AUF1 CF1 FULL0 PEER1 X0 DLD0",
    "v2 UNI1 AUF1 CF1 FULL0 PEER1 X0 DLD1", "v2 UNI1 AUF1 CF2 FULL0 PEER1 X0 DLD1", "v3 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD0",
    "v3 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD1", "v3 UNI0 AUF0 CF0 FULL1 PEER0 X0 DLD0", "v3 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD0",
    "v3 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD1", "v3 UNI0 AUF1 CF0 FULL0 PEER0 X0 DLD0", "v3 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD0",
    "v3 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD1", "v3 UNI0 AUF1 CF0 FULL1 PEER0 X0 DLD0", "v3 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD0",
    "v3 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD1", "v3 UNI1 AUF0 CF0 FULL0 PEER1 X0 DLD1", "v3 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD1",
    "v4 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD0", "v4 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD1", "v4 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD1",
    "v4 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD0", "v4 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD1", "v4 UNI0 AUF1 CF0 FULL1 PEER0 X0 DLD0",
    "v4 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD0", "v4 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD1", "v4 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD0",
    "v4 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD1", "v5 UNI0 AUF0 CF0 FULL0 PEER0 X0 DLD0", "v5 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD0",
    "v5 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD1", "v5 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD0", "v5 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD1",
    "v5 UNI0 AUF1 CF0 FULL0 PEER0 X0 DLD0", "v5 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD0", "v5 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD1",
    "v5 UNI0 AUF1 CF0 FULL1 PEER0 X0 DLD0", "v5 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD0", "v5 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD1",
    "v5 UNI1 AUF0 CF0 FULL0 PEER1 X0 DLD0", "v5 UNI1 AUF0 CF0 FULL0 PEER1 X0 DLD1", "v5 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD0",
    "v5 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD1", "v6 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD0", "v6 UNI0 AUF0 CF0 FULL0 PEER1 X0 DLD1",
    "v6 UNI0 AUF0 CF0 FULL1 PEER1 X0 DLD1", "v6 UNI0 AUF1 CF0 FULL0 PEER0 X0 DLD0", "v6 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD0",
    "v6 UNI0 AUF1 CF0 FULL0 PEER1 X0 DLD1", "v6 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD0", "v6 UNI0 AUF1 CF0 FULL1 PEER1 X0 DLD1",
    "v6 UNI1 AUF0 CF0 FULL0 PEER1 X0 DLD1", "v6 UNI1 AUF1 CF0 FULL0 PEER1 X0 DLD1", "v7 UNI0 AUF0 CF0 FULL0 PEER0 X1 DLD0",
    "v7 UNI0 AUF0 CF0 FULL0 PEER1 X1 DLD0", "v7 UNI0 AUF0 CF0 FULL0 PEER1 X1 DLD1", "v7 UNI0 AUF0 CF0 FULL1 PEER1 X1 DLD0",
    "v7 UNI0 AUF0 CF0 FULL1 PEER1 X1 DLD1", "v7 UNI0 AUF1 CF0 FULL0 PEER1 X1 DLD0", "v7 UNI0 AUF1 CF0 FULL0 PEER1 X1 DLD1",
    "v7 UNI0 AUF1 CF0 FULL1 PEER0 X1 DLD0", "v7 UNI0 AUF1 CF0 FULL1 PEER1 X1 DLD0", "v7 UNI0 AUF1 CF0 FULL1 PEER1 X1 DLD1",
    "v7 UNI1 AUF0 CF0 FULL0 PEER1 X1 DLD0", "v7 UNI1 AUF0 CF0 FULL0 PEER1 X1 DLD1", "v7 UNI1 AUF1 CF0 FULL0 PEER1 X1 DLD0",
    "v7 UNI1 AUF1 CF0 FULL0 PEER1 X1 DLD1", "v8 UNI0 AUF0 CF0 FULL0 PEER1 X1 DLD0", "v8 UNI0 AUF0 CF0 FULL0 PEER1 X1 DLD1",
    "v8 UNI0 AUF0 CF0 FULL1 PEER1 X1 DLD0", "v8 UNI0 AUF0 CF0 FULL1 PEER1 X1 DLD1", "v8 UNI0 AUF1 CF0 FULL0 PEER1 X1 DLD0",
    "v8 UNI0 AUF1 CF0 FULL0 PEER1 X1 DLD1", "v8 UNI0 AUF1 CF0 FULL1 PEER1 X1 DLD0", "v8 UNI0 AUF1 CF0 FULL1 PEER1 X1 DLD1",
    "v8 UNI1 AUF0 CF0 FULL0 PEER1 X1 DLD0", "v8 UNI1 AUF0 CF0 FULL0 PEER1 X1 DLD1", "v8 UNI1 AUF1 CF0 FULL0 PEER1 X1 DLD0",
    "v8 UNI1 AUF1 CF0 FULL0 PEER1 X1 DLD1", "v9 UNI0 AUF0 CF0 FULL0 PEER0 X2 DLD0", "v9 UNI0 AUF0 CF0 FULL0 PEER1 X2 DLD0",
    "v9 UNI0 AUF0 CF0 FULL0 PEER1 X2 DLD1", "v9 UNI0 AUF0 CF0 FULL1 PEER0 X2 DLD0", "v9 UNI0 AUF0 CF0 FULL1 PEER1 X2 DLD0",
    "v9 UNI0 AUF0 CF0 FULL1 PEER1 X2 DLD1", "v9 UNI0 AUF1 CF0 FULL0 PEER1 X2 DLD0", "v9 UNI0 AUF1 CF0 FULL0 PEER1 X2 DLD1",
    "v9 UNI0 AUF1 CF0 FULL1 PEER0 X2 DLD0", "v9 UNI0 AUF1 CF0 FULL1 PEER1 X2 DLD0", "v9 UNI0 AUF1 CF0 FULL1 PEER1 X2 DLD1",
    "v9 UNI1 AUF0 CF0 FULL0 PEER1 X2 DLD1", "v9 UNI1 AUF1 CF0 FULL0 PEER1 X2 DLD1", "v10 UNI0 AUF0 CF0 FULL0 PEER0 X2 DLD0",
    "v10 UNI0 AUF0 CF0 FULL0 PEER1 X2 DLD0", "v10 UNI0 AUF0 CF0 FULL0 PEER1 X2 DLD1", "v10 UNI0 AUF0 CF0 FULL1 PEER1 X2 DLD0",
    "v10 UNI0 AUF0 CF0 FULL1 PEER1 X2 DLD1", "v10 UNI0 AUF1 CF0 FULL0 PEER1 X2 DLD0", "v10 UNI0 AUF1 CF0 FULL0 PEER1 X2 DLD1",
    "v10 UNI0 AUF1 CF0 FULL1 PEER0 X2 DLD0", "v10 UNI0 AUF1 CF0 FULL1 PEER1 X2 DLD0", "v10 UNI0 AUF1 CF0 FULL1 PEER1 X2 DLD1",
    "v10 UNI1 AUF0 CF0 FULL0 PEER1 X2 DLD1", "v10 UNI1 AUF1 CF0 FULL0 PEER1 X2 DLD0", "v10 UNI1 AUF1 CF0 FULL0 PEER1 X2 DLD1",
)
