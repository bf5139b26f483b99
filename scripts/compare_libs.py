"""Bitwise comparison of two builds of the library: the named cases of tests/test_gpu_evp.py (every fusion level, FAST mode) and one
case per host path -- whole FE / RK3 steps, the one-launch RK stages, thermodynamics + mixed layer + tracers, ViscousRheology, the
ExplicitSolver, free-drift dynamics, the in-place fallback of run_fused, STRICT, the fold band in both forms, a 1 x 4 in-process tile
group on both halo transports -- each at the small shape its own test module uses.  Whole parents (interior and halos) of every field
and the last-path record of every case:
python scripts/compare_libs.py dump <out.npz> [substeps]     (run once per build, CSI_HIP_LIBRARY selects it; the tile group needs
                                                              4 < GPU_MAX_HW_QUEUES <= 32 in the environment)
python scripts/compare_libs.py diff <a.npz> <b.npz>"""
import os
import sys
sys.path[:0] = [".", "tests", "oracle"]
import numpy as np
if sys.argv[1] == "diff":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = {"arrays": 0, "records": 0}
    count = {"arrays": 0, "records": 0}
    for k in sorted(set(a.files) | set(b.files)):
        kind = "records" if k.endswith("/record") else "arrays"
        count[kind] += 1
        if k not in a.files or k not in b.files:
            bad[kind] += 1
            print("MISSING", k, "in", sys.argv[2] if k not in a.files else sys.argv[3])
        elif a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            bad[kind] += 1
            if kind == "records" or a[k].shape != b[k].shape:
                print("DIFF", k, a[k].tolist() if kind == "records" else a[k].shape, b[k].tolist() if kind == "records" else b[k].shape)
            else:
                d = np.abs(a[k] - b[k])
                print("DIFF", k, "max", np.nanmax(d), "count", int((d > 0).sum()), "of", d.size)
    print("arrays", count["arrays"], "different", bad["arrays"], "; records", count["records"], "different", bad["records"])
    sys.exit(1 if bad["arrays"] or bad["records"] else 0)
import cases
import climaseaice_jl_amd as csi
from test_gpu_evp import CASES, EVP_FIELDS
nsub = int(sys.argv[3]) if len(sys.argv) > 3 else 24
out = {}


def dump(tag, m):
    """whole parents of u, v, the stresses, the diagnostics, h, aice [, hs, the tracers, the mixed layer's temperature] and the record"""
    m.synchronize()
    fields = {"h": m.ice_thickness, "aice": m.ice_concentration, "hs": getattr(m, "snow_thickness", None)}
    for k in ("u", "v", "s11", "s22", "s12", "alpha", "zeta_c", "zeta_f", "Delta"):
        try:
            fields[k] = EVP_FIELDS[k](m)
        except AttributeError:      # (a dynamics without the EVP auxiliaries)
            pass
    fields.update({f"tracer_{k}": f for k, f in getattr(m, "tracers", {}).items()})
    if getattr(m, "ocean", None) is not None:
        fields["To"] = m.ocean.temperature
    for k, f in fields.items():
        if f is not None:
            out[f"{tag}/{k}"] = f.numpy().copy()
    p, ctx = m.ctx.last_path(), m.ctx
    rec = [p["level"], p["exchange_interval"], p["exchanges"], *ctx.last_launches(), ctx.launches_per_substep(), ctx.halo_transport() == "peer"]
    out[f"{tag}/record"] = np.array(rec, dtype=np.int64)
    print(tag, rec, flush=True)


# ---- the EVP momentum cases, every fusion level
for name in sorted(CASES):
    c = cases.make_case(substeps=nsub, **CASES[name])
    for fusion in (0, 2):
        try:
            m = cases.csi_model(c, mode="fast")
        except Exception as e:
            print("skip", name, e); break
        m.set_fusion(fusion)
        for _ in range(2):
            csi.time_step_momentum(m, c["dt"])
        dump(f"{name}/{fusion}", m)

# ---- whole FE / RK3 steps with dynamics (tests/test_gpu_steps.py)
from test_gpu_steps import STEP_CASES
for name in ("periodic", "masked"):
    c = cases.make_case(substeps=12, **STEP_CASES[name])
    for stepper in ("ForwardEuler", "SplitRungeKutta3"):
        for mode in ("strict", "fast"):
            m = cases.csi_model(c, mode=mode, timestepper=stepper, advection=csi.WENO(order=7))
            for _ in range(2):
                csi.time_step(m, c["dt"])
            dump(f"step_{name}/{stepper}/{mode}", m)

# ---- an RK3 step of an advection-only model: one launch per stage (and, fusion 0, the general stage loop)
c = cases.make_case(Nx=100, Ny=72, H=4, topo=("periodic", "bounded"), patches=True, random_uv=0.3)
for fusion in (0, 2):
    for adv, scheme in (("WENO7", csi.WENO(order=7)), ("Upwind3", csi.UpwindBiased(order=3))):
        m = csi.SeaIceModel(c["g"], dynamics=None, advection=scheme, timestepper="SplitRungeKutta3", mode="fast")
        m.set_fusion(fusion)
        csi.set_(m, h=c["h"], aice=c["a"], u=c["u"], v=c["v"])
        for _ in range(4):
            csi.time_step(m, 300.0)
        dump(f"advection_only/{adv}/{fusion}", m)
        out[f"advection_only/{adv}/{fusion}/hm"] = m.timestepper.Psi_minus.h.numpy().copy()
        out[f"advection_only/{adv}/{fusion}/stage_fused"] = np.array([m.ctx.last_advection()["stage_fused"]])

# ---- slab thermodynamics + mixed layer + two advected tracers (tests/test_gpu_mixed_layer.py's whole-step case)
c = cases.make_case(Nx=37, Ny=29, substeps=8, topo=("periodic", "bounded"), patches=True, random_uv=0.02)
rng = np.random.default_rng(71)
for stepper in ("ForwardEuler", "SplitRungeKutta3"):
    ice = csi.SlabThermodynamics(bottom_salinity=30.0, top_heat_boundary_condition=csi.MeltingConstrainedFluxBalance())
    specs = [csi.Tracer("plain", weighting=None, nonnegative=True, source=0.0), csi.Tracer("age", weighting="concentration", nonnegative=True, source=1.0)]
    m = cases.csi_model(c, mode="fast", timestepper=stepper, advection=csi.WENO(order=7), ice_thermodynamics=ice, top_heat_flux=-40.0,
                        ocean=csi.SlabOceanMixedLayer(30.0, temperature=-1.5 + 0.5 * rng.random((29, 37))), tracers=specs)
    csi.set_(m, plain=0.1 + rng.random((29, 37)), age=0.1 + rng.random((29, 37)))
    for _ in range(2):
        csi.time_step(m, c["dt"])
    dump(f"thermo_ml_tracers/{stepper}", m)

# ---- ViscousRheology split-explicit (even / odd sub-step counts), the ExplicitSolver with both rheologies (tests/test_gpu_momentum_variants.py)
from test_gpu_momentum_variants import model_of as variant_model, CASES as VARIANTS, NU
for name, kw in (VARIANTS[0], VARIANTS[2], VARIANTS[8]):
    for substeps in (4, 5):
        for mode in ("strict", "fast"):
            c = cases.make_case(substeps=substeps, **kw)
            m = variant_model(c, rheology=csi.ViscousRheology(nu=NU), solver=csi.SplitExplicitSolver(substeps=substeps), mode=mode)
            csi.time_step_momentum(m, c["dt"])
            dump(f"viscous_split/{name}/{substeps}/{mode}", m)
    for rheo in ("evp", "viscous"):
        for stepper in ("ForwardEuler", "SplitRungeKutta3"):
            c = cases.make_case(substeps=3, **kw)
            m = variant_model(c, rheology=csi.ViscousRheology(nu=NU) if rheo == "viscous" else None, solver=csi.ExplicitSolver(), mode="fast",
                              timestepper=stepper, advection=csi.WENO(order=5))
            for _ in range(2):
                csi.time_step(m, 60.0)
            dump(f"explicit/{name}/{rheo}/{stepper}", m)

# ---- StressBalanceFreeDrift as the dynamics (tests/test_gpu_free_drift.py)
from test_gpu_free_drift import model_of as free_drift_model, _dyn_case
for name in ("periodic_numbers", "masked_channel_arrays", "folded_arrays"):
    c = _dyn_case(name)
    m = free_drift_model(c, as_dynamics=True, mode="fast")
    csi.time_step_momentum(m, c["dt"])
    dump(f"free_drift_dynamics/{name}/momentum", m)
c = _dyn_case("masked_channel_arrays", Nx=24, Ny=20)
for stepper in ("ForwardEuler", "SplitRungeKutta3"):
    m = free_drift_model(c, as_dynamics=True, mode="fast", timestepper=stepper, advection=csi.WENO(order=5))
    for _ in range(2):
        csi.time_step(m, 60.0)
    dump(f"free_drift_dynamics/masked_channel_arrays/{stepper}", m)

# ---- masked, halo 3, FAST, fusion 2: no pair kernel.  (do_subcycle then declines the fused paths altogether and the unfused loop runs, level 0:
# the in-place three-kernel branch inside run_fused is not reached from any entry point, profiles/r31_host_launch_refactor.md)
for nsteps in (7, 8):
    c = cases.make_case(Nx=67, Ny=45, H=3, topo=("periodic", "bounded"), land=0.25, patches=True, random_uv=0.05, substeps=nsteps)
    m = cases.csi_model(c, mode="fast")
    m.set_fusion(2)
    for _ in range(2):
        csi.time_step_momentum(m, c["dt"])
    dump(f"masked_halo3_fallback/{nsteps}", m)

# ---- STRICT at fusion 0: one periodic and one walled case
for name in ("periodic_patches", "bounded"):
    c = cases.make_case(substeps=9, **CASES[name])
    m = cases.csi_model(c, mode="strict")
    m.set_fusion(0)
    for _ in range(2):
        csi.time_step_momentum(m, c["dt"])
    dump(f"strict/{name}", m)

# ---- a north fold with the band's fused launches (CSI_BAND_FUSED unset) and with the three kernels + copies (CSI_BAND_FUSED=0); the
# variable is read when the context is created
from test_gpu_activity import BAND_CASES
for name in ("rectilinear_odd", "latlon_masked_forced", "curvilinear"):
    for band in (None, "0"):
        os.environ.pop("CSI_BAND_FUSED", None)
        if band is not None:
            os.environ["CSI_BAND_FUSED"] = band
        c = cases.make_case(**BAND_CASES[name])
        m = cases.csi_model(c, mode="fast")
        for _ in range(2):
            csi.time_step_momentum(m, c["dt"])
        dump(f"fold_band/{name}/{'fused' if band is None else 'three_kernels'}", m)
os.environ.pop("CSI_BAND_FUSED", None)

# ---- a 1 x 4 in-process tile group (tests/test_gpu_local_tiles.py): the message exchange with interval 2 at fusion 0 and 2, the peer transport
from test_gpu_local_tiles import run_tile_threads, DECOMPOSITIONS
for name in ("1x4_periodic_y", "1x4_fold_tripolar"):
    Rx, Ry, kw, _ = DECOMPOSITIONS[name]
    c = cases.make_case(H=8, substeps=14, patches=True, random_uv=0.05, **kw)
    for what, k, fusion in (("exchange_k2_fusion0", 2, 0), ("exchange_k2_fusion2", 2, 2), ("peer", 0, 2)):
        def tile(rank, group):
            m = cases.csi_model(c, mode="fast", timestepper="SplitRungeKutta3", advection=csi.WENO(order=7), tile=(Rx, Ry, rank), local_group=group)
            m.set_exchange_interval(k)
            m.set_fusion(fusion)
            csi.time_step_momentum(m, c["dt"])
            csi.time_step_momentum(m, c["dt"])
            dump(f"tiles/{name}/{what}/rank{rank}/momentum", m)
            csi.time_step(m, c["dt"])
            dump(f"tiles/{name}/{what}/rank{rank}/step", m)
            del m
        run_tile_threads(Rx * Ry, tile)

np.savez(sys.argv[2], **out)
print("saved", len(out))
