"""Which of the 864 instantiations of the flux-term kernels (csrc/thermo_flux.hip: k_slab_flux, k_layered_flux) a test run executes.

    python scripts/thermo_flux_coverage.py OUT.json                       # the three thermodynamic GPU files of before the matrix
    python scripts/thermo_flux_coverage.py OUT.json tests/test_gpu_thermo_flux_matrix.py ...      # any other selection

Runs pytest on the files in this process with a wrapper around Context.call: after every call that steps the thermodynamics
(csi_slab_thermo_step, csi_layered_thermo_step, csi_time_step_fe, csi_time_step_rk3) it asks csi_last_thermo which kernel the library
launched and notes the key (step, shortwave, index).  The wrapper lives here, not in a conftest.py: the tests run as they are.  The set
of keys goes to OUT.json with the count out of 864 and, per key, the flags tests/thermo_flux_matrix.flags_of decodes.

A measurement, not a gate: no test reads its result."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
BEFORE = ["tests/test_gpu_heat_fluxes.py", "tests/test_gpu_thermo_linear.py", "tests/test_gpu_thermo_shortwave.py"]
STEPPING = {"csi_slab_thermo_step", "csi_layered_thermo_step", "csi_time_step_fe", "csi_time_step_rk3"}


def main(argv):
    if not argv:
        print(__doc__)
        return 2
    out, files = argv[0], (argv[1:] or BEFORE)
    import pytest
    import climaseaice_jl_amd as csi
    import thermo_flux_matrix as M
    seen = {}
    call = csi._lib.Context.call

    def recording_call(self, name, *args):
        call(self, name, *args)
        if name in STEPPING:
            last = self.last_thermo()
            key = (last["step"], last["shortwave"], last["index"])
            seen[key] = seen.get(key, 0) + 1

    csi._lib.Context.call = recording_call
    try:
        rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider"] + [os.path.join(ROOT, f) for f in files])
    finally:
        csi._lib.Context.call = call
    flux = sorted(k for k in seen if k[0] in (M.K_SLAB_FLUX, M.K_LAYERED_FLUX))
    report = dict(files=files, pytest_exit=int(rc), instantiations=len(M.all_keys()), executed=len(flux),
                  numeric_steps={str(k[0]): n for k, n in seen.items() if k[0] in (M.K_SLAB, M.K_LAYERED)},
                  keys=[dict(step=k[0], shortwave=k[1], index=k[2], steps=seen[k], flags=M.flags_of(k[0], k[2])) for k in flux])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(report, f, indent=1)
    by = {}
    for k in flux:
        by[(k[0], k[1])] = by.get((k[0], k[1]), 0) + 1
    print(f"{len(flux)} of {len(M.all_keys())} flux-kernel instantiations executed by {', '.join(files)}")
    for (step, sw), n in sorted(by.items()):
        print(f"  {'k_slab_flux' if step == M.K_SLAB_FLUX else 'k_layered_flux'} shortwave {sw}: {n} of {M.TABLE[step]}")
    return int(rc)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
