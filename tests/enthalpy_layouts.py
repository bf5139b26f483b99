"""The rule that chooses the form of the enthalpy-method column model's step kernel, stated ONCE in Python from include/csi.h
(csi_enthalpy_plan): tests/test_enthalpy_ref.py pins the library to it, tests/test_gpu_enthalpy.py takes its sizes from it."""
PER_STEP, ON_CHIP = 1, 2
LDS_PER_CU = 160 * 1024          # bytes
MIN_WAVES_PER_CU = 2             # the smallest residency taken
MAX_SUBSTEPS = 64                # sub-steps of one on-chip launch


class Unsupported(ValueError):
    pass


def lds_bytes(Nz):
    """H[1 .. Nz] and T[0 .. Nz + 1] of 64 columns, 8 bytes each."""
    return (2 * Nz + 2) * 512


def plan(Nz, forced=0):
    """dict(form, lds_bytes, waves_per_cu, max_substeps); forced: CSI_ENTH_PATH (0 auto, 1 per step, 2 on chip)."""
    if Nz < 1 or forced not in (0, 1, 2):
        raise ValueError("Nz >= 1 and a forced path of 0, 1 or 2")
    waves = LDS_PER_CU // lds_bytes(Nz)
    chip = waves >= MIN_WAVES_PER_CU
    if forced == 1:
        chip = False
    if forced == 2:
        if waves < 1:
            raise Unsupported("the column does not fit on chip")
        chip = True
    if chip:
        return dict(form=ON_CHIP, lds_bytes=lds_bytes(Nz), waves_per_cu=waves, max_substeps=MAX_SUBSTEPS)
    return dict(form=PER_STEP, lds_bytes=0, waves_per_cu=0, max_substeps=1)


LARGEST_ON_CHIP_NZ = max(n for n in range(1, 400) if plan(n)["form"] == ON_CHIP)      # 79
LARGEST_FORCED_NZ = max(n for n in range(1, 400) if LDS_PER_CU // lds_bytes(n) >= 1)   # 159


def launches(form_plan, n):
    """(launches, sub-steps of the first launch) of n steps."""
    cap = form_plan["max_substeps"]
    return -(-n // cap), min(n, cap)
