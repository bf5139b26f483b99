"""Generated code of the time-series interpolation kernel (csrc/time_series.hip; hipcc cross-compiles, nothing runs): 16-byte accesses on
the aligned path, every load of a thread issued before the first wait, no scratch, no LDS, no contraction of the two products and
the sum."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    path = tmp_path_factory.mktemp("isa") / "time_series.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-ffp-contract=off",
                        "--cuda-device-only", "-S", os.path.join(ROOT, "climaseaice.jl_amd", "csrc", "time_series.hip"), "-o", str(path),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(path).read().split("\n")
    start = next(k for k, ln in enumerate(lines) if re.match(r"^_ZN3csi13k_time_series\S*:", ln))
    end = next(k for k in range(start, len(lines)) if lines[k].strip().startswith(".Lfunc_end"))
    return [ln.strip() for ln in lines[start:end]], r.stderr


def test_aligned_path_uses_16_byte_accesses_and_no_load_follows_a_wait(kernel_asm):
    body, _ = kernel_asm
    loads = [k for k, t in enumerate(body) if t.startswith(("global_load", "buffer_load", "flat_load"))]
    waits = [k for k, t in enumerate(body) if t.startswith("s_waitcnt") and "vmcnt" in t]
    assert sum(body[k].startswith("global_load_dwordx4") for k in loads) == 4       # psi_1 and psi_2 of two rows
    assert sum(t.startswith("global_store_dwordx4") for t in body) == 2
    assert loads and waits and max(loads) < min(waits), "a load is issued behind a wait: the operand pairs are not all in flight together"


def test_no_scratch_no_lds_full_occupancy_and_no_fused_multiply_add(kernel_asm):
    body, remarks = kernel_asm
    get = lambda key: int(re.search(key + r"[^:]*:\s*(\d+)", remarks).group(1))
    assert get("ScratchSize") == 0 and get("VGPRs Spill") == 0 and get("SGPRs Spill") == 0 and get("LDS Size") == 0
    assert get(r"Occupancy \[waves/SIMD\]") == 8
    assert not any(t.startswith(("scratch_", "ds_")) for t in body)
    assert not any(t.startswith(("v_fma_f64", "v_fmac_f64", "v_pk_fma")) for t in body)
    assert sum(t.startswith("v_mul_f64") for t in body) == 8 and sum(t.startswith("v_add_f64") for t in body) == 4      # 2 rows x 2 points
