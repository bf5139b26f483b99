"""The pure-host launch helpers of csrc/csi_ctx.h (the advection scheme table, the copy batch's add, the row clip of a sub-step's ranges)
in a program of their own, tests/launch_helpers_host.cpp: built with the library's compiler and warning flags and the HOST address and
undefined-behaviour sanitizers, run once.  It makes no HIP call and needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_host_helpers_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "launch_helpers_host")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
                           "-Wno-bitwise-instead-of-logical", "-Wno-unused-value", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "climaseaice.jl_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "launch_helpers_host.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().splitlines() == ["ok"]
