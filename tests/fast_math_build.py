"""Builds the two test libraries of the FAST-arithmetic tests; test infrastructure.

  tests/libfast_math_probe.so  tests/fast_math_probe.hip through the `probe` target of csrc/Makefile (hipcc for gfx950, the flags of
                               evp_fast.o; cross-compiles without a GPU)
  tests/libfast_coef_host.so   tests/fast_coef_host.cpp (g++, host only): csrc/csi_fast_coef.h behind extern "C"
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaseaice.jl_amd", "csrc")
PROBE = os.path.join(ROOT, "tests", "libfast_math_probe.so")
COEF_SRC = os.path.join(ROOT, "tests", "fast_coef_host.cpp")
COEF = os.path.join(ROOT, "tests", "libfast_coef_host.so")


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(target) < os.path.getmtime(d) for d in deps)


def build_probe():
    subprocess.check_call(["make", "-s", "-C", CSRC, "probe"])      # make decides whether anything is stale
    return PROBE


def build_coef(force=False):
    if force or _stale(COEF, [COEF_SRC, os.path.join(CSRC, "csi_fast_coef.h")]):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-I" + CSRC, COEF_SRC, "-o", COEF])
    return COEF


def build():
    build_coef()
    return build_probe()


if __name__ == "__main__":
    print(build())
