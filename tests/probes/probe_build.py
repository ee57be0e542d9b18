"""Build of tests/probes/lf_math_probe.hip: hipcc with the CXXFLAGS of lisflood-code_amd/Makefile (so the inlined helpers
compute the bits they compute in the product's kernels), into a directory the caller owns."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "lisflood-code_amd")
PROBE = os.path.join(ROOT, "tests", "probes", "lf_math_probe.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BUILD_TIMEOUT_S = 600


def makefile_cxxflags():
    """CXXFLAGS of the product's Makefile with $(ARCH) expanded to its default."""
    text = open(os.path.join(PKG, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)\s*$", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*=\s*(.+?)\s*$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and any(f.startswith("--offload-arch=") for f in flags)
    return flags


def build(outdir):
    """Compile the probe into outdir/liblf_math_probe.so; returns its path."""
    so = os.path.join(outdir, "liblf_math_probe.so")
    cmd = ["timeout", "-k", "10", str(BUILD_TIMEOUT_S), HIPCC, *makefile_cxxflags(), "-shared",
           "-I", os.path.join(PKG, "csrc"), "-x", "hip", PROBE, "-o", so]
    subprocess.run(cmd, check=True)
    return so


def load(so):
    """ctypes handle with the argument types of the four entry points."""
    lib = C.CDLL(so)
    d, i, ll, u8 = C.POINTER(C.c_double), C.c_int, C.c_longlong, C.POINTER(C.c_ubyte)
    lib.probe_pow_beta.argtypes = [i, i, i, ll, d, d]
    lib.probe_solve.argtypes = [i, i, C.c_double, ll, d, d, d]
    lib.probe_pow_pos.argtypes = [i, i, ll, d, d, d]
    lib.probe_unsat_k.argtypes = [i, i, ll, d, u8, d, d, d, d, d, d]
    for f in (lib.probe_pow_beta, lib.probe_solve, lib.probe_pow_pos, lib.probe_unsat_k):
        f.restype = i
    return lib
