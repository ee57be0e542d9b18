"""The probe library of tests/test_device_math_gpu.py cross-compiles for gfx950 with the product's CXXFLAGS (no GPU)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "probes"))
import probe_build  # noqa: E402


def test_probe_builds_with_the_makefile_flags(tmp_path):
    flags = probe_build.makefile_cxxflags()
    assert "-O3" in flags and "--offload-arch=gfx950" in flags
    lib = probe_build.load(probe_build.build(str(tmp_path)))
    for name in ("probe_pow_beta", "probe_solve", "probe_pow_pos", "probe_unsat_k"):
        assert hasattr(lib, name), name
