"""CPU-only checks of the ensemble through the sub-step loop (lf_routing_substeps_fused_members / routingEnsemble): the two
symbols are exported with the header's argument kinds, argument errors come back with a message before a device is needed,
the slice arithmetic of the member form holds at its edges, and the Python layers refuse malformed input before they reach
the library."""
import ctypes as C
import types

import numpy as np
import pytest

from lisflood_amd import _lib
from lisflood_amd.kinematic_wave_parallel import kinematicWave
from lisflood_amd.routing import _SubstepArgs, routingEnsemble


def last_error():
    return _lib.lib().lf_last_error().decode()


def test_member_entry_points_are_exported_with_the_headers_kinds():
    L = _lib.lib()
    f = L.lf_routing_substeps_fused_members
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64]   # p p i q i q q
    s = L.lf_fused_members_slice
    assert s.restype is C.c_int64
    assert list(s.argtypes) == [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int]
    for args in ((None, None, 9, 0.0, 2, 8, 8), (None, None, 9, 0, 2, 8.0, 8), (None, None, 9, 0, 2, 8, 8.0)):
        with pytest.raises(C.ArgumentError):
            f(*args)                                                      # a float for an int64_t
    with pytest.raises(C.ArgumentError):
        s(2, 8.0, 9, 1, 1 << 20, 0)


def test_member_argument_errors_come_back_without_a_device():
    """member-count and stride errors first, then null arguments: none of them needs a router, so none can have asked for a
    device.  (A stride between 0 and N needs a router to know N: tests/test_substep_members_gpu.py has that refusal.)"""
    L = _lib.lib()
    a = _SubstepArgs()
    a.engine_order = 1
    f = L.lf_routing_substeps_fused_members
    assert f(None, C.byref(a), 9, 0, 2, 8, 8) == _lib.LF_E_INVALID
    assert "null argument" in last_error()
    for members in (0, -3):
        assert f(None, C.byref(a), 9, 0, members, 8, 8) == _lib.LF_E_INVALID
        assert "members must be at least 1" in last_error()
        assert f(None, None, 9, 0, members, -1, -1) == _lib.LF_E_INVALID          # the member count comes first
        assert "members must be at least 1" in last_error()
    assert f(None, C.byref(a), 9, 0, 2, -1, 8) == _lib.LF_E_INVALID
    assert "member_stride -1 is less than the router's number of cells" in last_error()
    assert f(None, None, 9, 0, 2, -1, -1) == _lib.LF_E_INVALID                     # ... then the member stride
    assert "member_stride -1 is less than" in last_error()
    assert f(None, C.byref(a), 9, 0, 2, 8, -5) == _lib.LF_E_INVALID
    assert "sideflow_member_stride -5" in last_error()


def slice_by_formula(members, n, nsteps, split, budget, cap):
    """the largest s <= min(members, 65535, cap if cap > 0) with s * nsteps * n * 8 * (2 if split else 1) <= budget"""
    per = nsteps * n * 8 * (2 if split else 1)
    top = min(members, 65535, cap) if cap > 0 else min(members, 65535)
    return min(top, budget // per)


def test_members_slice_at_its_edges():
    S = _lib.lib().lf_fused_members_slice
    n, nsteps = 25600, 24
    one = nsteps * n * 8
    # one byte short of one member: the member form does not apply
    assert S(5, n, nsteps, 0, one - 1, 0) == 0 == slice_by_formula(5, n, nsteps, False, one - 1, 0)
    assert S(5, n, nsteps, 0, one, 0) == 1
    # exactly k members, and one byte less
    for k in (2, 3, 4):
        assert S(5, n, nsteps, 0, k * one, 0) == k == slice_by_formula(5, n, nsteps, False, k * one, 0)
        assert S(5, n, nsteps, 0, k * one - 1, 0) == k - 1 == slice_by_formula(5, n, nsteps, False, k * one - 1, 0)
    # room for more than there are members
    assert S(5, n, nsteps, 0, 100 * one, 0) == 5
    # blockIdx.y: at most 65 535 members per slice
    assert S(70000, 10, 2, 0, 1 << 40, 0) == 65535 == slice_by_formula(70000, 10, 2, False, 1 << 40, 0)
    assert S(65535, 10, 2, 0, 1 << 40, 0) == 65535 and S(65534, 10, 2, 0, 1 << 40, 0) == 65534
    # the cap of LF_FUSED_MEMBERS_SLICE
    assert S(5, n, nsteps, 0, 100 * one, 2) == 2 == slice_by_formula(5, n, nsteps, False, 100 * one, 2)
    assert S(5, n, nsteps, 0, 100 * one, 9) == 5 and S(5, n, nsteps, 0, one, 2) == 1
    # split routing keeps two histories
    assert S(5, n, nsteps, 1, 4 * one, 0) == 2 == slice_by_formula(5, n, nsteps, True, 4 * one, 0)
    assert S(5, n, nsteps, 1, 4 * one - 1, 0) == 1 and S(5, n, nsteps, 1, 2 * one - 1, 0) == 0
    # one member
    assert S(1, n, nsteps, 0, one, 0) == 1 and S(1, n, nsteps, 0, one - 1, 0) == 0 and S(1, n, nsteps, 1, 2 * one, 7) == 1
    # sizes beyond 2^63 bytes per member do not wrap
    assert S(3, 1 << 50, 1 << 20, 1, (1 << 63) - 1, 0) == 0
    # nothing to run
    assert S(0, n, nsteps, 0, one, 0) == 0 and S(-2, n, nsteps, 0, one, 0) == 0


def unbuilt_router(n):
    """a kinematicWave without its constructor (which needs a device): what the wrapper checks before the library"""
    kw = kinematicWave.__new__(kinematicWave)
    kw.num_pixels = n
    kw._h = None
    return kw


@pytest.mark.parametrize("bad", [dict(members=0), dict(members=-2), dict(nsteps=0), dict(sideflow_stride=3)])
def test_wrapper_refuses_malformed_counts_before_the_library(bad):
    kw = unbuilt_router(6)
    call = dict(args=_SubstepArgs(), nsteps=9, members=2)
    call.update(bad)
    with pytest.raises(ValueError, match="members must be at least 1|nsteps must be at least 1|sideflow_stride must be 0 or 6"):
        kw.routing_substeps_members(**call)


def unbuilt_ensemble(members, n, nsteps):
    """a routingEnsemble without its constructor (which allocates on a device): what it checks before the device"""
    e = routingEnsemble.__new__(routingEnsemble)
    e.members, e.N, e.stride, e.nsteps, e.perm = members, n, n, nsteps, np.arange(n)
    e.vectors = e.router = e._side = None
    return e


def test_ensemble_refuses_no_member_before_it_touches_the_router():
    for members in (0, -1):
        with pytest.raises(ValueError, match="members must be at least 1"):
            routingEnsemble(types.SimpleNamespace(), None, members)


@pytest.mark.parametrize("case", ["float32", "one_dimensional", "wrong_width", "wrong_members", "a_list", "no_such_vector"])
def test_ensemble_refuses_malformed_state(case):
    M, N = 3, 6
    name = "Discharge" if case == "no_such_vector" else "ChanQKin"
    host = {"float32": np.zeros((M, N), np.float32), "one_dimensional": np.zeros(M * N), "wrong_width": np.zeros((M, N + 1)),
            "wrong_members": np.zeros((M + 1, N)), "a_list": [[0.0] * N] * M, "no_such_vector": np.zeros((M, N))}[case]
    want = "no state or output vector" if case == "no_such_vector" else r"float64 \[3, 6\] array"
    with pytest.raises(ValueError, match=want):
        unbuilt_ensemble(M, N, 4).set_state(name, host)
    if case == "no_such_vector":
        with pytest.raises(ValueError, match=want):
            unbuilt_ensemble(M, N, 4).state(name)


@pytest.mark.parametrize("shape", [(7,), (2, 6), (3, 5), (3, 3, 6), (4, 6), (3, 4, 5), (1, 3, 4, 6)])
def test_ensemble_refuses_malformed_sideflows(shape):
    e = unbuilt_ensemble(3, 6, 4)
    with pytest.raises(ValueError, match=r"shaped \[6\], \[3, 6\] or \[3, 4, 6\]"):
        e.dynamic_fused(np.zeros(shape))
    with pytest.raises(ValueError, match="float64"):
        e.dynamic_fused(np.zeros((3, 6), np.float32))


def test_ensemble_sideflow_strides():
    e = unbuilt_ensemble(3, 6, 4)
    assert e._sideflow_rows(np.zeros(6))[1:] == (0, 0)                  # one vector for every member and sub-step
    assert e._sideflow_rows(np.zeros((3, 6)))[1:] == (0, 6)
    assert e._sideflow_rows(np.zeros((3, 4, 6)))[1:] == (6, 24)
