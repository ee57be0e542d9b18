"""CPU-only checks of the ensemble entry points (one router, M members swept together): the two symbols are exported
with the header's argument kinds, argument errors are refused with a message before a device is needed, and the Python
wrapper refuses malformed arrays and section names before it reaches the library."""
import ctypes as C

import numpy as np
import pytest

from lisflood_amd import _lib
from lisflood_amd.kinematic_wave_parallel import kinematicWave


def last_error():
    return _lib.lib().lf_last_error().decode()


def test_member_entry_points_are_exported_with_the_headers_kinds():
    L = _lib.lib()
    f = L.lf_router_route_ordered_members
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]   # stride: q
    h = L.lf_router_route_members_host
    assert h.restype is C.c_int
    assert list(h.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    with pytest.raises(C.ArgumentError):
        f(None, None, None, 2, 7.0, 0)                                    # a float for the int64_t stride


def test_member_argument_errors_come_back_without_a_device():
    """null pointers, members = 0 and a negative stride are refused with LF_E_INVALID and a message; none of them needs a
    router, so none of them can have asked for a device.  Of `stride < N` only the negative strides are covered here:
    a stride between 0 and N needs a router to know N, and tests/test_members_gpu.py::test_edge_arguments has that
    refusal."""
    L = _lib.lib()
    buf = np.zeros(8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.lf_router_route_ordered_members(None, p, p, 2, 8, 0) == _lib.LF_E_INVALID
    assert "null argument" in last_error()
    assert L.lf_router_route_members_host(None, p, p, 2, 0) == _lib.LF_E_INVALID
    assert "null argument" in last_error()
    for members in (0, -3):
        assert L.lf_router_route_ordered_members(None, p, p, members, 8, 0) == _lib.LF_E_INVALID
        assert "members must be at least 1" in last_error()
        assert L.lf_router_route_members_host(None, p, p, members, 0) == _lib.LF_E_INVALID
        assert "members must be at least 1" in last_error()
    assert L.lf_router_route_ordered_members(None, p, p, 2, -1, 0) == _lib.LF_E_INVALID
    assert "stride -1 is less than the router's number of cells" in last_error()
    assert (buf == 0).all()


def unbuilt_router(n):
    """a kinematicWave without its constructor (which needs a device): what the wrapper checks before the library"""
    kw = kinematicWave.__new__(kinematicWave)
    kw.num_pixels = n
    kw.flagnancheck = False
    kw.kinematic_wave_warning_printed = False
    kw._h = None
    return kw


@pytest.mark.parametrize("case", ["non_contiguous", "float32", "one_dimensional", "wrong_width", "no_member"])
def test_ensemble_wrapper_refuses_malformed_discharge(case):
    N = 6
    discharge = {"non_contiguous": np.zeros((3, 2 * N))[:, ::2],
                 "float32": np.zeros((3, N), np.float32),
                 "one_dimensional": np.zeros(3 * N),
                 "wrong_width": np.zeros((3, N + 1)),
                 "no_member": np.zeros((0, N))}[case]
    with pytest.raises(ValueError, match=r"C-contiguous float64 \[members, 6\]"):
        unbuilt_router(N).kinematicWaveRoutingEnsemble(discharge, np.zeros(N))


def test_ensemble_wrapper_raises_the_references_section_text():
    kw = unbuilt_router(6)
    want = "The section parameter must be either 'main_channel' or 'floodplain'!"
    with pytest.raises(Exception) as e:
        kw.kinematicWaveRoutingEnsemble(np.zeros((2, 6)), 0.0, section="floodplain")
    assert type(e.value) is Exception and str(e.value) == want
    with pytest.raises(Exception) as e:
        kw.route_ordered_members(None, None, 2, section="overland")
    assert type(e.value) is Exception and str(e.value) == want
