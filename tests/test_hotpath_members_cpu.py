"""No GPU: the host side of the ensemble forms of the stages between the land surface and the channel loop --
lf_pixel_aggregates_members_device, lf_surface_step_members, lf_router_route_ordered_members_multi, lf_gather_rows_device
and lf_module_last_form.  The exports are in the header, the library and the ctypes table; every refusal comes back as
LF_E_INVALID with the argument named before a device is touched; a valid call then needs a device.  (A stride between 0 and
a router's N needs a router, which needs a device: tests/test_route_members_multi_gpu.py has that refusal.)  The order in
which the element-wise member kernels take their (pixel block, member) units is lf_module_members_unit -- the function the
kernels call -- and must be the land surface's (lf_land_members_unit): any bijection gives the same bits, only this one keeps
the members of a block on one XCD."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from lisflood_amd import _lib
from lisflood_amd.pixel_aggregates import _PixelArgs
from lisflood_amd.surface_routing import _SurfaceArgs

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
EXPORTS = {"lf_pixel_aggregates_members_device": "ipiqqq", "lf_surface_step_members": "ppppiqq",
           "lf_router_route_ordered_members_multi": "ipppiqi", "lf_gather_rows_device": "iqppqpqi",
           "lf_module_last_form": "ii", "lf_module_members_unit": "qiqpp"}
N = 600                            # 3 blocks of 256 pixels
FAKE = 64                          # a pointer that is never dereferenced: every call here ends before a device is touched
ROUTER = C.c_void_p(FAKE)          # ... and before a router is looked at


def last_error():
    return _lib.lib().lf_last_error()


def test_the_exports_are_in_the_header_the_library_and_the_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + name: sig for sig, names in _lib._SIGNATURES.items() for name in names.split()}
    L = _lib.lib()
    for name, sig in EXPORTS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert re.search(r"\sT\s+%s$" % name, dynamic, flags=re.M), name
        assert table[name] == sig, name
        assert list(getattr(L, name).argtypes) == [_lib._KIND[k] for k in sig] and getattr(L, name).restype is C.c_int


def pixel_block(n=N, report=True):
    """lf_pixel_args with every vector named (report=False: only what is always needed)"""
    a = _PixelArgs()
    for name, _ in _PixelArgs._fields_[:-3]:
        setattr(a, name, FAKE)
    if not report:
        for name in ("RainSnowmelt", "TaPixel", "TaCUM", "Ta", "Theta", "ThetaAll", "W1a", "W1b", "W2", "LZAvInflow", "LZInflowCUM"):
            setattr(a, name, None)
    a.InvDtDay, a.TimeSinceStart, a.N = 1.0, 1.0, n
    return a


def surface_block(n=N):
    a = _SurfaceArgs()
    for name, kind in _SurfaceArgs._fields_:
        if kind is C.c_void_p:
            setattr(a, name, FAKE)
    a.Beta, a.N = 0.6, n
    return a


def pixel_call(a, members, stride, pstride, fstride):
    return _lib.lib().lf_pixel_aggregates_members_device(0, C.byref(a), members, stride, pstride, fstride)


def surface_call(a, members, stride, pstride):
    return _lib.lib().lf_surface_step_members(ROUTER, ROUTER, ROUTER, C.byref(a), members, stride, pstride)


TOO_MANY = (2 ** 31) // 3 + 1      # members * 3 blocks is beyond the 32-bit range of a launch
REFUSED = {                        # members, member_stride, pixel_member_stride, forcing_member_stride, the word
    "members_0": (0, 3 * N, N, 0, b"members"),
    "members_negative": (-2, 3 * N, N, 0, b"members"),
    "member_stride_short": (2, 3 * N - 1, N, 0, b"member_stride"),
    "member_stride_0": (2, 0, N, 0, b"member_stride"),
    "pixel_stride_short": (2, 3 * N, N - 1, 0, b"pixel_member_stride"),
    "pixel_stride_negative": (2, 3 * N, -N, 0, b"pixel_member_stride"),
    "forcing_stride_1": (2, 3 * N, N, 1, b"forcing_member_stride"),
    "forcing_stride_short": (2, 3 * N, N, N - 1, b"forcing_member_stride"),
    "forcing_stride_negative": (2, 3 * N, N, -N, b"forcing_member_stride"),
    "units_beyond_32_bits": (TOO_MANY, 3 * N, N, 0, b"32-bit"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_member_arguments_are_refused_before_any_device(case):
    members, stride, pstride, fstride, word = REFUSED[case]
    for report in (True, False):
        assert pixel_call(pixel_block(report=report), members, stride, pstride, fstride) == _lib.LF_E_INVALID, case
        assert word in last_error() and b"pixel aggregates" in last_error(), (case, last_error())
    if not case.startswith("forcing"):                                   # (the surface step has no forcing of its own)
        assert surface_call(surface_block(), members, stride, pstride) == _lib.LF_E_INVALID, case
        assert word in last_error() and b"surface step" in last_error(), (case, last_error())


def test_the_checks_of_the_single_calls_are_inherited():
    L = _lib.lib()
    a = pixel_block()
    a.LZ = None                                                          # a vector that is always needed
    assert pixel_call(a, 2, 3 * N, N, 0) == _lib.LF_E_INVALID and b"required vector is NULL" in last_error()
    a = pixel_block()
    a.Ta = None                                                          # TaPixel is asked for, its input is not there
    assert pixel_call(a, 2, 3 * N, N, 0) == _lib.LF_E_INVALID and b"input vector is NULL" in last_error()
    assert L.lf_pixel_aggregates_members_device(0, None, 2, 3 * N, N, 0) == _lib.LF_E_INVALID
    s = surface_block()
    for routers in ((None, ROUTER, ROUTER), (ROUTER, None, ROUTER), (ROUTER, ROUTER, None)):
        assert L.lf_surface_step_members(*routers, C.byref(s), 2, 3 * N, N) == _lib.LF_E_INVALID and b"null argument" in last_error()
    assert L.lf_surface_step_members(ROUTER, ROUTER, ROUTER, None, 2, 3 * N, N) == _lib.LF_E_INVALID


def test_route_members_multi_checks_its_counts_before_it_looks_at_a_router():
    L = _lib.lib()
    three = (C.c_void_p * 3)(FAKE, FAKE, FAKE)
    call = lambda count, members, stride: L.lf_router_route_ordered_members_multi(count, three, three, three, members, stride, 0)
    for count in (0, -1, 5):
        assert call(count, 2, N) == _lib.LF_E_INVALID and b"count" in last_error(), count
    for members in (0, -3):
        assert call(3, members, N) == _lib.LF_E_INVALID and b"members must be at least 1" in last_error()
    assert call(3, 2, -1) == _lib.LF_E_INVALID and b"stride -1" in last_error()
    assert L.lf_router_route_ordered_members_multi(3, None, three, three, 2, N, 0) == _lib.LF_E_INVALID
    assert b"null argument" in last_error()
    holes = (C.c_void_p * 3)(FAKE, None, FAKE)
    for args in ((holes, three, three), (three, holes, three), (three, three, holes)):
        assert L.lf_router_route_ordered_members_multi(3, *args, 2, N, 0) == _lib.LF_E_INVALID and b"null argument" in last_error()


def test_gather_rows_and_the_form_query_refuse_bad_arguments():
    L = _lib.lib()
    p = C.c_void_p(FAKE)
    gather = lambda n, sstride, dstride, rows, idx=p, src=p, dst=p: L.lf_gather_rows_device(0, n, idx, src, sstride, dst, dstride, rows)
    for rows in (0, -1):
        assert gather(N, N, N, rows) == _lib.LF_E_INVALID and b"rows" in last_error()
    assert gather(N, N, N - 1, 2) == _lib.LF_E_INVALID and b"dst_stride" in last_error()
    assert gather(N, -1, N, 2) == _lib.LF_E_INVALID and b"src_stride" in last_error()
    assert gather(-1, N, N, 2) == _lib.LF_E_INVALID and b"n = -1" in last_error()
    assert gather(2 ** 31, 2 ** 31, 2 ** 31, 2) == _lib.LF_E_INVALID and b"32-bit" in last_error()
    for hole in ("idx", "src", "dst"):
        assert gather(N, N, N, 2, **{hole: None}) == _lib.LF_E_INVALID and b"null argument" in last_error()
    for stage in (-1, 2):
        assert L.lf_module_last_form(0, stage) == _lib.LF_E_INVALID and b"stage" in last_error()


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_a_valid_call_needs_a_device():
    L = _lib.lib()
    for report in (True, False):
        for members, stride, pstride, fstride in ((1, 3 * N, N, 0), (2, 3 * N, N, 0), (3, 3 * N + 5, N + 5, N + 7),
                                                  (TOO_MANY - 1, 3 * N, N, N)):
            assert pixel_call(pixel_block(report=report), members, stride, pstride, fstride) == _lib.LF_E_NO_DEVICE
    p = C.c_void_p(FAKE)
    assert L.lf_gather_rows_device(0, N, p, p, 0, p, N, 3) == _lib.LF_E_NO_DEVICE
    assert L.lf_gather_rows_device(0, 0, None, None, 0, None, 0, 1) == _lib.LF_E_NO_DEVICE
    assert L.lf_module_last_form(0, 0) == _lib.LF_E_NO_DEVICE and L.lf_module_last_form(0, 1) == _lib.LF_E_NO_DEVICE


def _units(fn, nblocks, members, positions):
    """-> [len(positions), 2]: (block, member) of the given launch positions by lf_land_members_unit / lf_module_members_unit"""
    block, member = C.c_int64(-1), C.c_int(-1)
    out = np.empty((len(positions), 2), np.int64)
    for i, p in enumerate(positions):
        assert fn(nblocks, members, int(p), C.byref(block), C.byref(member)) == _lib.LF_OK
        out[i] = block.value, member.value
    return out


@pytest.mark.parametrize("members", [1, 2, 3, 8, 17])
@pytest.mark.parametrize("nblocks", [1, 7, 8, 9, 12, 75, 1000])
def test_the_member_kernels_deal_their_units_as_the_land_surface_does(nblocks, members):
    L = _lib.lib()
    units = nblocks * members
    order = _units(L.lf_module_members_unit, nblocks, members, range(units))
    assert ((order[:, 0] >= 0) & (order[:, 0] < nblocks) & (order[:, 1] >= 0) & (order[:, 1] < members)).all()
    unit = order[:, 0] * members + order[:, 1]                          # block-major: u = block * members + m
    assert np.array_equal(np.sort(unit), np.arange(units))              # every (block, member) exactly once
    xcd = np.arange(units) % 8                                          # workgroups go to the XCDs round robin
    for c in range(8):
        mine = unit[xcd == c]                                           # in launch order: one run of consecutive units
        assert np.array_equal(mine, mine[0] + np.arange(len(mine))) if len(mine) else True, (c, mine[:10])
    sample = np.unique(np.concatenate([np.arange(min(units, 40)), np.arange(max(units - 40, 0), units),
                                       np.random.default_rng(nblocks * 31 + members).integers(0, units, 60)]))
    assert np.array_equal(order[sample], _units(L.lf_land_members_unit, nblocks, members, sample))


def test_unit_positions_outside_the_launch_are_refused():
    L = _lib.lib()
    block, member = C.c_int64(), C.c_int()
    for nblocks, members, position in ((9, 3, 27), (9, 3, -1), (0, 3, 0), (9, 0, 0), (2 ** 30, 4, 0)):
        assert L.lf_module_members_unit(nblocks, members, position, C.byref(block), C.byref(member)) == _lib.LF_E_INVALID
    assert L.lf_module_members_unit(9, 3, 0, None, C.byref(member)) == _lib.LF_E_INVALID
