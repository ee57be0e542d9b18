"""No GPU: the ensemble form of the land surface (lf_soil_columns_members_device, lf_land_columns_members_device,
lf_soil_last_form, lf_land_members_unit) on the host side -- the four exports in the header, the library and the ctypes table,
every refusal before a device is touched, and the order in which the member launch hands its (tile, member) units to the
workgroups: a bijection, the workgroups of one XCD (position mod 8) on one run of consecutive units of the tile-major order,
at most 7 tiles with members on two XCDs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from lisflood_amd import _lib
from lisflood_amd.soilloop import _CanopyArgs, _SoilArgs

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
EXPORTS = {"lf_soil_columns_members_device": "ipiiqq", "lf_land_columns_members_device": "ipppiiqq",
           "lf_soil_last_form": "i", "lf_land_members_unit": "qiqpp"}
TILE = 256
V, N = 3, 600                      # 3 tiles per row, 9 per member
ES = C.c_void_p(8)                 # never dereferenced: every call here ends before a device is touched, or without one


def test_the_four_exports_are_in_the_header_the_library_and_the_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + name: sig for sig, names in _lib._SIGNATURES.items() for name in names.split()}
    L = _lib.lib()
    for name, sig in EXPORTS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert re.search(r"\sT\s+%s$" % name, dynamic, flags=re.M), name
        assert table[name] == sig, name
        assert list(getattr(L, name).argtypes) == [_lib._KIND[k] for k in sig] and getattr(L, name).restype is C.c_int


def _blocks(n_canopy=N):
    """-> (canopy block, soil block, what keeps their host arrays alive): no vector named, identity land-use rows"""
    idx = np.arange(V, dtype=np.int64)
    paddy = np.zeros(V, np.uint8)
    s = _SoilArgs()
    s.index_landuse_all, s.is_paddy_irrig = idx.ctypes.data, paddy.ctypes.data
    s.V, s.L, s.N = V, V, N
    s.DtDay, s.CourantCrit = 1.0, 0.4
    c = _CanopyArgs()
    c.index_landuse = idx.ctypes.data
    c.V, c.L, c.N = V, V, n_canopy
    return c, s, (idx, paddy)


def _soil(s, members, stride, fstride):
    return _lib.lib().lf_soil_columns_members_device(0, C.byref(s), 1, members, stride, fstride)


def _land(c, s, members, stride, fstride):
    return _lib.lib().lf_land_columns_members_device(0, C.byref(c), C.byref(s), ES, 1, members, stride, fstride)


TOO_MANY = (2 ** 31) // 9 + 1      # members * 9 tiles is beyond the 32-bit range of a launch
REFUSED = {
    "members_0": (0, V * N, N, b"members"),
    "members_negative": (-2, V * N, N, b"members"),
    "member_stride_short": (2, V * N - 1, N, b"member_stride"),
    "member_stride_0": (2, 0, N, b"member_stride"),
    "forcing_stride_1": (2, V * N, 1, b"forcing_member_stride"),
    "forcing_stride_short": (2, V * N, N - 1, b"forcing_member_stride"),
    "forcing_stride_negative": (2, V * N, -N, b"forcing_member_stride"),
    "units_beyond_32_bits": (TOO_MANY, V * N, 0, b"32-bit"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_member_arguments_are_refused_before_any_device(case):
    members, stride, fstride, word = REFUSED[case]
    c, s, keep = _blocks()
    for rc in (_soil(s, members, stride, fstride), _land(c, s, members, stride, fstride)):
        assert rc == _lib.LF_E_INVALID, case
        assert word in _lib.lib().lf_last_error(), (case, _lib.lib().lf_last_error())


def test_the_checks_of_the_single_call_are_inherited():
    L = _lib.lib()
    c, s, keep = _blocks(n_canopy=N + 1)                               # canopy and soil disagree about N
    assert _land(c, s, 2, V * N, N) == _lib.LF_E_INVALID and b"same V = L and N" in L.lf_last_error()
    c, s, keep = _blocks()
    s.L = V + 1                                                        # V != L
    assert _land(c, s, 2, V * N, N) == _lib.LF_E_INVALID and b"same V = L and N" in L.lf_last_error()
    c, s, keep = _blocks()
    keep[0][:] = [0, 0, 2]                                             # not the identity
    assert _land(c, s, 2, V * N, N) == _lib.LF_E_INVALID and b"index_landuse" in L.lf_last_error()
    c, s, keep = _blocks()
    keep[1][1] = 1                                                     # a paddy fraction
    assert _land(c, s, 2, V * N, N) == _lib.LF_E_INVALID and b"paddy" in L.lf_last_error()
    c, s, keep = _blocks()
    c.W1a = 64                                                         # the two blocks name different W1a vectors
    assert _land(c, s, 2, V * N, N) == _lib.LF_E_INVALID and b"different vectors" in L.lf_last_error()
    c, s, keep = _blocks()
    assert L.lf_land_columns_members_device(0, None, C.byref(s), ES, 1, 2, V * N, N) == _lib.LF_E_INVALID
    assert L.lf_land_columns_members_device(0, C.byref(c), None, ES, 1, 2, V * N, N) == _lib.LF_E_INVALID
    assert L.lf_land_columns_members_device(0, C.byref(c), C.byref(s), None, 1, 2, V * N, N) == _lib.LF_E_INVALID
    assert L.lf_soil_columns_members_device(0, None, 1, 2, V * N, N) == _lib.LF_E_INVALID


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_a_valid_call_needs_a_device():
    c, s, keep = _blocks()
    for members, stride, fstride in ((1, V * N, 0), (2, V * N, 0), (3, V * N + 5, N + 5), (TOO_MANY - 1, V * N, N)):
        assert _soil(s, members, stride, fstride) == _lib.LF_E_NO_DEVICE, (members, stride, fstride)
        assert _land(c, s, members, stride, fstride) == _lib.LF_E_NO_DEVICE, (members, stride, fstride)
    assert _lib.lib().lf_soil_last_form(0) == _lib.LF_E_NO_DEVICE


def _order(ntiles, members):
    """-> [units, 2]: (tile, member) of every launch position"""
    L = _lib.lib()
    tile, member = C.c_int64(-1), C.c_int(-1)
    out = np.empty((ntiles * members, 2), np.int64)
    for p in range(ntiles * members):
        assert L.lf_land_members_unit(ntiles, members, p, C.byref(tile), C.byref(member)) == _lib.LF_OK
        out[p] = tile.value, member.value
    return out


@pytest.mark.parametrize("members", [1, 2, 3, 8, 17])
@pytest.mark.parametrize("ntiles", [1, 7, 8, 9, 75, 1000])
def test_launch_order_keeps_the_members_of_a_tile_on_one_xcd(ntiles, members):
    order = _order(ntiles, members)
    units = ntiles * members
    assert ((order[:, 0] >= 0) & (order[:, 0] < ntiles) & (order[:, 1] >= 0) & (order[:, 1] < members)).all()
    unit = order[:, 0] * members + order[:, 1]                          # the tile-major order
    assert np.array_equal(np.sort(unit), np.arange(units))              # every (tile, member) exactly once
    xcd = np.arange(units) % 8                                          # workgroups go to the XCDs round robin
    for c in range(8):
        mine = unit[xcd == c]                                           # in launch order
        assert np.array_equal(mine, mine[0] + np.arange(len(mine))) if len(mine) else True, (c, mine[:10])
    xcds_of_tile = [len(set(xcd[order[:, 0] == t])) for t in range(ntiles)]
    assert sum(n > 1 for n in xcds_of_tile) <= 7, xcds_of_tile
    if units >= 8 * members:                                            # room for whole tiles: most tiles sit on one XCD
        assert sum(n == 1 for n in xcds_of_tile) >= ntiles - 7


def test_positions_outside_the_launch_are_refused():
    L = _lib.lib()
    tile, member = C.c_int64(), C.c_int()
    for ntiles, members, position in ((9, 3, 27), (9, 3, -1), (0, 3, 0), (9, 0, 0), (2 ** 30, 4, 0)):
        assert L.lf_land_members_unit(ntiles, members, position, C.byref(tile), C.byref(member)) == _lib.LF_E_INVALID
    assert L.lf_land_members_unit(9, 3, 0, None, C.byref(member)) == _lib.LF_E_INVALID
