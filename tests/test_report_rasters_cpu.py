"""No GPU: the host side of the report rasters -- lf_pack_rasters_device and the download protocol (lf_report_acquire,
lf_download_begin / _copy / _end / _wait) are in the header, the library and the ctypes table; every refusal that needs no
device comes back with its message; output.raster_index against a cell-by-cell loop; the restatement the device test
compares with (report_rasters.py) against float32 bit patterns written out by hand; a float32 map through
NetCDF4MapWriter.write_step."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import report_rasters as RR
from lisflood_amd import _lib, output

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
CELLS = 600
FAKE = 64                         # a pointer that is never dereferenced: every call here ends before a device is touched
EXPORTS = {"lf_pack_rasters_device": "iippppppppqd", "lf_report_acquire": "ii", "lf_download_begin": "ii",
           "lf_download_copy": "ippz", "lf_download_end": "ii", "lf_download_wait": "ii"}


def last_error():
    return _lib.lib().lf_last_error()


def pack(nmaps=2, src=(FAKE, FAKE), dst=(FAKE, FAKE), rows=(1, 3), stride=(0, CELLS + 5), src_kind=(RR.F64, RR.F64),
         dst_kind=(RR.F32, RR.F64), divisor=(1.0, 24.0), idx=C.c_void_p(FAKE), cells=CELLS, fill=RR.FILL, arrays=()):
    return RR.pack_call(_lib.lib(), nmaps, src, dst, rows, stride, src_kind, dst_kind, divisor, idx, cells, fill, arrays)


@pytest.mark.parametrize("name", list(EXPORTS))
def test_the_exports_are_in_the_header_the_library_and_the_table(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + n: sig for sig, names in _lib._SIGNATURES.items() for n in names.split()}
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert re.search(r"\sT\s+%s$" % name, dynamic, flags=re.M)
    assert table[name] == EXPORTS[name]
    f = getattr(_lib.lib(), name)
    assert list(f.argtypes) == [_lib._KIND[k] for k in EXPORTS[name]] and f.restype is C.c_int
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text).group(1)
    kinds = "".join("p" if "*" in p else {"int": "i", "int64_t": "q", "size_t": "z", "double": "d"}[" ".join(p.split()[:-1])]
                    for p in proto.split(","))
    assert kinds == EXPORTS[name], (name, kinds)


def test_the_kinds_of_the_header_are_the_ones_the_binding_uses():
    text = open(HEADER).read()
    for word, value in (("LF_PACK_F64", RR.F64), ("LF_PACK_F32", RR.F32), ("LF_PACK_I32", RR.I32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (word, value), text), word
    from lisflood_amd.hotpath import _HotPath
    assert _HotPath._PACK_KIND == RR.KIND and _HotPath._PACK_MAX == 16


PACK_REFUSED = {                  # arguments that differ from a valid call, a word of the message
    "nmaps_0": (dict(nmaps=0), b"nmaps"),
    "nmaps_17": (dict(nmaps=17), b"nmaps"),
    "nmaps_negative": (dict(nmaps=-1), b"nmaps"),
    "cells_negative": (dict(cells=-1), b"cells = -1"),
    "cells_beyond_32_bits": (dict(cells=2 ** 31), b"32-bit"),
    "rows_0": (dict(rows=(1, 0)), b"rows_host[1]"),
    "rows_negative": (dict(rows=(-3, 1)), b"rows_host[0]"),
    "stride_negative": (dict(stride=(0, -1)), b"stride_host[1]"),
    "src_kind_unknown": (dict(src_kind=(RR.F64, 3)), b"src_kind_host[1]"),
    "src_kind_float32": (dict(src_kind=(RR.F32, RR.F64)), b"src_kind_host[0]"),
    "dst_kind_unknown": (dict(dst_kind=(RR.F32, -1)), b"dst_kind_host[1]"),
    "int32_to_float32": (dict(src_kind=(RR.I32, RR.F64), dst_kind=(RR.F32, RR.F64)), b"int32 source to int32"),
    "fp64_to_int32": (dict(dst_kind=(RR.F32, RR.I32)), b"int32 source to int32"),
    "int32_with_a_divisor": (dict(src_kind=(RR.F64, RR.I32), dst_kind=(RR.F64, RR.I32)), b"divisor_host[1]"),
    "src_null": (dict(src=(FAKE, None)), b"src_dev[1]"),
    "dst_null": (dict(dst=(None, FAKE)), b"dst_dev[0]"),
    "idx_null": (dict(idx=None), b"idx_dev"),
}


@pytest.mark.parametrize("case", list(PACK_REFUSED))
def test_pack_refuses_bad_arguments_before_any_device(case):
    kw, word = PACK_REFUSED[case]
    assert pack(**kw) == _lib.LF_E_INVALID, case
    assert word in last_error() and b"pack rasters" in last_error(), (case, last_error())


@pytest.mark.parametrize("name", ["src", "dst", "rows", "stride", "src_kind", "dst_kind", "divisor"])
def test_pack_refuses_a_null_host_array(name):
    valid = dict(src=(C.c_void_p * 2)(FAKE, FAKE), dst=(C.c_void_p * 2)(FAKE, FAKE), rows=(C.c_int32 * 2)(1, 3),
                 stride=(C.c_int64 * 2)(0, CELLS), src_kind=(C.c_int32 * 2)(0, 0), dst_kind=(C.c_int32 * 2)(1, 0),
                 divisor=(C.c_double * 2)(1.0, 24.0))
    valid[name] = None
    assert pack(arrays=tuple(valid), **valid) == _lib.LF_E_INVALID
    assert b"is NULL" in last_error() and b"pack rasters" in last_error(), last_error()


def test_pack_names_the_first_bad_argument_only():
    assert pack(nmaps=0, cells=-1) == _lib.LF_E_INVALID and b"nmaps must be 1 to 16" in last_error()
    assert pack(rows=(0, 0), stride=(-1, -1)) == _lib.LF_E_INVALID and b"rows_host[0]" in last_error()


def test_pack_of_no_cells_is_done_without_a_device():
    assert pack(cells=0) == 0
    assert pack(cells=0, src=(None, None), dst=(None, None), idx=None) == 0
    assert pack(cells=0, rows=(0, 1)) == _lib.LF_E_INVALID         # (what is wrong is still refused)


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_a_valid_call_needs_a_device():
    L = _lib.lib()
    for kw in (dict(), dict(nmaps=1), dict(cells=2 ** 31 - 1), dict(divisor=(1.0, 1.0)),
               dict(src_kind=(RR.I32, RR.F64), dst_kind=(RR.I32, RR.F64))):
        assert pack(**kw) == _lib.LF_E_NO_DEVICE, kw
        assert b"no HIP device" in last_error()
    buf = np.zeros(4)
    for call in (lambda: L.lf_report_acquire(0, 0), lambda: L.lf_download_begin(0, 1), lambda: L.lf_download_end(0, 0),
                 lambda: L.lf_download_wait(0, 1), lambda: L.lf_download_copy(0, buf.ctypes.data_as(C.c_void_p), FAKE, 32),
                 lambda: L.lf_download_copy(0, None, None, 0)):
        assert call() == _lib.LF_E_NO_DEVICE
        assert b"no HIP device" in last_error()


@pytest.mark.parametrize("name", ["lf_report_acquire", "lf_download_begin", "lf_download_end", "lf_download_wait"])
def test_a_download_set_is_0_or_1(name):
    for bad in (-1, 2):
        assert getattr(_lib.lib(), name)(0, bad) == _lib.LF_E_INVALID
        assert b"download set must be 0 or 1" in last_error(), last_error()


def test_download_copy_refuses_null_with_bytes():
    L, buf = _lib.lib(), np.zeros(4)
    assert L.lf_download_copy(0, None, FAKE, 32) == _lib.LF_E_INVALID and b"lf_download_copy" in last_error()
    assert L.lf_download_copy(0, buf.ctypes.data_as(C.c_void_p), None, 32) == _lib.LF_E_INVALID and b"null" in last_error()


# ---- output.raster_index -------------------------------------------------------------------------------------------------
def masks():
    rng = np.random.default_rng(7)
    big = rng.random((23, 37)) < 0.7
    big[5] = False                                   # an all-sea row
    big[-1, -1] = True                               # land in the last cell
    big[0, 0] = False
    return {"1x1_land": np.ones((1, 1), bool), "1x1_sea": np.zeros((1, 1), bool), "1x257": rng.random((1, 257)) < 0.6,
            "23x37": big}


@pytest.mark.parametrize("case", list(masks()))
@pytest.mark.parametrize("rows", ["none", "permuted_with_outside"])
def test_raster_index_against_a_loop(case, rows):
    mask = masks()[case]
    n = int(mask.sum())
    rng = np.random.default_rng(n + 1)
    row_of_pixel = None
    if rows != "none":
        row_of_pixel = rng.permutation(n).astype(np.int64)
        row_of_pixel[rng.random(n) < 0.3] = -1          # pixels the rows' domain leaves out
        if n:
            row_of_pixel[-1] = -5                        # (any negative entry)
    got = output.raster_index(mask, row_of_pixel)
    assert got.dtype == np.int32 and got.shape == (mask.size,)
    want, p = [], 0
    for cell in range(mask.size):
        if not mask.reshape(-1)[cell]:
            want.append(-1)
            continue
        r = p if row_of_pixel is None else int(row_of_pixel[p])
        want.append(-2 if r < 0 else r)
        p += 1
    assert got.tolist() == want
    if case == "23x37":
        assert (got.reshape(mask.shape)[5] == -1).all() and got[-1] != -1 and ((got == -2).any() == (rows != "none"))
    # decompress is the gather through the table
    v = rng.normal(size=n)
    if row_of_pixel is None:
        assert np.array_equal(np.where(got >= 0, v[np.maximum(got, 0)] if n else 0.0, output.FILL).reshape(mask.shape),
                              output.decompress(v, mask))


def test_raster_index_refuses_a_table_of_another_length():
    with pytest.raises(ValueError, match="one entry per land pixel"):
        output.raster_index(np.ones((3, 4), bool), np.arange(11))


# ---- the restatement -----------------------------------------------------------------------------------------------------
def test_the_value_set_converts_to_the_bit_patterns_written_out_by_hand():
    v = RR.special_values()
    want = np.array([b for _, b in RR.VALUES], np.uint32)
    idx = np.arange(v.size, dtype=np.int32)
    got = RR.pack_reference(v[None], idx, 1.0, np.float32)
    assert got.dtype == np.float32 and got.shape == (1, v.size)
    assert RR.bits(got)[0].tolist() == want.tolist(), [hex(b) for b in RR.bits(got)[0]]
    same = RR.pack_reference(v[None], idx, 1.0, np.float64)
    assert RR.same_bits(same[0], v)                                    # fp64 -> fp64: the bits themselves
    for needed in (1e-40, 1e-46, 3.5e38, 1e39, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, RR.FILL, 0.0, np.inf):
        assert (v == needed).any(), needed
    assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all() and np.isnan(v).any() and np.isneginf(v).any()


def test_the_restatement_fills_zeroes_divides_and_gathers():
    rows = np.array([[24.0, -48.0, 7.0, np.nan], [1.0, 2.0, 3.0, -0.0]])
    idx = np.array([3, -1, 0, -2, 1, 1], np.int32)
    got = RR.pack_reference(rows, idx, 24.0, np.float32)
    want = np.array([[np.nan, RR.FILL, 1.0, 0.0, -2.0, -2.0], [-0.0, RR.FILL, 1 / 24, 0.0, 2 / 24, 2 / 24]]).astype(np.float32)
    assert RR.same_bits(got, want)
    assert np.float32(np.float64(1.0) / 24.0) == got[1, 2]             # the fp64 quotient, then the conversion
    ints = np.array([[5, -7, 2 ** 31 - 1]], np.int32)
    got = RR.pack_reference(ints, np.array([2, -1, 0, -2], np.int32), 1.0, np.int32)
    assert got.dtype == np.int32 and got.tolist() == [[2 ** 31 - 1, -9999, 5, 0]]
    padded = RR.layout(rows, 7, RR.SENTINEL).reshape(2, 7)
    assert RR.same_bits(padded[:, :4], rows) and (padded[:, 4:] == RR.SENTINEL).all()


# ---- the map writer takes what wait() hands out ---------------------------------------------------------------------------
def test_write_step_takes_a_float32_map(tmp_path):
    rng = np.random.default_rng(5)
    mask = rng.random((9, 13)) < 0.7
    v = rng.normal(0, 50, int(mask.sum()))
    raster = np.where(mask, output.decompress(v, mask).astype(np.float32), np.float32(output.FILL))
    assert raster.dtype == np.float32
    flat = np.zeros(raster.size * 4 + 64, np.uint8)                    # a view into a larger byte buffer, as wait() gives
    view = flat[64:].view(np.float32).reshape(raster.shape)
    view[:] = raster
    path = str(tmp_path / "dis.nc")
    with output.NetCDF4MapWriter(path, "dis", np.arange(13.0), np.arange(9.0)[::-1], time_values=[0.0, 1.0], dtype="f4") as w:
        w.write_step(0, view)
        w.write_step(1, raster)
    assert RR.same_bits(view, raster)                                  # the writer left its input alone
    got = output.read_netcdf4(path, "dis")[0]
    assert got.shape == (2, 9, 13) and np.isnan(got[0][~mask]).all()
    for t in (0, 1):
        assert np.array_equal(got[t][mask].astype(np.float32), raster[mask])
