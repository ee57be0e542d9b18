"""No GPU: the host side of lf_upload_rows, the upload of an ensemble's forcing rows as the caller holds them (raw copy into
a staging buffer + a gather / widen kernel on the copy stream).  The export is in the header, the library and the ctypes
table; every refusal comes back as LF_E_INVALID with the argument named before a device is touched; a valid call then needs a
device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from lisflood_amd import _lib

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
N = 600
FAKE = C.c_void_p(64)              # a pointer that is never dereferenced: every call here ends before a device is touched


def last_error():
    return _lib.lib().lf_last_error()


def upload(dst=FAKE, dst_stride=N, rows=3, src=FAKE, src_rows=3, src_f32=0, n=N, index=FAKE):
    return _lib.lib().lf_upload_rows(0, dst, dst_stride, rows, src, src_rows, src_f32, n, index)


def test_the_export_is_in_the_header_the_library_and_the_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + name: sig for sig, names in _lib._SIGNATURES.items() for name in names.split()}
    assert re.search(r"\bint\s+lf_upload_rows\s*\(", text)
    assert re.search(r"\sT\s+lf_upload_rows$", dynamic, flags=re.M)
    assert table["lf_upload_rows"] == "ipqipiiqp"
    f = _lib.lib().lf_upload_rows
    assert list(f.argtypes) == [_lib._KIND[k] for k in "ipqipiiqp"] and f.restype is C.c_int
    proto = re.search(r"\bint\s+lf_upload_rows\s*\(([^)]*)\)", text).group(1)
    names = [p.split()[-1].lstrip("*") for p in proto.split(",")]
    assert names == ["device", "dst_dev", "dst_stride", "rows", "src_host", "src_rows", "src_f32", "n", "index_dev"], names


REFUSED = {                        # arguments that differ from a valid call, the word of the message
    "rows_0": (dict(rows=0, src_rows=1), b"rows"),
    "rows_negative": (dict(rows=-2, src_rows=1), b"rows"),
    "src_rows_0": (dict(src_rows=0), b"src_rows"),
    "src_rows_2_of_3": (dict(src_rows=2), b"src_rows"),
    "src_rows_more": (dict(src_rows=4), b"src_rows"),
    "src_rows_negative": (dict(src_rows=-1), b"src_rows"),
    "src_f32_2": (dict(src_f32=2), b"src_f32"),
    "src_f32_negative": (dict(src_f32=-1), b"src_f32"),
    "n_negative": (dict(n=-1), b"n = -1"),
    "n_beyond_32_bits": (dict(n=2 ** 31, dst_stride=2 ** 31), b"32-bit"),
    "dst_stride_short": (dict(dst_stride=N - 1), b"dst_stride"),
    "dst_stride_0": (dict(dst_stride=0), b"dst_stride"),
    "dst_null": (dict(dst=None), b"dst_dev"),
    "src_null": (dict(src=None), b"src_host"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_bad_arguments_are_refused_before_any_device(case):
    kw, word = REFUSED[case]
    for f32 in (0, 1):
        assert upload(**dict(dict(src_f32=f32), **kw)) == _lib.LF_E_INVALID, case
        assert word in last_error() and b"upload rows" in last_error(), (case, last_error())


def test_a_refusal_names_the_first_bad_argument_only():
    assert upload(rows=0, src_rows=5, src_f32=7) == _lib.LF_E_INVALID and b"rows must be at least 1" in last_error()
    assert upload(src_rows=2, src_f32=7) == _lib.LF_E_INVALID and b"src_rows must be 1 or rows" in last_error()


def test_the_sources_of_the_device_test_hold_the_special_values():
    """what tests/test_members_upload_gpu.py feeds the kernel: +-0, +-inf, a NaN, float32 denormals and float32 max in a
    source of either type, and its reference keeps them (the sign of a zero included)"""
    import members_upload as MU
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        a = MU.source(rng, 3, 257, dtype)
        bits = a.view(np.uint32 if dtype is np.float32 else np.uint64)
        zero_neg = 1 << (31 if dtype is np.float32 else 63)
        assert (bits == 0).any() and (bits == zero_neg).any() and np.isposinf(a).any() and np.isneginf(a).any() and np.isnan(a).any()
        assert (a == float(MU.F32.max)).any() and (a == dtype(1e-45)).any()
        if dtype is np.float32:
            assert ((np.abs(a) < MU.F32.tiny) & (a != 0)).sum() >= 3
        want = MU.reference(a, 3, None)
        assert MU.same_bits(want, a.astype(np.float64)) and np.signbit(want[bits == zero_neg]).all()
        perm = rng.permutation(257)
        assert MU.same_bits(MU.reference(a[:1], 3, perm), np.broadcast_to(a[:1].astype(np.float64)[:, perm], (3, 257)))


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_a_valid_call_needs_a_device():
    for kw in (dict(), dict(src_rows=1), dict(src_f32=1), dict(index=None), dict(dst_stride=N + 7), dict(rows=1, src_rows=1),
               dict(n=2 ** 31 - 1, dst_stride=2 ** 31 - 1), dict(n=0, dst=None, src=None, index=None, dst_stride=0)):
        assert upload(**kw) == _lib.LF_E_NO_DEVICE, kw
        assert b"no HIP device" in last_error()
