"""Shared by tests/test_report_rasters_cpu.py and tests/test_report_rasters_gpu.py: the numpy restatement of
lf_pack_rasters_device (np.where over the index table, astype), the value set with the float32 bit pattern each value must
become, written out by hand, and the one call of the entry point both tests make."""
import ctypes as C

import numpy as np

FILL = -9999.0
SENTINEL = -777.25
F64, F32, I32 = 0, 1, 2                        # LF_PACK_F64 / LF_PACK_F32 / LF_PACK_I32
KIND = {np.dtype(np.float64): F64, np.dtype(np.float32): F32, np.dtype(np.int32): I32}

# value -> bits of numpy's astype(float32): round to nearest even, subnormals kept, overflow to +-inf, the sign of a zero kept
VALUES = [
    (1.5, 0x3FC00000), (-2.75, 0xC0300000),                          # finite, both signs
    (0.0, 0x00000000), (-0.0, 0x80000000), (np.inf, 0x7F800000), (-np.inf, 0xFF800000), (np.nan, 0x7FC00000),
    (1e-40, 0x000116C2),                                             # float32 subnormal: 71362 * 2**-149
    (1e-46, 0x00000000),                                             # below half the smallest subnormal: zero
    (3.4e38, 0x7F7FC99E),                                            # just below float32 max: finite
    (3.5e38, 0x7F800000), (1e39, 0x7F800000),                        # past float32 max + half an ulp: inf
    (-3.5e38, 0xFF800000),
    (1 + 2.0 ** -24, 0x3F800000),                                    # a tie: down to the even 1.0
    (1 + 3 * 2.0 ** -24, 0x3F800002),                                # a tie: up to the even 1 + 2**-22
    (1 + 2.0 ** -24 + 2.0 ** -50, 0x3F800001),                       # just above a tie
    (FILL, 0xC61C3C00),                                              # the fill itself as a data value
]


def special_values():
    return np.array([v for v, _ in VALUES], np.float64)


def bits(a):
    """the array's bit patterns (uint32 / uint64), so that a NaN equals itself and -0.0 differs from 0.0"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def source(rng, rows, n, dtype=np.float64):
    """[rows, n] with the value set planted at random places (every value at least once when rows * n allows)"""
    if np.dtype(dtype) == np.int32:
        a = rng.integers(-50, 50, (rows, n)).astype(np.int32)
        if a.size >= 2:
            a.reshape(-1)[rng.permutation(a.size)[:2]] = (np.iinfo(np.int32).max, np.iinfo(np.int32).min)
        return a
    a = rng.normal(0.0, 100.0, (rows, n))
    v = special_values()
    at = rng.permutation(a.size)[:v.size]
    a.reshape(-1)[at] = v[:at.size]
    return a


def index_table(rng, cells, n, permuting, kinds=True):
    """int32 [cells]: entries into rows of n elements -- ascending (a land table) or permuted (a sweep-order table) -- with
    cells off the mask (-1) and land pixels outside the rows' domain (-2) among them; cells <= n"""
    at = rng.permutation(n)[:cells] if permuting else np.sort(rng.choice(n, cells, replace=False))
    idx = at.astype(np.int32)
    if kinds and cells >= 3:
        where = rng.permutation(cells)
        idx[where[:cells // 4]] = -1
        idx[where[cells // 4:cells // 4 + max(cells // 7, 1)]] = -2
    return idx


def pack_reference(rows, idx, divisor, dst_dtype, fill=FILL):
    """[rows, cells] of dst_dtype: what lf_pack_rasters_device leaves of the source rows [rows, n]"""
    dst_dtype = np.dtype(dst_dtype)
    x = rows if divisor == 1.0 else rows / np.float64(divisor)
    with np.errstate(over="ignore", invalid="ignore"):
        x = x.astype(dst_dtype)
    gathered = x[:, np.where(idx >= 0, idx, 0)]
    outside = np.where(idx == -1, dst_dtype.type(fill), dst_dtype.type(0))
    return np.where(idx >= 0, gathered, outside[None]).astype(dst_dtype, copy=False)


def layout(rows, stride, sentinel):
    """[rows, n] -> flat [rows * stride] with the sentinel between the rows"""
    host = np.full((rows.shape[0], stride), sentinel, rows.dtype)
    host[:, :rows.shape[1]] = rows
    return host.reshape(-1)


def pack_call(L, nmaps, src, dst, rows, stride, src_kind, dst_kind, divisor, idx, cells, fill=FILL, arrays=()):
    """lf_pack_rasters_device(0, ...) with the seven per-source arguments as Python lists (or, named in `arrays`, as the
    ctypes value given: None for a NULL array)"""
    def arr(name, ctype, v):
        return v if name in arrays else (ctype * len(v))(*v)
    return L.lf_pack_rasters_device(0, nmaps, arr("src", C.c_void_p, src), arr("dst", C.c_void_p, dst),
                                    arr("rows", C.c_int32, rows), arr("stride", C.c_int64, stride),
                                    arr("src_kind", C.c_int32, src_kind), arr("dst_kind", C.c_int32, dst_kind),
                                    arr("divisor", C.c_double, divisor), idx, cells, fill)
