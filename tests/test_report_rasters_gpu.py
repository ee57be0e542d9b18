"""Report rasters on the device.  lf_pack_rasters_device against its restatement (report_rasters.py) as bit patterns: every
size around a workgroup and around a lane's four cells, one and three rows with plain and padded strides (sentinels between
the rows and around every destination stay), the three kinds of table entry, ascending and permuting tables, fp64 -> fp64,
fp64 -> float32 and int32 -> int32, divisor 1 and 24, 1 / 9 / 16 sources in a call, destinations that take 16-byte stores and
ones that do not.  Then summary_rasters() and rasters() of both hot-path classes against summary() / chan_q_avg() / download()
decompressed on the host, on a mask with sea cells and a channel domain smaller than the land; requests waited for only after
the next step() has been issued, against a twin stepped in lockstep; the two buffer sets, stale handles and free()."""
import ctypes as C

import numpy as np
import pytest

import report_rasters as RR

pytestmark = pytest.mark.gpu

H, W, M, PAD = 24, 30, 3, 5
N = H * W
LAND_ROW = "DirectRunoff"
CELLS = [1, 255, 256, 257, 851, 4096]


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


# ---- the pack entry point ---------------------------------------------------------------------------------------------------
# (source type, destination type, rows, elements between the rows, divisor): 3 conversions x rows 1 / 3 x stride n / n + 37,
# the fp64 ones with divisor 1 and 24 in turn; then the four fp64 -> float32 ones with the other divisor
SPECS = [(s, d, rows, pad, 1.0 if s is np.int32 else (1.0, 24.0)[(i + j + k) % 2])
         for i, (s, d) in enumerate(((np.float64, np.float64), (np.float64, np.float32), (np.int32, np.int32)))
         for j, rows in enumerate((1, 3)) for k, pad in enumerate((0, 37))]
SPECS += [(s, d, rows, pad, 25.0 - div) for s, d, rows, pad, div in SPECS if d is np.float32]
assert len(SPECS) == 16


def run_pack(amd, cells, permuting, specs, seed, guard=4):
    """one call with the sources of `specs`; -> None, or the first thing that is not as the restatement says.  guard:
    sentinel elements in front of and behind every destination (4: the destination starts on a 16-byte boundary, 1: not)"""
    L = amd.lib()
    rng = np.random.default_rng(seed)
    n = cells + 13
    idx = RR.index_table(rng, cells, n, permuting)
    d_idx = amd.DeviceArray.from_host(idx)
    held, want, images = [], [], []
    for s, d, rows, pad, div in specs:
        src = RR.source(rng, rows, n, s)
        image = RR.layout(src, n + pad, np.dtype(s).type(RR.SENTINEL))
        out = np.full(rows * cells + 2 * guard, np.dtype(d).type(RR.SENTINEL), d)
        held.append((amd.DeviceArray.from_host(image), amd.DeviceArray.from_host(out)))
        images.append(image)
        want.append(RR.pack_reference(src, idx, div, d))
    rc = RR.pack_call(L, len(specs), [h[0].ptr.value for h in held],
                      [h[1].ptr.value + guard * np.dtype(sp[1]).itemsize for h, sp in zip(held, specs)],
                      [sp[2] for sp in specs], [n + sp[3] for sp in specs], [RR.KIND[np.dtype(sp[0])] for sp in specs],
                      [RR.KIND[np.dtype(sp[1])] for sp in specs], [sp[4] for sp in specs], d_idx.ptr, cells)
    amd.check(rc)
    bad = None
    for k, (sp, (d_src, d_dst)) in enumerate(zip(specs, held)):
        got, sentinel = d_dst.download(), np.dtype(sp[1]).type(RR.SENTINEL)
        body = got[guard:got.size - guard].reshape(sp[2], cells)
        if bad is None and not RR.same_bits(body, want[k]):
            at = np.argwhere(RR.bits(body) != RR.bits(want[k]))[0]
            bad = ("source %d %s" % (k, sp), tuple(at), idx[at[1]], body[tuple(at)], want[k][tuple(at)])
        if bad is None and not ((got[:guard] == sentinel).all() and (got[got.size - guard:] == sentinel).all()):
            bad = ("source %d %s: written outside the destination" % (k, sp), got[:guard], got[got.size - guard:])
        if bad is None and not RR.same_bits(d_src.download(), images[k]):
            bad = ("source %d %s: the source rows or their gaps changed" % (k, sp),)
        d_src.free(); d_dst.free()
    d_idx.free()
    return bad


@pytest.mark.parametrize("permuting", [False, True], ids=["ascending", "permuting"])
@pytest.mark.parametrize("cells", CELLS)
def test_pack_against_the_restatement(amd, cells, permuting):
    seed = 7 * cells + permuting
    assert run_pack(amd, cells, permuting, SPECS, seed) is None                                   # 16 sources, mixed rows
    one_row = [sp for sp in SPECS if sp[2] == 1] + [(np.float64, np.float32, 1, 3, 24.0)]
    assert len(one_row) == 9
    assert run_pack(amd, cells, permuting, one_row, seed + 1) is None                            # 9 sources of one row each
    for k in (cells % 16, (cells + 5) % 16):                                                     # 1 source
        assert run_pack(amd, cells, permuting, SPECS[k:k + 1], seed + 2 + k) is None
        assert run_pack(amd, cells, permuting, SPECS[k:k + 1], seed + 2 + k, guard=1) is None    # (no 16-byte boundary)


def test_pack_carries_the_special_values(amd):
    """every value of the set, through each conversion, on both store paths, with the bit patterns written out by hand"""
    L = amd.lib()
    v = RR.special_values()
    want32 = np.array([b for _, b in RR.VALUES], np.uint32)
    d_src = amd.DeviceArray.from_host(v)
    d_idx = amd.DeviceArray.from_host(np.arange(v.size, dtype=np.int32))
    for guard in (4, 1):
        d32 = amd.DeviceArray.from_host(np.zeros(v.size + 2 * guard, np.float32))
        d64 = amd.DeviceArray.from_host(np.zeros(v.size + 2 * guard, np.float64))
        amd.check(RR.pack_call(L, 2, [d_src.ptr.value] * 2, [d32.ptr.value + 4 * guard, d64.ptr.value + 8 * guard], [1, 1], [0, 0],
                               [RR.F64] * 2, [RR.F32, RR.F64], [1.0, 1.0], d_idx.ptr, v.size))
        got32, got64 = d32.download()[guard:guard + v.size], d64.download()[guard:guard + v.size]
        assert RR.bits(got32).tolist() == want32.tolist(), (guard, [hex(b) for b in RR.bits(got32)])
        assert RR.same_bits(got64, v), guard
        d32.free(); d64.free()
    d_src.free(); d_idx.free()


def test_the_download_protocol_refuses_what_is_out_of_order(amd):
    L = amd.lib()
    amd.synchronize(0)
    dev = amd.DeviceArray.from_host(np.arange(64.0))
    pin = amd.PinnedArray(64, np.float64)
    INVALID = amd.LF_E_INVALID
    assert L.lf_download_copy(0, pin.ptr, dev.ptr, 512) == INVALID and b"outside lf_download_begin" in L.lf_last_error()
    assert L.lf_download_end(0, 0) == INVALID and b"without lf_download_begin" in L.lf_last_error()
    amd.check(L.lf_download_wait(0, 1))                              # never downloaded: returns at once
    amd.check(L.lf_report_acquire(0, 1))
    amd.check(L.lf_download_begin(0, 1))
    assert L.lf_download_begin(0, 0) == INVALID and b"still open" in L.lf_last_error()
    assert L.lf_download_end(0, 0) == INVALID and b"the other one" in L.lf_last_error()
    assert L.lf_download_copy(0, None, dev.ptr, 8) == INVALID
    amd.check(L.lf_download_copy(0, pin.ptr, dev.ptr, 512))
    amd.check(L.lf_download_copy(0, None, None, 0))
    amd.check(L.lf_download_end(0, 1))
    amd.check(L.lf_download_wait(0, 1))
    assert np.array_equal(pin.a, np.arange(64.0))
    amd.check(L.lf_device_trim(0))                                   # the stream and its events go; made again on next use
    amd.check(L.lf_download_wait(0, 1))
    dev.free(); pin.free()


# ---- the hot-path classes -----------------------------------------------------------------------------------------------------
def cp(d):
    return {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}


def scenario():
    """the smallest scenario of the ensemble tests, its all-land raster framed by sea: a sea column left and right, a sea
    row above and two below (pixel order and the flow directions are the ones of the raster alone)"""
    from lisflood_amd import synthetic as syn
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    framed = np.zeros((H + 3, W + 2), bool)
    framed[1:H + 1, 1:W + 1] = mask
    return values, sc, framed, ldd_to_chan, ldd_kin


def forcing(s, members=M):
    from lisflood_amd import synthetic as syn
    f = [syn.hotpath_forcing(N, s + 10 * m) for m in range(members)]
    return {k: np.stack([x[k] for x in f]) for k in f[0]}


def make(kind):
    from lisflood_amd.hotpath import HotPathDevice, HotPathEnsemble
    values, sc, mask, ldd_to_chan, ldd_kin = scenario()
    if kind == "ensemble":
        obj = HotPathEnsemble(cp(values), sc, mask, ldd_to_chan, ldd_kin, members=M, pad=PAD)
    else:
        obj = HotPathDevice(cp(values), sc, mask, ldd_to_chan, ldd_kin)
    assert obj.Nk < obj.N == N and not mask.all() and obj._outside.size         # a channel domain smaller than the land; sea
    return obj


def step(obj, s):
    f = forcing(s)
    obj.step(f if hasattr(obj, "members") else {k: a[0] for k, a in f.items()}, time_since_start=s + 1)


@pytest.fixture(scope="module")
def ensemble(amd):
    ens = make("ensemble")
    for s in range(2):
        step(ens, s)
    yield ens
    ens.free()


def raster_of(obj, a, dtype, fill=RR.FILL):
    """[..., N] in pixel order -> [..., H, W] of dtype as the host makes it today: decompress, astype, the fill off the mask"""
    from lisflood_amd import output
    a = np.asarray(a)
    maps = np.stack([output.decompress(row, obj.land_mask) for row in a.reshape(-1, a.shape[-1])])
    with np.errstate(over="ignore"):
        maps = np.where(obj.land_mask, maps.astype(dtype), np.dtype(dtype).type(fill))
    return maps.reshape(a.shape[:-1] + obj.land_mask.shape)


def thresholds_for(ens, x, seed):
    """two maps in pixel order around the members' values: a NaN, +-0.0 and, on pixels outside the channel domain, negative
    entries (every member is 0.0 there: all of them exceed)"""
    rng = np.random.default_rng(seed)
    thr = np.stack([np.median(x, axis=0), x.max(axis=0)]) * rng.choice([0.5, 1.0, 1.5], (2, x.shape[1]))
    thr[0, ::97] = np.nan
    thr[1, 5::89] = -0.0
    thr[0, ens._outside[::2]] = -1.0
    thr[1, ens._outside[1::3]] = -0.5
    return thr


def check_summary(ens, name, dtype, thr, ranks):
    got = ens.summary_rasters(name, thresholds=thr, ranks=ranks, dtype=dtype).wait()
    ref = ens.summary(name, thresholds=thr, ranks=ranks)
    assert sorted(got) == sorted(ref) == ["exceed", "max", "mean", "min", "order"]
    for k in ref:
        want = raster_of(ens, ref[k], np.int32 if k == "exceed" else dtype)
        assert RR.same_bits(got[k], want), (name, k, np.argwhere(RR.bits(got[k]) != RR.bits(want))[:3])
    return got, ref


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["ChanQAvg", "ChanQ", LAND_ROW])
def test_summary_rasters_are_the_summary_decompressed(ensemble, name, dtype):
    ens = ensemble
    x = ens.chan_q_avg() if name == "ChanQAvg" else ens.download(name)
    assert np.abs(x).max() > 0
    thr = thresholds_for(ens, x, 5)
    got, ref = check_summary(ens, name, dtype, thr, (0, M - 1))
    assert got["mean"].shape == ens.land_mask.shape and got["exceed"].shape == (2,) + ens.land_mask.shape
    assert got["order"].shape == (2,) + ens.land_mask.shape and got["exceed"].dtype == np.int32 and got["mean"].dtype == dtype
    assert (got["mean"][~ens.land_mask] == RR.FILL).all() and (got["exceed"][:, ~ens.land_mask] == -9999).all()
    if name != LAND_ROW:                       # outside the channel domain: 0.0 and members x (0.0 > threshold)
        out = ens._outside
        assert (ref["mean"][out] == 0).all() and (ref["exceed"][0, out[::2]] == M).all() and (ref["exceed"][:, out] == 0).any()
    # parts of it, another fill
    some = ens.summary_rasters(name, mean=False, maximum=False, dtype=dtype, fill=1e20).wait()
    assert sorted(some) == ["min"] and RR.same_bits(some["min"], raster_of(ens, ref["min"], dtype, 1e20))


def test_a_land_row_between_two_channel_rows_does_not_show_outside_the_domain(ensemble):
    """the product maps are shared: a land row fills every pixel of them, the channel row after it must read 0.0 / the
    exceedance of 0.0 outside the channel domain again -- also with another threshold set and another number of thresholds"""
    ens = ensemble
    thr = thresholds_for(ens, ens.chan_q_avg(), 8)
    check_summary(ens, "ChanQAvg", np.float32, thr, (1,))
    check_summary(ens, LAND_ROW, np.float32, thr, (1,))
    check_summary(ens, "ChanQ", np.float32, thr, (1,))
    other = thr[::-1].copy()
    check_summary(ens, "ChanQ", np.float64, other, (0, 1, 2))
    got = ens.summary_rasters("ChanQ", thresholds=other[0], dtype=np.float32).wait()
    assert RR.same_bits(got["exceed"], raster_of(ens, ens.summary("ChanQ", thresholds=other[0])["exceed"], np.int32))
    ens.summary(LAND_ROW, thresholds=thr)                            # summary() itself fills the shared maps too
    check_summary(ens, "ChanQAvg", np.float32, thr, (1,))


def host_rasters(obj, names, dtype):
    return {k: raster_of(obj, obj.chan_q_avg() if k == "ChanQAvg" else obj.download(k), dtype) for k in names}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ensemble_rasters_are_the_downloads_decompressed(ensemble, dtype):
    ens = ensemble
    names = ["ChanQAvg", LAND_ROW, "ChanQ", "sumDisDay"]
    got = ens.rasters(names, dtype=dtype).wait()
    want = host_rasters(ens, names, dtype)
    assert sorted(got) == sorted(names)
    for k in names:
        assert got[k].shape == (M,) + ens.land_mask.shape and RR.same_bits(got[k], want[k]), k
        assert np.abs(want[k][:, ens.land_mask]).max() > 0
    with pytest.raises(ValueError, match="neither a channel row"):
        ens.rasters(["ChanQ", "W1a"])
    with pytest.raises(ValueError, match="twice"):
        ens.rasters(["ChanQ", "ChanQ"])
    with pytest.raises(ValueError, match="float32 or float64"):
        ens.rasters(["ChanQ"], dtype=np.int32)
    with pytest.raises(ValueError, match="1 to 16 maps"):
        ens.rasters([])


@pytest.mark.parametrize("kind", ["ensemble", "device"])
def test_rasters_requested_before_the_next_step_are_the_ones_of_their_step(amd, kind):
    """four steps; the rasters of a step are requested right after it and waited for only once the next step() has been
    issued; a twin stepped in lockstep gives the same step's maps synchronously.  The device object shows here that its
    rasters() are its download() / chan_q_avg(), and that the run itself is the twin's."""
    obj, twin = make(kind), make(kind)
    names = ["ChanQAvg", LAND_ROW, "ChanQ"]
    pending, want = None, None
    for s in range(4):
        step(obj, s)
        step(twin, s)
        if pending is not None:                  # of step s - 1, while step s is in flight
            for handle, ref in zip(pending, want):
                got = handle.wait()
                for k in ref:
                    assert RR.same_bits(got[k], ref[k]), (kind, s - 1, k)
        pending, want = [obj.rasters(names)], [host_rasters(twin, names, np.float32)]           # one request per buffer set
        if kind == "ensemble":
            thr = thresholds_for(twin, twin.chan_q_avg(), s)
            pending.append(obj.summary_rasters("ChanQAvg", thresholds=thr, ranks=(1,)))
            want.append({k: raster_of(twin, a, np.int32 if k == "exceed" else np.float32)
                         for k, a in twin.summary("ChanQAvg", thresholds=thr, ranks=(1,)).items()})
        else:
            pending.append(obj.rasters(names[:1], dtype=np.float64))
            want.append(host_rasters(twin, names[:1], np.float64))
    for handle, ref in zip(pending, want):
        got = handle.wait()
        for k in ref:
            assert RR.same_bits(got[k], ref[k]) and np.abs(ref[k][..., obj.land_mask]).max() > 0, (kind, 3, k)
    for k in obj.state_names():                  # the requests changed nothing of the run
        assert RR.same_bits(obj.download(k), twin.download(k)), k
    if kind == "device":
        with pytest.raises(ValueError, match="neither a channel vector"):
            obj.rasters(["Rain"])
        with pytest.raises(ValueError, match="neither a channel vector"):
            obj.rasters(["W1a"])
    obj.free(); twin.free()


def test_a_handle_holds_until_its_set_is_used_again_and_free_leaves_nothing(amd):
    L = amd.lib()
    ens = make("ensemble")
    step(ens, 0)
    first = ens.rasters(["ChanQAvg"])
    kept = {k: a.copy() for k, a in first.wait().items()}
    step(ens, 1)
    second = ens.rasters(["ChanQAvg"])                               # the other set
    assert second.buffer_set != first.buffer_set
    newer = second.wait()["ChanQAvg"]
    assert RR.same_bits(first.wait()["ChanQAvg"], kept["ChanQAvg"]) and not RR.same_bits(newer, kept["ChanQAvg"])
    third = ens.rasters(["ChanQAvg"])                                # the first set again
    assert third.buffer_set == first.buffer_set
    with pytest.raises(RuntimeError, match="stale PendingRasters handle"):
        first.wait()
    assert RR.same_bits(second.wait()["ChanQAvg"], newer) and RR.same_bits(third.wait()["ChanQAvg"], newer)
    sets = list(ens._report_sets)
    assert all(st is not None for st in sets)
    ens.free()
    assert ens._report_sets == [None, None] and ens._report_tables == {}
    assert all(d.ptr.value is None and p.ptr.value is None for d, p in sets)    # device staging and page-locked image: freed
    for handle in (second, third):
        with pytest.raises(RuntimeError, match="stale PendingRasters handle"):
            handle.wait()
    amd.check(L.lf_device_trim(0))                                   # nothing of the download sets is in use any more
    for b in (0, 1):
        amd.check(L.lf_download_wait(0, b))
