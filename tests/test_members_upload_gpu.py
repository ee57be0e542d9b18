"""The double-buffered forcing upload of an ensemble, on the device: lf_upload_rows (raw copy into a staging buffer, then a
kernel on the copy stream that gathers into sweep order, widens and writes every member's row) against numpy bit for bit,
its staging buffers under reuse, and hotpath.HotPathEnsemble fed through prefetch / pinned_forcing / step(rows) against one
HotPathDevice per member fed the same arrays by its blocking step."""
import ctypes as C

import numpy as np
import pytest

import members_upload as MU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


# ---- 1. the kernel against numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("rows", [1, 3, 9])                  # 9 crosses a row slice
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_rows_arrive_as_numpy_orders_and_widens_them(amd, n, rows, dtype):
    """reference: src.astype(np.float64)[..., index]; every combination of one source row / a row per destination row,
    permutation / no index table, dense / padded destination, pageable / page-locked source"""
    rng = np.random.default_rng(1000 * n + 10 * rows + (dtype is np.float32))
    perm = rng.permutation(n).astype(np.int32)
    d_perm = amd.DeviceArray.from_host(perm)
    dst = amd.DeviceArray(rows * (n + 7))
    calls = 0
    for src_rows in sorted({1, rows}):
        pinned = amd.PinnedArray((src_rows, n), dtype)
        for index, d_index in ((perm, d_perm), (None, None)):
            for dst_stride in (n, n + 7):
                for page_locked in (False, True):
                    what = (src_rows, index is not None, dst_stride, page_locked)
                    src = MU.source(rng, src_rows, n, dtype)
                    want = MU.reference(src, rows, index).copy()
                    if page_locked:
                        pinned.a[...] = src
                        src = pinned.a
                    dst.upload(np.full(rows * (n + 7), MU.SENTINEL))
                    MU.upload_rows(amd, dst, dst_stride, rows, src, n, d_index, buffer_set=calls % 2)
                    if page_locked:                       # after lf_upload_wait the source belongs to the caller again
                        pinned.a[...] = 12345.0
                    MU.check_rows(dst, rows, n, dst_stride, want, what)
                    tail = dst.download()[rows * dst_stride:]
                    assert (tail == MU.SENTINEL).all(), (what, "written beyond the last row")
                    calls += 1
        pinned.free()
    assert calls == (8 if rows == 1 else 16)
    for d in (d_perm, dst):
        d.free()


def test_more_row_slices_than_one_grid_holds(amd):
    """8 * 65535 + 9 rows of two elements: the launch is sliced; a row per destination row and one row for all"""
    rows, n, stride = 8 * 65535 + 9, 2, 3
    rng = np.random.default_rng(11)
    swap = np.array([1, 0], np.int32)
    d_swap = amd.DeviceArray.from_host(swap)
    dst = amd.DeviceArray(rows * stride)
    for src_rows, dtype in ((rows, np.float32), (1, np.float64), (rows, np.float64)):
        src = rng.standard_normal((src_rows, n)).astype(dtype)
        dst.upload(np.full(rows * stride, MU.SENTINEL))
        MU.upload_rows(amd, dst, stride, rows, src, n, d_swap)
        MU.check_rows(dst, rows, n, stride, MU.reference(src, rows, swap), (src_rows, dtype))
    for d in (d_swap, dst):
        d.free()


# ---- 2. staging reuse -------------------------------------------------------------------------------------------------------
def test_staging_buffers_regrow_and_serve_two_destinations(amd):
    L = amd.lib()
    rng = np.random.default_rng(21)
    big_n, big_rows = 1000, 9
    perm = {n: rng.permutation(n).astype(np.int32) for n in (300, big_n)}
    d_perm = {n: amd.DeviceArray.from_host(p) for n, p in perm.items()}
    dst = [amd.DeviceArray.from_host(np.full(big_rows * big_n, MU.SENTINEL)) for _ in range(2)]

    def one(d, n, rows, dtype, src_rows=None, wait=True):
        src = MU.source(rng, src_rows or rows, n, dtype)
        MU.upload_rows(amd, dst[d], n, rows, src, n, d_perm[n], wait=wait)
        return src, MU.reference(src, rows, perm[n]).copy(), (d, n, rows)

    def check(job):
        _, want, (d, n, rows) = job
        got = dst[d].download()[:rows * n].reshape(rows, n)
        assert MU.same_bits(got, want), (d, n, rows, MU.first_difference(got, want))
    check(one(0, 300, 2, np.float32))                     # a small staging buffer ...
    check(one(0, big_n, big_rows, np.float64))            # ... replaced by a larger one
    check(one(0, 300, 3, np.float64))                     # ... which is kept for a smaller image
    check(one(0, 300, 5, np.float32, src_rows=1))
    # the two destinations alternately without a wait in between: each has its own staging buffer, the copy stream orders
    # the rest (the sources stay alive in `jobs` until the wait)
    jobs = [one(k % 2, (300, big_n)[(k // 2) % 2], 1 + k, (np.float32, np.float64)[k % 3 == 0], wait=False) for k in range(8)]
    amd.check(L.lf_upload_wait(0, 0))
    for d in (0, 1):                                      # what the last upload to each destination left
        check([j for j in jobs if j[2][0] == d][-1])
    # the widening copy of a single vector shares the destination's staging buffer
    v = rng.standard_normal(big_n).astype(np.float32)
    amd.check(L.lf_upload_begin(0, 1))
    amd.check(L.lf_upload_copy_f32(0, dst[1].ptr, v.ctypes.data_as(C.c_void_p), v.size))
    amd.check(L.lf_upload_end(0, 1))
    last = one(1, big_n, 2, np.float64, wait=False)
    amd.check(L.lf_upload_wait(0, 0))
    check(last)
    # after a trim the buffers are made again on demand
    amd.check(L.lf_device_trim(0))
    check(one(0, big_n, big_rows, np.float32))
    check(one(1, 300, 2, np.float64))
    for d in dst + list(d_perm.values()):
        d.free()


# ---- 3. the chain: HotPathEnsemble beside one HotPathDevice per member ------------------------------------------------------
@pytest.fixture(scope="module")
def scenario():
    return MU.make_scenario()


def new_ensemble(scenario, structures, overlap=True, members=MU.MEMBERS):
    from lisflood_amd.hotpath import HotPathEnsemble
    ens = MU.build(scenario, HotPathEnsemble, structures, members=members, pad=MU.PAD, overlap_channel=overlap)
    ens.set_gaps(MU.SENTINEL)
    return ens


def pinned_set(ens, kind):
    """a forcing dict of page-locked arrays with the shapes and types of MU.ensemble_forcing(kind, .)"""
    if kind == "mixed":
        return dict(ens.pinned_forcing(np.float64, per_member=False), Rain=ens.pinned_forcing(np.float32)["Rain"])
    return ens.pinned_forcing(np.float32 if kind == "float32" else np.float64)


def fill(pinned, rows):
    for k in MU.FORCING:
        assert pinned[k].shape == rows[k].shape and pinned[k].dtype == rows[k].dtype, k
        pinned[k][...] = rows[k]


@pytest.mark.parametrize("feed", ["prefetch", "step"])
@pytest.mark.parametrize("kind", MU.KINDS)
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "one_stream"])
@pytest.mark.parametrize("structures", [False, True], ids=["plain", "structures"])
def test_every_member_as_its_own_hot_path(amd, scenario, monkeypatch, structures, overlap, kind, feed):
    for k in ("LF_FUSED_TIME_MAJOR", "LF_LAND_MEMBERS", "LF_PIXEL_MEMBERS", "LF_SURFACE_MEMBERS", "LF_MEMBERS_MB"):
        monkeypatch.delenv(k, raising=False)
    want = MU.alone(scenario, structures, kind)
    assert not MU.same_bits(want[2][0]["ChanQ"], want[2][1]["ChanQ"]) and not MU.same_bits(want[2][0]["LZ"], want[2][1]["LZ"])
    ens = new_ensemble(scenario, structures, overlap)
    if feed == "prefetch":
        # two page-locked sets, alternating: the next step's set is refilled in place after upload_wait and handed to
        # prefetch while the step just enqueued is still running
        sets = [pinned_set(ens, kind) for _ in range(2)]
        fill(sets[0], MU.ensemble_forcing(kind, 0))
        ens.prefetch(sets[0])
    for s in range(MU.STEPS):
        q = MU.inflow_rows(scenario, structures, s)
        if feed == "prefetch":
            ens.step(sets[s % 2], time_since_start=s + 1, QInM3=q)
            if s + 1 < MU.STEPS:
                ens.upload_wait()
                fill(sets[(s + 1) % 2], MU.ensemble_forcing(kind, s + 1))
                ens.prefetch(sets[(s + 1) % 2])
                for a in sets[s % 2].values():            # (handed over and waited for: the device has its own copy)
                    a[...] = np.nan
        else:
            ens.step(MU.ensemble_forcing(kind, s), time_since_start=s + 1, QInM3=q)
        MU.assert_members(ens, want[s], s)
        assert ens.forcing_member_stride() == ens.pstride == MU.N + MU.PAD
        f = ens.last_forms()
        assert (f["land"], f["pixel_aggregates"], f["overland"]) == (2, 2, 2), f
    MU.assert_gaps(ens)
    ens.free()


def test_a_step_on_the_forcing_of_a_prefetched_step(amd, scenario, monkeypatch):
    """step(None) after a prefetched step is a second step on the same rows -- also with a prefetch pending"""
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    rows, other = MU.ensemble_forcing("float64", 0), MU.ensemble_forcing("float64", 1)
    a, b = new_ensemble(scenario, False), new_ensemble(scenario, False)
    a.prefetch(rows)
    a.step(rows)
    a.prefetch(other)                                     # goes to the set that is not in use and stays pending
    a.step(None)
    b.step(rows)
    b.step(rows)
    second = MU.compared(b)
    for k, x in MU.compared(a).items():
        assert MU.same_bits(x, second[k]), (k, MU.first_difference(x, second[k]))
    assert a.steps_done == b.steps_done == 2
    a.step(other)                                         # the pending prefetch: no second upload, the same result
    b.step({k: x.copy() for k, x in other.items()})
    for k in a.state_names():
        assert MU.same_bits(a.download(k), b.download(k)), k
    MU.assert_gaps(a)
    a.free(); b.free()


def test_a_step_with_other_rows_than_the_prefetched_ones_uses_its_own(amd, scenario, monkeypatch):
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    want = MU.alone(scenario, False, "float64")
    ens = new_ensemble(scenario, False)
    ens.prefetch(MU.ensemble_forcing("float64", 1))       # a: never used
    ens.step(MU.ensemble_forcing("float64", 0), time_since_start=1)
    MU.assert_members(ens, want[0], 0)
    MU.assert_gaps(ens)
    ens.free()


def test_shared_vectors_are_one_row_for_every_member(amd, scenario, monkeypatch):
    """all five vectors [N]: forcing_member_stride() is 0 and every member is member 0's own hot path; a [members, N] vector in
    the next step's set makes it the row stride again, and a step back on [N] vectors 0 -- tracked per set"""
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    want = MU.alone(scenario, False, "float32")
    ens = new_ensemble(scenario, False)
    assert ens.forcing_member_stride() == 0               # (the constructor's forcing is shared)
    ens.step(MU.member_forcing("float32", 0, 0), time_since_start=1)
    assert ens.forcing_member_stride() == 0 == ens.land.forcing_member_stride()
    MU.assert_members(ens, [want[0][0]] * MU.MEMBERS, 0)
    for k in MU.FORCING:                                  # every member's row is written all the same
        rows = ens.download(k)
        assert rows.shape == (MU.MEMBERS, MU.N) and all(MU.same_bits(rows[m], rows[0]) for m in range(MU.MEMBERS)), k
    ens.prefetch(MU.ensemble_forcing("mixed", 1))
    assert ens.forcing_member_stride() == 0               # (the set in use is still the shared one)
    ens.step(None)
    assert ens.forcing_member_stride() == 0
    ens.step(MU.ensemble_forcing("mixed", 1))
    assert ens.forcing_member_stride() == ens.pstride
    ens.step(MU.member_forcing("float64", 0, 2))
    assert ens.forcing_member_stride() == 0
    MU.assert_gaps(ens)
    ens.free()


def test_forcing_of_another_shape_is_refused(amd, scenario):
    ens = new_ensemble(scenario, False)
    rows = MU.ensemble_forcing("float64", 0)
    for bad in (rows["Rain"][:2], rows["Rain"][:, :-1], rows["Rain"][0][:-1], rows["Rain"].T):
        with pytest.raises(ValueError, match="forcing vector Rain"):
            ens.step(dict(rows, Rain=bad))
        with pytest.raises(ValueError, match="forcing vector Rain"):
            ens.prefetch(dict(rows, Rain=bad))
    assert ens.steps_done == 0
    p = ens.pinned_forcing(np.float32, per_member=False)
    assert all(p[k].shape == (MU.N,) and p[k].dtype == np.float32 for k in MU.FORCING)
    ens.free()
