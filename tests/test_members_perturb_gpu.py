"""lf_members_perturb_device and lf_upload_perturb_rows on the device against their restatement (members_perturb.py) on the
uint64 view, every NaN as one pattern: every size around a wavefront and a workgroup, member counts on both sides of the rows
staged at once (16), every rank edge, additive and multiplicative, the three base forms, each bound absent, a scalar and a
row, plain and padded strides with a sentinel between the rows that must keep its bits.  Then the upload form inside an
upload section behind lf_upload_rows, and hotpath.HotPathEnsemble -- forcing_perturbation() with step / prefetch
coefficients and perturb() -- against a twin that is fed rows made on the host by the restatement."""
import ctypes as C
import itertools

import numpy as np
import pytest

import hotpath_members as HM
import members_perturb as MP
import members_upload as MU

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
MEMBERS = (1, 2, 7, 8, 9, 15, 16, 17, 51, 128)           # 15, 16, 17: both sides of the rows staged at once (kStage)
RANKS = (1, 2, 3, 8, 15, 16)
BOUNDS = ("absent", "scalar", "row")
OPTIONS = list(itertools.product((False, True), MP.BASE_FORMS, BOUNDS, BOUNDS))      # mode, base, lower, upper: 54
PADS = ((0, 0), (5, 0), (0, 3), (5, 3))                  # of stride and pattern_stride


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def up(amd, a):
    return None if a is None else amd.DeviceArray.from_host(np.ascontiguousarray(a, np.float64))


def run_perturb(amd, x, stride, coeff, P, pstride, form, base_row, multiplicative, lower, upper, times=1):
    """the call on x [members, n] laid out with `stride`, the patterns with `pstride`
    -> (rows after it, what lies between them, the pattern image after it)"""
    members, n = x.shape
    rank = P.shape[0]
    d_rows, d_p, d_b = up(amd, MP.layout(x, stride)), up(amd, MP.layout(P, pstride)), up(amd, base_row)
    d_lo, d_hi = up(amd, lower[1]), up(amd, upper[1])
    p = lambda d: None if d is None else d.ptr
    base = d_rows.ptr if form == "alias" else p(d_b)
    c = np.ascontiguousarray(coeff, np.float64)
    for _ in range(times):
        amd.check(amd.lib().lf_members_perturb_device(0, d_rows.ptr, members, stride, n, base, rank, d_p.ptr, pstride,
                                                      amd.ptr(c), int(multiplicative), p(d_lo), lower[2], p(d_hi), upper[2]))
    image = d_rows.download().reshape(members, stride)
    patterns = d_p.download()
    for d in (d_rows, d_p, d_b, d_lo, d_hi):
        if d is not None:
            d.free()
    return image[:, :n], image[:, n:], patterns


def untouched(gaps):
    return np.array_equal(MP.bits(gaps), MP.bits(np.full(gaps.shape, MP.SENTINEL)))


@pytest.mark.parametrize("members", MEMBERS)
def test_perturb_against_the_restatement(amd, members):
    seen, count = set(), 7 * MEMBERS.index(members)
    for n, rank, (pad, ppad) in itertools.product(SIZES, RANKS, PADS):
        option = OPTIONS[count % len(OPTIONS)]
        count += 1
        seen.add(option)
        multiplicative, form, lower, upper = option
        x = MP.make_rows(n, members, 100 * members + n)
        c, P = MP.make_coefficients(members, rank, members + rank), MP.make_patterns(rank, n, n + rank)
        base, base_row = MP.base_of(form, x, n, n + 4)
        lo, hi = MP.bound_of(lower, n, n + 2, True), MP.bound_of(upper, n, n + 3, False)
        got, gaps, patterns = run_perturb(amd, x, n + pad, c, P, n + ppad, form, base_row, multiplicative, (lower,) + lo[1:],
                                          (upper,) + hi[1:])
        want = MP.perturb(x, c, P, base, multiplicative, lo[0], hi[0])
        what = (members, n, rank, pad, ppad, option)
        bad = np.argwhere(MP.canonical(got) != MP.canonical(want))
        assert bad.size == 0, (what, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        assert untouched(gaps), what
        assert np.array_equal(MP.bits(patterns), MP.bits(MP.layout(P, n + ppad))), what
    assert seen == set(OPTIONS)                      # every combination of mode, base form and bounds came up for this member count


@pytest.mark.parametrize("members,n,rank", [(1, 65, 1), (7, 257, 3), (17, 64, 16), (51, 1000, 8)])
def test_the_stated_consequences_on_the_device(amd, members, n, rank):
    """zero coefficients under `multiplicative` keep every non-NaN bit, -0.0 included, in both base forms; in additive mode
    -0.0 becomes +0.0; a zero coefficient does not switch an infinite pattern value off; infinite scalar bounds take nothing"""
    x = MP.make_rows(n, members, 5)
    finite = np.abs(np.random.default_rng(3).standard_normal((rank, n))) + 0.1
    zero = np.zeros((members, rank))
    absent = ("absent", None, -np.inf), ("absent", None, np.inf)
    got, gaps, _ = run_perturb(amd, x, n + 5, zero, finite, n, "absent", None, True, *absent)
    keep = ~np.isnan(x)
    assert np.array_equal(MP.bits(got)[keep], MP.bits(x)[keep]) and np.isnan(got[~keep]).all() and untouched(gaps)
    assert np.signbit(got[0, 0]) and got[0, 0] == 0
    got, _, _ = run_perturb(amd, x, n + 5, zero, finite, n, "alias", None, True, *absent)
    keep = ~np.isnan(x[0])
    assert np.array_equal(MP.bits(got)[:, keep], MP.bits(np.broadcast_to(x[0], x.shape))[:, keep])
    got, _, _ = run_perturb(amd, x, n, zero, finite, n, "absent", None, False, *absent)
    assert MP.same(got, MP.perturb(x, zero, finite)) and got[0, 0] == 0 and not np.signbit(got[0, 0])
    if n > 40:
        P = MP.make_patterns(rank, n, 9)
        got, _, _ = run_perturb(amd, x, n, zero, P, n, "absent", None, True, *absent)
        assert MP.same(got, MP.perturb(x, zero, P, None, True)) and np.isnan(got[:, np.isinf(P).any(axis=0)]).all()


@pytest.mark.parametrize("members,n", [(2, 63), (17, 256), (51, 257)])
def test_twice_is_the_restatement_twice(amd, members, n):
    x, c, P = MP.make_rows(n, members, 8), MP.make_coefficients(members, 3, 4), MP.make_patterns(3, n, 6)
    lo, hi = MP.bound_of("row", n, 1, True), MP.bound_of("scalar", n, 2, False)
    got, gaps, _ = run_perturb(amd, x, n + 5, c, P, n + 3, "absent", None, True, ("row",) + lo[1:], ("scalar",) + hi[1:], times=2)
    once = MP.perturb(x, c, P, None, True, lo[0], hi[0])
    want = MP.perturb(once, c, P, None, True, lo[0], hi[0])
    assert MP.same(got, want) and untouched(gaps) and not MP.same(once, want)


def test_one_member_and_rank_one_need_no_stride(amd):
    """members == 1 with stride 0 and rank == 1 with pattern_stride 0 are legal: neither stride is used"""
    n = 300
    x, c, P = MP.make_rows(n, 1, 2), np.array([[0.75]]), MP.make_patterns(1, n, 3)
    d_rows, d_p = up(amd, x[0]), up(amd, P[0])
    amd.check(amd.lib().lf_members_perturb_device(0, d_rows.ptr, 1, 0, n, None, 1, d_p.ptr, 0, amd.ptr(c), 0, None, -np.inf, None,
                                                  np.inf))
    assert MP.same(d_rows.download()[None, :], MP.perturb(x, c, P))
    d_rows.free(); d_p.free()


def test_the_coefficient_tables_come_back_after_a_trim(amd):
    """lf_device_trim releases the four tables on the device; the next call makes them again.  Six calls in a row with a table
    each go round the ring of four."""
    n, members, rank = 257, 7, 3
    x, P = MP.make_rows(n, members, 1), MP.make_patterns(rank, n, 2)
    absent = ("absent", None, -np.inf), ("absent", None, np.inf)
    for round_ in range(2):
        for k in range(6):
            c = MP.make_coefficients(members, rank, 10 * round_ + k)
            got, _, _ = run_perturb(amd, x, n, c, P, n, "absent", None, False, *absent)
            assert MP.same(got, MP.perturb(x, c, P)), (round_, k)
        amd.check(amd.lib().lf_device_trim(0))


# ---- lf_upload_perturb_rows ------------------------------------------------------------------------------------------------------
def upload_perturbed(amd, dst, stride, members, src, n, d_index, d_patterns, rank, coeff, multiplicative, lower, upper, buffer_set,
                     scribble=True):
    """lf_upload_rows and lf_upload_perturb_rows behind it, as HotPathEnsemble._upload issues them: a one-row source goes into
    member 0's row and is spread from there (base_dev = rows_dev), member rows are perturbed in place.  The coefficient array
    is overwritten as soon as the call has returned."""
    L = amd.lib()
    one = src.shape[0] == 1
    c = np.array(coeff, np.float64)
    amd.check(L.lf_upload_begin(0, buffer_set))
    amd.check(L.lf_upload_rows(0, dst.ptr, stride, 1 if one else members, src.ctypes.data_as(C.c_void_p), src.shape[0],
                               1 if src.dtype == np.float32 else 0, n, d_index.ptr))
    amd.check(L.lf_upload_perturb_rows(0, dst.ptr, members, stride, n, dst.ptr if one else None, rank, d_patterns.ptr, n,
                                       amd.ptr(c), int(multiplicative), None, lower, None, upper))
    if scribble:
        c[...] = 1e30
    amd.check(L.lf_upload_end(0, buffer_set))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("src_rows", ["one", "members"])
def test_upload_perturb_rows_behind_upload_rows(amd, dtype, src_rows):
    """both buffer sets alternating, two destinations, no host wait between the calls: the copy stream orders the
    coefficient tables, the coefficient array belongs to the caller again on return"""
    L = amd.lib()
    members, n, rank, stride = 9, 1000, 5, 1007
    rng = np.random.default_rng(17 + (dtype is np.float32))
    perm = rng.permutation(n).astype(np.int32)
    d_perm = amd.DeviceArray.from_host(perm)
    P = MP.make_patterns(rank, n, 4)
    d_p = amd.DeviceArray.from_host(P.reshape(-1))
    dst = [amd.DeviceArray.from_host(np.full(members * stride, MP.SENTINEL)) for _ in range(2)]
    jobs = []
    for k in range(6):
        src = MU.source(rng, 1 if src_rows == "one" else members, n, dtype)
        c = MP.make_coefficients(members, rank, 30 + k)
        multiplicative, lower, upper = bool(k % 2), (-np.inf, 0.0, -1.5)[k % 3], (np.inf, 4.0)[k % 2]
        upload_perturbed(amd, dst[k % 2], stride, members, src, n, d_perm, d_p, rank, c, multiplicative, lower, upper, k % 2)
        up_rows = np.array(MU.reference(src, members, perm))
        want = MP.perturb(up_rows, c, P, up_rows[0] if src_rows == "one" else None, multiplicative, lower, upper)
        jobs.append((k % 2, src, want))
    for b in (0, 1):
        amd.check(L.lf_upload_wait(0, b))
    for d in (0, 1):                                      # what the last call into each destination left
        want = [j for j in jobs if j[0] == d][-1][2]
        got = dst[d].download().reshape(members, stride)
        bad = np.argwhere(MP.canonical(got[:, :n]) != MP.canonical(want))
        assert bad.size == 0, (d, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        assert untouched(got[:, n:])
    for d in dst + [d_perm, d_p]:
        d.free()


def test_upload_perturb_rows_outside_an_upload_section_is_refused(amd):
    L = amd.lib()
    n = 64
    rows, P, c = up(amd, np.zeros(n)), up(amd, np.ones(n)), np.ones((1, 1))
    amd.check(L.lf_upload_begin(0, 0))
    amd.check(L.lf_upload_end(0, 0))
    rc = L.lf_upload_perturb_rows(0, rows.ptr, 1, n, n, None, 1, P.ptr, n, amd.ptr(c), 0, None, -np.inf, None, np.inf)
    assert rc == amd.LF_E_INVALID and b"lf_upload_begin" in L.lf_last_error()
    assert not rows.download().any()
    amd.check(L.lf_upload_begin(0, 1))
    amd.check(L.lf_upload_perturb_rows(0, rows.ptr, 1, n, n, None, 1, P.ptr, n, amd.ptr(c), 0, None, -np.inf, None, np.inf))
    amd.check(L.lf_upload_end(0, 1))
    amd.check(L.lf_upload_wait(0, 1))
    assert (rows.download() == 1.0).all()
    rows.free(); P.free()


# ---- HotPathEnsemble ---------------------------------------------------------------------------------------------------------
H, W, PAD, RANK = 24, 30, 5, 4
N = H * W


def cp(d):
    return {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}


def make(members, with_structures=False, shape=(H, W)):
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathEnsemble
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(*shape)
    st = None
    if with_structures:
        st, ldd_kin = syn.structures_scenario(ldd_kin, shape, values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5, seed=MU.PLANNED)
    ens = HotPathEnsemble(cp(values), sc, mask, ldd_to_chan, ldd_kin, members=members, structures=cp(st) if st else None, pad=PAD)
    ens.set_gaps(HM.SENTINEL)
    return ens, st, mask


def patterns_of(mask, seed, rank=RANK):
    from lisflood_amd import assimilation as AS
    return AS.fourier_patterns(mask, rank, 6.0, np.random.default_rng(seed))


def coefficients_of(members, seed, sigma=0.3, rank=RANK):
    from lisflood_amd import assimilation as AS
    return AS.ar1_coefficients(None, (members, rank), sigma, np.random.default_rng(seed))


def state_of(ens):
    out = {k: ens.download(k) for k in ens.state_names()}
    out["ChanQAvg"] = ens.chan_q_avg()
    return out


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        bad = np.argwhere(MP.bits(a[k]) != MP.bits(b[k]))
        assert bad.size == 0, (what, k, len(bad), bad[:3], a[k][tuple(bad[0])], b[k][tuple(bad[0])])


def host_rows(forcing, members, perturbed):
    """the forcing a twin without perturbations is fed: [members, N] float64 rows made by the restatement for the names in
    `perturbed` (name -> (coefficients, patterns, multiplicative, lower, upper)), everything else as it is"""
    out = dict(forcing)
    for k, (c, P, multiplicative, lower, upper) in perturbed.items():
        f = np.asarray(forcing[k]).astype(np.float64)
        out[k] = MP.perturb(f if f.ndim == 2 else None, c, P, f if f.ndim == 1 else None, multiplicative, lower, upper)
    return out


@pytest.mark.parametrize("members", [3, 5])
def test_perturbed_forcing_is_the_host_made_rows(amd, members):
    """Rain multiplicative and ETRef additive over three steps: one through step(), one through prefetch() and step(), one
    step(None); the twin is fed [members, N] rows made on the host by the restatement"""
    from lisflood_amd import synthetic as syn
    (A, _, mask), (B, _, _) = make(members), make(members)
    P_rain, P_et = patterns_of(mask, 1), patterns_of(mask, 2, rank=2)
    A.forcing_perturbation("Rain", P_rain)
    A.forcing_perturbation("ETRef", P_et, multiplicative=False, lower=0.5, upper=3.5)
    regs = lambda c: {"Rain": (c["Rain"], P_rain, True, 0.0, np.inf), "ETRef": (c["ETRef"], P_et, False, 0.5, 3.5)}
    # step 1: [N] float64 vectors, coefficients through step()
    f = syn.hotpath_forcing(N, 0)
    c = {"Rain": coefficients_of(members, 11), "ETRef": coefficients_of(members, 12, 1.0, 2)}
    A.step(f, time_since_start=1, coefficients=c)
    B.step(host_rows(f, members, regs(c)), time_since_start=1)
    assert A.forcing_member_stride() != 0
    assert_same(state_of(A), state_of(B), "step 1")
    # step 2: Rain as [members, N] float32 rows (perturbed in place), ETRef [N]; through prefetch(), which carries the coefficients
    f = syn.hotpath_forcing(N, 1)
    f["Rain"] = np.stack([syn.hotpath_forcing(N, 1 + 10 * m)["Rain"] for m in range(members)]).astype(np.float32)
    c = {"Rain": coefficients_of(members, 13), "ETRef": coefficients_of(members, 14, 1.0, 2)}
    A.prefetch(f, coefficients=c)
    held = cp(c)
    for a in c.values():
        a[...] = 1e30                                               # (the tables were read before prefetch returned)
    A.step(f, time_since_start=2)
    B.step(host_rows(f, members, regs(held)), time_since_start=2)
    assert A.forcing_member_stride() != 0
    assert_same(state_of(A), state_of(B), "step 2")
    rain = A.download("Rain")
    assert rain.shape == (members, N) and (rain >= 0).all() and not np.array_equal(rain[0], rain[1])
    et = A.download("ETRef")
    assert et.min() == 0.5 and et.max() == 3.5 and ((et > 0.5) & (et < 3.5)).any()          # both bounds bite
    # step 3: the rows on the device once more
    A.step(None, time_since_start=3)
    B.step(None, time_since_start=3)
    assert_same(state_of(A), state_of(B), "step 3")
    for k in MU.FORCING:                                          # nothing was written between the rows of either set
        for b in (0, 1):
            assert (A.gaps(k, buffer_set=b) == HM.SENTINEL).all(), (k, b)
    # a vector without coefficients behaves as ever; a registration removed is gone
    f = syn.hotpath_forcing(N, 2)
    A.forcing_perturbation("ETRef", None)
    A.step(f, time_since_start=4, coefficients={"Rain": held["Rain"]})
    B.step(host_rows(f, members, {"Rain": regs(held)["Rain"]}), time_since_start=4)
    assert_same(state_of(A), state_of(B), "step 4")
    with pytest.raises(ValueError, match="no forcing_perturbation"):
        A.step(f, coefficients={"ETRef": held["ETRef"]})
    A.step(f, time_since_start=5)
    assert all(A._shared[A._cur][k] for k in MU.FORCING)          # one row for every member again
    A.free(); B.free()


def is_site(name):
    from lisflood_amd import routing as RT
    return name in RT._LAKE_STATE + RT._RES_STATE


def host_perturb(ens, st, c, P, names, multiplicative, bounds):
    """the route perturb() replaces: download, the restatement, set_member_state -- once per vector.  A channel vector is
    perturbed on the pixels of the channel domain (the others are not on the device), a site row at the site's pixel."""
    from lisflood_amd import routing as RT
    for name in names:
        lower, upper = bounds.get(name, (None, None))
        if is_site(name):
            pix = np.asarray(st["LakeIndex" if name in RT._LAKE_STATE else "ReservoirIndex"], np.int64)
            x = ens.download_site(name)
        elif name in RT._STATE:
            pix = ens.gpix
            x = ens.download(name)[:, pix]
        else:
            pix = np.arange(ens.N)
            x = ens.download(name)
        pick = lambda b, inf: inf if b is None else b if np.ndim(b) == 0 else np.asarray(b)[..., pix]
        lo, hi = pick(lower, -np.inf), pick(upper, np.inf)
        if x.ndim == 3:                                             # [members, 3, N]: the same patterns in each of the three rows
            row = lambda b, v: b if np.ndim(b) < 2 else b[v]
            new = np.stack([MP.perturb(x[:, v], c, P[:, pix], None, multiplicative, row(lo, v), row(hi, v)) for v in range(3)],
                           axis=1)
        else:
            new = MP.perturb(x, c, P[:, pix], None, multiplicative, lo, hi)
        if is_site(name):
            ens._set_channel_rows(name, new)
        elif name in RT._STATE:
            full = ens.download(name)
            full[:, pix] = new
            ens.set_member_state(name, full)
        else:
            ens.set_member_state(name, new)


@pytest.mark.parametrize("with_structures", [False, True], ids=["plain", "structures"])
def test_perturb_is_the_host_route(amd, with_structures):
    from lisflood_amd import synthetic as syn
    members = 3
    shape = (MU.H, MU.W) if with_structures else (H, W)
    (A, st, mask), (B, _, _) = make(members, with_structures, shape), make(members, with_structures, shape)
    n = A.N
    inflow = (lambda s: st["QInM3Old"] * (1.0 + 0.1 * s)) if with_structures else (lambda s: None)
    for ens in (A, B):
        ens.step(syn.hotpath_forcing(n, 0), time_since_start=1, QInM3=inflow(0))
    P, c = patterns_of(mask, 5), coefficients_of(members, 6, 0.2)
    names = ["LZ", "W1a", "ChanQ"] + (["LakeStorageM3CC"] if with_structures else [])
    assert "LZ" not in A.land._member and "W1a" in A.land._member and [r[3] for r in A._analysis_rows("ChanQ")] == ["channel"]
    bounds = {"LZ": (0.0, A.download("LZ").mean(axis=0)), "W1a": (np.zeros((3, n)), None), "ChanQ": (0.0, None)}
    gaps = {k: A.gaps(k) for k in A.gap_names()}
    fetch = lambda ens, k: ens.download_site(k) if is_site(k) or k == "TransCum" else ens.download(k)
    everything = lambda ens: dict(state_of(ens), **{k: fetch(ens, k) for k in ens.analysis_names()})
    before = {k: fetch(A, k) for k in A.analysis_names()}
    A.perturb(c, P, names, multiplicative=True, bounds=bounds)
    host_perturb(B, st, c, P, names, True, bounds)
    assert_same(everything(A), everything(B), "after perturb")
    after = {k: fetch(A, k) for k in A.analysis_names()}
    for k in A.analysis_names():                                    # the names of the call moved, the others kept their bits
        assert (k in names) == (not MP.same(before[k], after[k])), k
    assert (after["LZ"] <= bounds["LZ"][1]).all() and not (before["LZ"] <= bounds["LZ"][1]).all()
    # additive, on one vector, through the same pattern rows (nothing goes to the device twice)
    on_device = lambda: {key: hit[1].ptr.value for key, hit in A._analysis_cache.items() if key[0] == id(P)}
    held = on_device()
    assert {key[1:] for key in held} == {(r[3], "all") for k in names for r in A._analysis_rows(k)}    # one row set per order
    A.perturb(c, P, "LZ", bounds={"LZ": (0.0, None)})
    host_perturb(B, st, c, P, ["LZ"], False, {"LZ": (0.0, None)})
    assert on_device() == held and A._analysis_pinned == set()
    assert_same(everything(A), everything(B), "after the additive perturb")
    for k, g in gaps.items():
        assert np.array_equal(MP.bits(A.gaps(k)), MP.bits(g)), k
    for ens in (A, B):
        ens.step(syn.hotpath_forcing(n, 1), time_since_start=2, QInM3=inflow(1))
    assert_same(everything(A), everything(B), "the step behind it")
    A.free(); B.free()


def test_perturbed_forcing_keeps_resampled_particles_apart(amd):
    from lisflood_amd import synthetic as syn
    members = 3
    (U, _, mask), (V, _, _) = make(members), make(members)
    P = patterns_of(mask, 7)
    V.forcing_perturbation("Rain", P)
    V.forcing_perturbation("ETRef", P)
    for ens in (U, V):
        f = [syn.hotpath_forcing(N, 10 * m) for m in range(members)]
        ens.step({k: np.stack([x[k] for x in f]) for k in f[0]}, time_since_start=1)
        ens.resample([0, 0, 0])
    for s in (1, 2):
        c = coefficients_of(members, 20 + s, 0.5)
        c[0] = 0.0                                                  # member 0: no perturbation at all
        U.step(syn.hotpath_forcing(N, s), time_since_start=s + 1)
        V.step(syn.hotpath_forcing(N, s), time_since_start=s + 1, coefficients={"Rain": c, "ETRef": c})
    u, v = state_of(U), state_of(V)
    for k, a in u.items():                                          # shared forcing: the copies stay copies for ever
        for m in (1, 2):
            assert np.array_equal(MP.bits(a[m]), MP.bits(a[0])), (k, m)
    q = v["ChanQAvg"]
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(q[i], q[j]), (i, j)
    for k in u:                                                     # zero coefficients under `multiplicative`: the unperturbed run
        assert np.array_equal(MP.bits(v[k][0]), MP.bits(u[k][0])), k
    U.free(); V.free()


def test_the_refusals(amd):
    from lisflood_amd import synthetic as syn
    members = 3
    ens, _, mask = make(members)
    P, f = patterns_of(mask, 1), syn.hotpath_forcing(N, 0)
    c = coefficients_of(members, 2)
    good = {"Rain": c}
    before = state_of(ens)
    refused = [
        (lambda: ens.forcing_perturbation("ChanQ", P), "no forcing vector"),
        (lambda: ens.forcing_perturbation("Rain", P[:, :-1]), "patterns must be"),
        (lambda: ens.forcing_perturbation("Rain", P[0]), "patterns must be"),
        (lambda: ens.forcing_perturbation("Rain", np.zeros((17, N))), "patterns must be"),
        (lambda: ens.forcing_perturbation("Rain", P, lower=2.0, upper=1.0), "greater than upper"),
        (lambda: ens.step(f, coefficients=good), "no forcing_perturbation"),
    ]
    for call, word in refused:
        with pytest.raises(ValueError, match=word):
            call()
    ens.forcing_perturbation("Rain", P)
    other = {"Rain": c.copy()}
    ens.prefetch(f, coefficients=good)
    refused = [
        (lambda: ens.step(None, coefficients=good), "without forcing"),
        (lambda: ens.prefetch(None, coefficients=good), "without forcing"),
        (lambda: ens.step(f, coefficients=other), "prefetched with other coefficients"),
        (lambda: ens.step(dict(f), coefficients={"ETRef": c}), "no forcing_perturbation"),
        (lambda: ens.step(dict(f), coefficients={"Rain": c[:2]}), "coefficients\\[Rain\\] must be"),
        (lambda: ens.step(dict(f), coefficients={"Rain": c[:, :2]}), "coefficients\\[Rain\\] must be"),
        (lambda: ens.step(dict(f), coefficients=[c]), "must be a dict"),
        (lambda: ens.perturb(c, P, None), "names is required"),
        (lambda: ens.perturb(c, P, ["Rain"]), "no state vector"),
        (lambda: ens.perturb(c, P, ["LZ", "LZ"]), "twice"),
        (lambda: ens.perturb(c[:2], P, ["LZ"]), "coefficients must be"),
        (lambda: ens.perturb(c, P[:, :-1], ["LZ"]), "patterns must be"),
        (lambda: ens.perturb(c, P.astype(np.float32), ["LZ"]), "patterns must be"),
        (lambda: ens.perturb(c, P, ["LZ"], bounds={"UZ": (0.0, None)}), "not among the names"),
        (lambda: ens.perturb(c, P, ["LZ"], bounds={"LZ": (2.0, 1.0)}), "greater than upper"),
    ]
    for call, word in refused:
        with pytest.raises(ValueError, match=word):
            call()
    assert ens._analysis_cache == {} and ens.steps_done == 0         # refused before anything went to the device
    assert_same(state_of(ens), before, "after the refusals")
    ens.step(f, coefficients=good)                                  # the prefetch is still good: None or the same dict
    assert ens.steps_done == 1 and ens.forcing_member_stride() != 0
    ens.free()
