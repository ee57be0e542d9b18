"""HotPathEnsemble.track_begin and what follows from it: every step() folds the tracked rows into accumulators on the device
(lf_members_track_device).  On the framed scenario of test_report_rasters_gpu.py -- sea around the land, a channel domain
smaller than the land, padded member rows -- with trackers on "ChanQAvg" (two threshold maps) and on a land row, after every
step: download() of every derived name is the restatement (members_track.py) folded over chan_q_avg() / download() of the
steps so far; summary(), summary_rasters(), rasters() and sample() on the derived names are what they are on any row with
those values; the elements between the accumulator rows keep their gap values; track_reset() starts over; and a twin
without trackers ends with the same bits in every vector.  Once as built, once with LF_FUSED_TIME_MAJOR=1 and once with
overlap_channel=False."""
import numpy as np
import pytest

import members_products as MP
import members_track as MT
import report_rasters as RR

pytestmark = pytest.mark.gpu

H, W, M, PAD, STEPS = 24, 30, 3, 5, 5
N = H * W
LAND_ROW = "DirectRunoff"
GAP = -1.2345678e300                   # planted between the member rows before the trackers are made
F64_KEYS, I32_KEYS = ("peak", "sum", "period_mean"), ("peak_step", "first_above", "steps_above")


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def cp(d):
    return {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}


def make(overlap_channel=True):
    """the smallest scenario of the ensemble tests, its all-land raster framed by sea: a sea column left and right, a sea
    row above and two below"""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathEnsemble
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    framed = np.zeros((H + 3, W + 2), bool)
    framed[1:H + 1, 1:W + 1] = mask
    ens = HotPathEnsemble(cp(values), sc, framed, ldd_to_chan, ldd_kin, members=M, pad=PAD, overlap_channel=overlap_channel)
    assert ens.Nk < ens.N == N and not framed.all() and ens._outside.size and ens.kstride > ens.Nk and ens.pstride > ens.N
    ens.set_gaps(GAP)
    return ens


def step(ens, s):
    from lisflood_amd import synthetic as syn
    f = [syn.hotpath_forcing(N, s + 10 * m) for m in range(M)]
    ens.step({k: np.stack([x[k] for x in f]) for k in f[0]}, time_since_start=s + 1)


def raster_of(ens, a, dtype, fill=RR.FILL):
    """[..., N] in pixel order -> [..., H, W] of dtype as the host makes it: decompress, astype, the fill off the mask"""
    from lisflood_amd import output
    a = np.asarray(a)
    maps = np.stack([output.decompress(row, ens.land_mask) for row in a.reshape(-1, a.shape[-1])])
    maps = np.where(ens.land_mask, maps.astype(dtype), np.dtype(dtype).type(fill))
    return maps.reshape(a.shape[:-1] + ens.land_mask.shape)


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


def snapshot(ens):
    """every vector that holds member rows, and what lies between the rows"""
    out = {k: ens.download(k) for k in ens.gap_names()}
    out.update({"gaps:" + k: ens.gaps(k) for k in ens.gap_names()})
    out["chan_q_avg"] = ens.chan_q_avg()
    return out


def folded(history, thr):
    """the restatement over the steps so far -> derived key -> [members, N] / [T, members, N]"""
    x = np.stack(history)
    acc = MT.fold(x, thr)
    acc["period_mean"] = acc["sum"] / np.float64(len(history))
    return acc


def check_derived(ens, name, ref, channel, what):
    """download() of every derived name; the int32 rows of a channel row are not tracked outside the channel domain: 0"""
    for key, want in ref.items():
        got = ens.download("%s.%s" % (name, key))
        assert got.dtype == want.dtype and got.shape == want.shape, (what, name, key)
        if key in I32_KEYS and channel:
            assert (got[..., ens._outside] == 0).all(), (what, name, key)
            got, want = got[..., ens.ids], want[..., ens.ids]
        assert MT.same(got, want), (what, name, key)


def check_products(ens, thr, gauges, ref, land_ref, what):
    # summary() on the folded rows is the restatement of the products on those rows
    peak, mean = ref["peak"], ref["period_mean"]
    got = ens.summary("ChanQAvg.peak", thresholds=thr, ranks=(0, 2))
    want = dict(mean=MP.mean_of(peak), min=MP.min_of(peak), max=MP.max_of(peak), exceed=MP.exceed_of(peak, thr),
                order=MP.order_table(peak)[[0, 2]])
    assert sorted(got) == sorted(want)
    for k in want:
        assert MT.same(got[k], want[k]), (what, "peak", k)
    assert (got["exceed"][0, ens._outside[::2]] == M).all()          # 0.0 > -1.0 in every member outside the channel domain
    got = ens.summary("ChanQAvg.period_mean")
    for k, f in (("mean", MP.mean_of), ("min", MP.min_of), ("max", MP.max_of)):
        assert MT.same(got[k], f(mean)), (what, "period_mean", k)
    # summary_rasters() is summary() decompressed
    ref_maps = ens.summary("ChanQAvg.peak", thresholds=thr, ranks=(0, 2))
    maps = ens.summary_rasters("ChanQAvg.peak", thresholds=thr, ranks=(0, 2)).wait()
    assert sorted(maps) == sorted(ref_maps)
    for k in ref_maps:
        want = raster_of(ens, ref_maps[k], np.int32 if k == "exceed" else np.float32)
        assert RR.same_bits(maps[k], want), (what, "summary_rasters", k)
    # rasters() of fp64 and int32 names are the downloads decompressed
    names = ["ChanQAvg.%s" % k for k in F64_KEYS + I32_KEYS] + ["ChanQAvg", LAND_ROW + ".peak", LAND_ROW + ".peak_step", LAND_ROW + ".sum"]
    for dtype in (np.float32, np.float64):
        maps = ens.rasters(names, dtype=dtype).wait()
        assert sorted(maps) == sorted(names)
        for k in names:
            rows = ens.chan_q_avg() if k == "ChanQAvg" else ens.download(k)
            want = raster_of(ens, rows, np.int32 if rows.dtype == np.int32 else dtype)
            assert maps[k].dtype == want.dtype and maps[k].shape == want.shape, (what, k)
            assert RR.same_bits(maps[k], want), (what, "rasters", k)
    assert maps["ChanQAvg.first_above"].shape == (2, M) + ens.land_mask.shape
    assert (maps["ChanQAvg.peak_step"][:, ~ens.land_mask] == int(RR.FILL)).all()
    assert MT.same(ens.download(LAND_ROW + ".peak"), land_ref["peak"])
    # sample() is the download at the gauges (one of them outside the channel domain: 0.0)
    for key in ("peak", "period_mean"):
        assert MT.same(ens.sample("ChanQAvg." + key, gauges), ref[key][:, gauges]), (what, "sample", key)
    assert MT.same(ens.sample(LAND_ROW + ".peak", gauges), land_ref["peak"][:, gauges])


def check_gaps(ens, T):
    from lisflood_amd.hotpath import TRACK_GAP_I32
    assert TRACK_GAP_I32 == -7
    for name, keys, pad in (("ChanQAvg", MT.KEYS, ens.kstride - ens.Nk), (LAND_ROW, MT.KEYS[:3], ens.pstride - ens.N)):
        for key in keys:
            gaps = ens.track_gaps(name, key)
            assert gaps.shape == ((T, M, pad) if key in ("first_above", "steps_above") else (M, pad)) and pad == PAD
            assert (gaps == (GAP if key in ("peak", "sum") else TRACK_GAP_I32)).all(), (name, key)


@pytest.mark.parametrize("variant", ["as_built", "time_major", "one_stream"])
def test_trackers_follow_the_run_and_leave_it_alone(amd, monkeypatch, variant):
    monkeypatch.delenv("LF_FUSED_TIME_MAJOR", raising=False)
    if variant == "time_major":
        monkeypatch.setenv("LF_FUSED_TIME_MAJOR", "1")
    ens, twin = make(variant != "one_stream"), make(variant != "one_stream")
    step(ens, 0)                                                      # the run is under way when the trackers begin
    step(twin, 0)
    thr = thresholds_for(ens, ens.chan_q_avg(), 5)
    gauges = np.array([int(ens.ids[3]), int(ens._outside[0]), int(ens.ids[-1]), int(ens.ids[3])])
    ens.track_begin("ChanQAvg", thresholds=thr)
    ens.track_begin(LAND_ROW)
    assert ens.track_steps("ChanQAvg") == ens.track_steps(LAND_ROW) == 0
    with pytest.raises(RuntimeError, match="no step"):
        ens.download("ChanQAvg.peak")
    with pytest.raises(RuntimeError, match="no step"):
        ens.summary("ChanQAvg.period_mean")
    check_gaps(ens, 2)
    chan, land, moved = [], [], False
    for s in range(1, 1 + STEPS):
        step(ens, s)
        step(twin, s)
        chan.append(ens.chan_q_avg())
        land.append(ens.download(LAND_ROW))
        assert ens.track_steps("ChanQAvg") == ens.track_steps(LAND_ROW) == len(chan)
        ref, land_ref = folded(chan, thr), folded(land, thr[:0])
        check_derived(ens, "ChanQAvg", ref, True, (variant, s))
        check_derived(ens, LAND_ROW, land_ref, False, (variant, s))
        check_products(ens, thr, gauges, ref, land_ref, (variant, s))
        check_gaps(ens, 2)
        moved |= len(chan) > 1 and bool((ref["peak_step"][:, ens.ids] > 0).any()) and bool((ref["steps_above"] > 0).any())
        if s == 3:                                                    # a new horizon: the next update is a first one again
            ens.track_reset("ChanQAvg")
            ens.track_reset(LAND_ROW)
            chan, land = [], []
            assert ens.track_steps("ChanQAvg") == 0
            with pytest.raises(RuntimeError, match="no step"):
                ens.rasters(["ChanQAvg.peak_step"])
    assert moved and len(chan) == 2                                   # (peaks moved and thresholds were crossed: something to see)
    with pytest.raises(ValueError, match="without thresholds"):
        ens.download(LAND_ROW + ".first_above")
    a, b = snapshot(ens), snapshot(twin)
    assert sorted(a) == sorted(b)
    for k in a:                                                       # (byte vectors among them: compared as bytes)
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (variant, k)
    ens.track_end(LAND_ROW)
    with pytest.raises(ValueError, match="neither a channel row"):
        ens.summary(LAND_ROW + ".peak")                               # (the name went with its tracker)
    ens.free(); twin.free()
    assert ens._trackers == {}


def test_the_refusals(amd):
    ens = make()
    with pytest.raises(ValueError, match="neither a channel row"):
        ens.track_begin("NoSuchRow")
    with pytest.raises(ValueError, match="neither a channel row"):
        ens.track_begin("W1a")                                        # a [3, N] member vector is no [N] row
    with pytest.raises(ValueError, match="thresholds must be"):
        ens.track_begin("ChanQ", thresholds=np.zeros((5, N)))
    with pytest.raises(ValueError, match="thresholds must be"):
        ens.track_begin("ChanQ", thresholds=np.zeros(N - 1))
    assert ens._trackers == {}
    for name in ("ChanQAvg", "ChanQ", LAND_ROW, "sumDisDay"):
        ens.track_begin(name, thresholds=np.zeros(N) if name == "ChanQ" else None)
    with pytest.raises(ValueError, match="at most 4"):
        ens.track_begin("ChanQKin")
    with pytest.raises(ValueError, match="tracked already"):
        ens.track_begin("ChanQ")
    with pytest.raises(RuntimeError, match="no step"):
        ens.sample("ChanQ.peak", np.array([0]))
    with pytest.raises(ValueError, match="not tracked"):
        ens.track_steps("ChanQKin")
    step(ens, 0)
    for name in ("summary", "summary_rasters"):
        with pytest.raises(ValueError, match="integer rows"):
            getattr(ens, name)("ChanQ.first_above")
    with pytest.raises(ValueError, match="integer rows"):
        ens.sample("ChanQAvg.peak_step", np.array([0]))
    with pytest.raises(ValueError, match="without thresholds"):
        ens.rasters(["ChanQAvg.steps_above"])
    with pytest.raises(ValueError, match="no accumulator"):
        ens.track_gaps("ChanQAvg", "first_above")
    assert ens.download("ChanQ.steps_above").shape == (1, M, N) and ens.download("sumDisDay.peak_step").dtype == np.int32
    ens.track_end("sumDisDay")
    with pytest.raises(ValueError, match="neither a channel row"):
        ens.track_begin("ChanQ.peak")                                 # (an accumulator is no source of another tracker)
    ens.track_begin("ChanQKin")                                       # (there is room again)
    ens.free()
