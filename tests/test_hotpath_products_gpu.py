"""HotPathEnsemble.summary() and sample(): the products over the members made on the device against the restatement
(members_products.py) applied to what download() brings to the host -- bit for bit, on the compact channel domain of a run
with structures (pixels outside the domain included) and on the plain one, behind the channel loop on the side stream.
The threshold maps go up once per array object, the member rows and their gaps stay as they are, and a gauge row goes through
output.TssWriter.append."""
import numpy as np
import pytest

import hotpath_members as HM
import members_products as MP
from module_edges import first_difference, same_bits

pytestmark = pytest.mark.gpu

H, W, M, STEPS, PAD = 70, 90, 3, 2, 5
N = H * W
SEED = 23                  # of structures_scenario(n_lakes=3, n_res=5), as tests/test_hotpath_members_gpu.py draws it
LAND_ROW = "DirectRunoff"


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def cp(d):
    return {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}


def member_forcing(m, s):
    from lisflood_amd import synthetic as syn
    return syn.hotpath_forcing(N, s + 10 * m)


# structures=, compact=: the channel domain is every land pixel (plain), or leaves out the pixels whose sub-step is the
# identity -- which this scenario has with and without structures
VARIANTS = {"plain": (False, False), "compact": (False, True), "structures": (True, True)}


@pytest.fixture(scope="module", params=list(VARIANTS))
def ensemble(request, amd):
    """two steps of three members with their own forcing; sentinels between the rows"""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathEnsemble
    with_structures, compact = VARIANTS[request.param]
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    st = None
    if with_structures:
        st, ldd_kin = syn.structures_scenario(ldd_kin, (H, W), values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5, seed=SEED)
    ens = HotPathEnsemble(cp(values), sc, mask, ldd_to_chan, ldd_kin, members=M, structures=cp(st) if st else None,
                          compact=compact, pad=PAD)
    ens.set_gaps(HM.SENTINEL)
    for s in range(STEPS):
        f = [member_forcing(m, s) for m in range(M)]
        q = np.stack([st["QInM3Old"] * (1.0 + 0.1 * s + 0.05 * m) for m in range(M)]) if st else None
        ens.step({k: np.stack([x[k] for x in f]) for k in f[0]}, time_since_start=s + 1, QInM3=q)
    assert (ens.Nk < ens.N) == compact                      # the compact domain leaves pixels out, the plain one none
    yield ens
    ens.free()


def host_rows(ens, name):
    """[members, N] in pixel order, as the host has had to fetch it so far"""
    return ens.chan_q_avg() if name == "ChanQAvg" else ens.download(name)


def thresholds_for(x, seed):
    """three maps in pixel order around the members' values, with a NaN, an exact hit and +-0.0 among them"""
    rng = np.random.default_rng(seed)
    thr = np.stack([np.median(x, axis=0), x.min(axis=0) - 1e-9, x.max(axis=0)]) * rng.choice([0.5, 1.0, 1.5], (3, x.shape[1]))
    thr[0, ::97] = np.nan
    thr[1, 5::89] = 0.0
    thr[2, 7::83] = -0.0
    thr[1, 11::79] = -1.0
    return thr


@pytest.mark.parametrize("name", ["ChanQAvg", "ChanQ", LAND_ROW])
def test_summary_is_the_restatement_of_the_download(ensemble, name):
    ens = ensemble
    x = host_rows(ens, name)
    assert x.shape == (M, N) and not same_bits(x[0], x[1]) and np.abs(x).max() > 0
    thr = thresholds_for(x, 5)
    ranks = (0, M // 2, M - 1)
    got = ens.summary(name, thresholds=thr, ranks=ranks)
    want = dict(mean=MP.mean_of(x), min=MP.min_of(x), max=MP.max_of(x), exceed=MP.exceed_of(x, thr),
                order=MP.order_table(x)[list(ranks)])
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, got[k].dtype)
        if k == "exceed":
            assert np.array_equal(got[k], want[k]), (name, k, np.flatnonzero((got[k] != want[k]).any(axis=0))[:5])
        else:
            assert same_bits(got[k], want[k]), (name, k, first_difference(got[k], want[k]))
    if name != LAND_ROW and ens._outside.size:       # outside the channel domain every member is 0.0 ...
        out = ens._outside
        assert (x[:, out] == 0).all() and (got["mean"][out] == 0).all() and (got["order"][:, out] == 0).all()
        assert ((got["exceed"][:, out] == M) == (thr[:, out] < 0)).all() and (got["exceed"][1, out] == M).any()   # ... M x (0 > threshold)
    # parts of it, alone
    some = ens.summary(name, mean=False, maximum=False)
    assert sorted(some) == ["min"] and same_bits(some["min"], want["min"])
    some = ens.summary(name, mean=False, minimum=False, maximum=False, thresholds=thr[1])
    assert sorted(some) == ["exceed"] and np.array_equal(some["exceed"], want["exceed"][1:2])
    some = ens.summary(name, mean=False, minimum=False, maximum=False, ranks=[1])
    assert sorted(some) == ["order"] and same_bits(some["order"], want["order"][1:2])


def test_what_summary_refuses(ensemble):
    ens = ensemble
    for name in ("ChanLength", "W1a", "Rain", "no_such_vector"):
        with pytest.raises(ValueError, match="neither a channel row"):
            ens.summary(name)
        with pytest.raises(ValueError, match="neither a channel row"):
            ens.sample(name, np.arange(3))
    with pytest.raises(ValueError, match="nothing requested"):
        ens.summary("ChanQ", mean=False, minimum=False, maximum=False)
    with pytest.raises(ValueError, match="ranks"):
        ens.summary("ChanQ", ranks=(0, M))
    with pytest.raises(ValueError, match="thresholds"):
        ens.summary("ChanQ", thresholds=np.zeros((5, N)))
    with pytest.raises(ValueError, match="thresholds"):
        ens.summary("ChanQ", thresholds=np.zeros(N - 1))
    with pytest.raises(ValueError, match="pixels"):
        ens.sample("ChanQ", np.array([0, N]))


def gauges(ens):
    """compressed land indices inside and, where there are any, outside the channel domain; one of them twice"""
    rng = np.random.default_rng(11)
    pix = list(rng.choice(ens.ids, 40, replace=False))
    if ens._outside.size:
        pix += list(rng.choice(ens._outside, 7, replace=False))
    pix.append(pix[0])
    return rng.permutation(np.array(pix, np.int64))


@pytest.mark.parametrize("name", ["ChanQAvg", "ChanQ", "sumDisDay", LAND_ROW])
def test_sample_is_the_download_at_the_gauges(ensemble, name):
    ens = ensemble
    pix = gauges(ens)
    got = ens.sample(name, pix)
    want = host_rows(ens, name)[:, pix]
    assert got.shape == (M, pix.size) and same_bits(got, want), first_difference(got, want)
    assert np.abs(want).max() > 0
    if name != LAND_ROW and ens._outside.size:
        assert (got[:, np.isin(pix, ens._outside)] == 0).all() and np.isin(pix, ens._outside).sum() == 7
    assert same_bits(ens.sample(name, pix), want)                           # the cached table
    assert ens.sample(name, np.zeros(0, np.int64)).shape == (M, 0)
    assert same_bits(ens.sample(name, pix[:1]), want[:, :1])


def test_thresholds_and_gauge_tables_go_up_once(ensemble, monkeypatch):
    from lisflood_amd.hotpath import HotPathEnsemble
    ens = ensemble
    calls = {"thresholds": 0, "gauges": 0}

    def counted(what, inner):
        def f(self, *a, **kw):
            calls[what] += 1
            return inner(self, *a, **kw)
        return f
    monkeypatch.setattr(HotPathEnsemble, "_upload_thresholds", counted("thresholds", HotPathEnsemble._upload_thresholds))
    monkeypatch.setattr(HotPathEnsemble, "_gauge_table", counted("gauges", HotPathEnsemble._gauge_table))
    thr = thresholds_for(ens.chan_q_avg(), 9)
    first = ens.summary("ChanQAvg", thresholds=thr)
    assert calls["thresholds"] == 1
    keep = thr.copy()
    thr[:] = np.nan                                   # the call must not look at the host array again
    again = ens.summary("ChanQAvg", thresholds=thr)
    assert calls["thresholds"] == 1 and np.array_equal(first["exceed"], again["exceed"]) and first["exceed"].max() > 0
    ens.summary("ChanQ", thresholds=thr)              # another channel row: the same rows on the device
    assert calls["thresholds"] == 1
    ens.summary(LAND_ROW, thresholds=thr)             # a land row: the same maps in the other order
    assert calls["thresholds"] == 2
    fresh = ens.summary("ChanQAvg", thresholds=keep)  # another array object
    assert calls["thresholds"] == 3 and np.array_equal(first["exceed"], fresh["exceed"])
    pix = gauges(ens)
    a = ens.sample("ChanQAvg", pix)
    b = ens.sample("ChanQ", pix)
    assert calls["gauges"] == 1 and not same_bits(a, b)
    ens.sample("ChanQ", pix.copy())
    assert calls["gauges"] == 2


def test_the_rows_and_their_gaps_are_untouched(ensemble):
    """everything summary() and sample() read is as it was, and so is every element between the members' rows"""
    from lisflood_amd.soilloop import GAP_BYTE
    ens = ensemble
    names = ["sumDisDay", "ChanQ", LAND_ROW]
    before = {k: ens.download(k) for k in names}
    x = ens.chan_q_avg()
    thr = thresholds_for(x, 3)
    for name in ("ChanQAvg", "ChanQ", LAND_ROW):
        ens.summary(name, thresholds=thr, ranks=(0, M - 1))
        ens.sample(name, gauges(ens))
    for k in names:
        assert same_bits(ens.download(k), before[k]), k
    for k in ens.gap_names():
        g = ens.gaps(k)
        assert g.shape == (M, PAD), (k, g.shape)
        if g.dtype == np.uint8:
            assert (g == GAP_BYTE).all(), k
        else:
            assert ((g == HM.SENTINEL) | np.isnan(g)).all() and not np.isnan(g[:-1]).any(), (k, g)


def test_a_step_after_the_products_is_the_step_without_them(amd):
    """summary() and sample() between two steps (behind the channel loop on the side stream) change nothing of the run"""
    from lisflood_amd import synthetic as syn
    from lisflood_amd.hotpath import HotPathEnsemble
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(24, 30)
    n = 24 * 30
    runs = []
    for products in (False, True):
        ens = HotPathEnsemble(cp(values), sc, mask, ldd_to_chan, ldd_kin, members=2)
        for s in range(3):
            f = [syn.hotpath_forcing(n, s + 10 * m) for m in range(2)]
            ens.step({k: np.stack([x[k] for x in f]) for k in f[0]}, time_since_start=s + 1)
            if products:
                got = ens.summary("ChanQAvg", ranks=(1,))
                assert same_bits(got["max"], got["order"][0])            # two members: the upper one is the maximum
                ens.sample("ChanQ", np.arange(0, n, 7))
        runs.append({k: ens.download(k) for k in ens.state_names()})
        ens.free()
    for k in runs[0]:
        assert same_bits(runs[0][k], runs[1][k]), k


def test_a_gauge_row_goes_through_the_tss_writer(ensemble, tmp_path):
    from lisflood_amd import output
    ens = ensemble
    pix = gauges(ens)[:9]
    ids = list(range(101, 110))
    rows = ens.sample("ChanQAvg", pix)
    path = str(tmp_path / "dis_member1.tss")
    w = output.TssWriter(path, ids, pix, first_timestep=4, date="now")
    w.append(rows[1])
    w.sample(ens.chan_q_avg()[1])                    # the full vector gives the same line
    w.append(list(rows[1] * np.nan))                 # missing values
    w.close()
    _, got_ids, first, vals = output.read_tss(path)
    assert got_ids == ids and first == 4 and vals.shape == (3, 9)
    want = np.array([float("%14g" % v) for v in rows[1]])
    assert np.array_equal(vals[0], want) and np.array_equal(vals[1], want) and np.isnan(vals[2]).all()
    with pytest.raises(ValueError, match="one value per id"):
        w.append(rows[1][:5])
    with pytest.raises(ValueError, match="whole map"):
        output.TssWriter(path, ids, pix, how="mapmaximum").append(rows[1])
