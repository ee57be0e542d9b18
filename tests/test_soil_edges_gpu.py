"""-m gpu: the soil column kernel (csrc/lf_soil.hip) on the inputs of tests/soil_edges.py -- planted on both sides and on
the ties of its comparisons, on exact sub-step counts at the edges of its lists, and a hair from saturation -- in every
form: device-resident with derived and with streamed parameters, the 73-argument host call, LF_SOIL_TRIP_CAP unset / 0 / 1
and LF_GENERAL_POW=1.  (The land-surface form is pinned to the two-launch form bit for bit in tests/test_module_edges_gpu.py.)
tests/test_soil_edges_cpu.py shows, without a GPU, that the references used here are what they claim.

  a / b  pow-free columns: every form gives the oracle's bits in all 22 outputs, sentinels where the reference skips
  c      planted counts: the engine's histogram and its deferred count equal the oracle's, the FASTPOW forms give the same
         bits, every column is within the project's bar of the oracle, a sample is within 2 S + 4 E of the 240-bit reference
  d      soil_params and near-edge columns: finite where the reference is, within 2 S + 4 E of it"""
import ctypes as C

import numpy as np
import pytest

import module_edges as E
import soil_edges as S

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-11          # the soil tests of tests/test_gpu_parity.py
ENV = ("LF_SOIL_NO_DERIVED", "LF_SOIL_TRIP_CAP", "LF_GENERAL_POW")
FORMS = {                          # name: (device-resident?, environment, FASTPOW?)
    "derived": (True, {}, True),
    "streamed": (True, {"LF_SOIL_NO_DERIVED": "1"}, True),
    "host_call": (False, {}, True),
    "trip_cap_0": (True, {"LF_SOIL_TRIP_CAP": "0"}, True),
    "trip_cap_1": (True, {"LF_SOIL_TRIP_CAP": "1"}, True),
    "streamed_trip_cap_1": (True, {"LF_SOIL_NO_DERIVED": "1", "LF_SOIL_TRIP_CAP": "1"}, True),
    "general_pow": (True, {"LF_GENERAL_POW": "1"}, False),
    "general_pow_trip_cap_0": (True, {"LF_GENERAL_POW": "1", "LF_SOIL_TRIP_CAP": "0"}, False),
}


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def _run(amd, monkeypatch, d, form):
    """one soilColumnsWaterBalance pass of d in `form` -> (the 22 written arrays, sub-step histogram, deferred count)"""
    from lisflood_amd import soilloop
    resident, env, _ = FORMS[form]
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = S.clone(d)
    d.pop("powfree_drawn", None)
    hist = deferred = None
    if resident:
        dev = soilloop.SoilColumnsDevice(d)
        assert dev.derived
        dev.step()
        out = {k: dev.get(k) for k in S.WRITTEN}
        hist = dev.substep_histogram()
        nd = C.c_int64(0)
        amd.check(amd.lib().lf_soil_last_deferred(C.c_int(0), C.byref(nd)))
        deferred = nd.value
        for a in dev.dev.values():
            a.free()
    else:
        assert soilloop.soilColumnsWaterBalance(*[d[k] for k in soilloop.ARG_ORDER]) is None
        out = {k: d[k] for k in S.WRITTEN}
    return out, hist, deferred


def _oracle_run(oracle, d):
    ref = S.clone(d)
    ref.pop("powfree_drawn", None)
    oracle.soil_columns(ref)
    return ref, oracle.soil_trip_hist()


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(S.POWFREE_SETS))
def powfree(request, oracle):
    d, out, census, mid = S.powfree_case(**S.POWFREE_SETS[request.param]["kw"])
    return request.param, d, _oracle_run(oracle, d)[0], mid


@pytest.mark.parametrize("form", list(FORMS))
def test_powfree_columns_give_the_oracle_bits(amd, monkeypatch, powfree, form):
    name, d, ref, mid = powfree
    out, hist, deferred = _run(amd, monkeypatch, d, form)
    for k in S.WRITTEN:
        assert E.same_bits(out[k], ref[k]), "%s %s %s: %s" % (name, form, k, E.first_difference(out[k], ref[k]))
        assert (out[k][~mid["active"]] == S.SENTINEL).all(), (name, form, k)
    if hist is not None:
        assert hist.sum() == 0 and deferred == 0


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def substeps(oracle):
    d, counts, frozen = S.substep_inputs()
    ref, hist = _oracle_run(oracle, d)
    assert np.array_equal(hist, S.trip_histogram(counts))
    # the engine does not run a frozen column's sub-steps (its seepage is zero whatever they give): it is in no list
    want = hist - S.trip_histogram(counts[:, frozen])
    want[1] = 0
    cols = S.substep_sample(counts, frozen)
    return d, counts, frozen, ref, want, cols, S.exact_reference(d, cols, ref, np.minimum(counts, 127))


def test_planted_substep_counts_in_every_form(amd, monkeypatch, substeps):
    d, counts, frozen, ref, want, cols, R = substeps
    assert R["kept"].all()
    first = None
    for form, (resident, env, fastpow) in FORMS.items():
        out, hist, deferred = _run(amd, monkeypatch, d, form)
        if resident:
            assert np.array_equal(hist, want), (form, np.nonzero(hist != want)[0], hist[hist != want], want[hist != want])
            assert deferred == want.sum(), (form, deferred)
        for k in S.WRITTEN:
            np.testing.assert_allclose(out[k], ref[k], rtol=RTOL, atol=ATOL, err_msg="%s %s" % (form, k))
            if k.startswith("Seep"):
                assert (out[k][:, frozen] == 0).all(), (form, k)
        if fastpow:
            if first is None:
                first = out
            for k in S.WRITTEN:
                assert E.same_bits(out[k], first[k]), "%s %s: %s" % (form, k, E.first_difference(out[k], first[k]))
        got = np.array([[out[k][c] for k in S.WRITTEN] for c in cols])
        dist = S.rel_distance(got, R["ref"])
        print(S.bar_table("sub-step family, %s: bar, device distance from the exact reference, ratio" % form, R["bar"], dist))
        assert (dist <= R["bar"]).all(), (form, np.argwhere(dist > R["bar"])[:5])


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def near_edge(oracle):
    return S.near_edge_case(oracle)


@pytest.mark.parametrize("form", list(FORMS))
def test_near_edge_columns_against_the_exact_reference(amd, monkeypatch, near_edge, form):
    """E of the bar is taken separately over the soil_params columns and the planted ones: an ulp below saturation the
    oracle itself is up to 3.9e-3 from the exact result, which must not loosen the bar of the others (about 1e-12)."""
    d, cols, R = near_edge["d"], near_edge["cols"], near_edge["R"]
    kept = R["kept"]
    assert (~kept).sum() <= len(cols) // 100
    out, hist, deferred = _run(amd, monkeypatch, d, form)
    got = np.array([[out[k][c] for k in S.WRITTEN] for c in cols])
    assert np.isfinite(got[np.isfinite(R["ref"])]).all()
    dist = S.rel_distance(got, R["ref"])
    for gid, name in ((S.GENERIC, "soil_params columns"), (S.PLANTED, "planted columns")):
        sel = kept & (R["group"] == gid)
        print(S.bar_table("near-edge family, %s, %s: bar, device distance from the exact reference, ratio" % (name, form),
                          R["bar"][sel], dist[sel]))
    bad = kept[:, None] & (dist > R["bar"])
    assert not bad.any(), (form, [(cols[i], S.WRITTEN[k], dist[i, k], R["bar"][i, k]) for i, k in np.argwhere(bad)[:5]])
