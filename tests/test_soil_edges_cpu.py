"""No device: the C oracle's soil columns (oracle/lf_oracle.c: lfo_soil_columns) against the restatements of
tests/soil_edges.py, so that what tests/test_soil_edges_gpu.py compares the HIP kernel with is trustworthy before a GPU is
involved.

  a / b  the pow-free family (four parameter sets): the oracle equals the numpy restatement of soilloop.py:131-354 bit
         for bit, every census entry the set can have is non-zero, sentinels survive exactly where the reference skips
  c      lfo_soil_trip_hist equals the planted sub-step counts, exact ties and one-ulp neighbours included
  d      on soil_params and near-edge columns the oracle's sub-step count equals the 240-bit reference's; a column
         whose count differs, or changes under a perturbation of x^y, is left out -- at most 1 % may be"""
import numpy as np
import pytest

import module_edges as E
import soil_edges as S


def _oracle_run(oracle, d):
    ref = S.clone(d)
    ref.pop("powfree_drawn", None)
    oracle.soil_columns(ref)
    return ref


@pytest.fixture(scope="module", params=list(S.POWFREE_SETS))
def powfree(request):
    spec = S.POWFREE_SETS[request.param]
    d, out, census, mid = S.powfree_case(**spec["kw"])
    return request.param, spec, d, out, census, mid


def test_powfree_inputs_are_what_they_claim(powfree):
    from lisflood_amd.soilloop import derived_parameters_hold
    name, spec, d, out, census, mid = powfree
    V, N = d["W1a"].shape
    assert (V, N) == (4, S.POWFREE_N) and N % 256 != 0 and d["WS1a"].shape[0] == 3
    assert derived_parameters_hold(d)
    assert mid["powfree"][mid["active"]].all()            # every column that runs: x in {0, 1} in every x^y, one sub-step
    assert d["powfree_drawn"] > 0.9                        # (the rest are the saturated fall-back column)
    print(E.counts_table("soil columns, %s" % name, census))
    empty = [k for k, v in census.items() if v == 0]
    assert sorted(empty) == sorted(spec["empty"]), empty
    if name.startswith("paddy"):
        act = mid["active"]
        assert not act[1, 256:].any() and act[1, :256].any()         # mask row 0: empty over the whole second tile
        assert act[2].any() == (name == "paddy_two") and act[0].all() and act[3].all()


def test_oracle_equals_the_restatement_bit_for_bit(powfree, oracle):
    name, spec, d, out, census, mid = powfree
    ref = _oracle_run(oracle, d)
    for k in S.WRITTEN:
        assert E.same_bits(ref[k], out[k]), "%s %s: %s" % (name, k, E.first_difference(ref[k], out[k]))
        assert (ref[k][~mid["active"]] == S.SENTINEL).all(), (name, k)       # untouched where the reference skips
        assert not (ref[k][mid["active"]] == S.SENTINEL).any(), (name, k)
    hist = oracle.soil_trip_hist()
    assert hist[1] == mid["active"].sum() and hist.sum() == hist[1]


def test_trip_histogram_equals_the_planted_counts(oracle):
    d, counts, frozen = S.substep_inputs()
    from lisflood_amd.soilloop import derived_parameters_hold
    assert derived_parameters_hold(d)
    multi = [(counts[r, t * 256:(t + 1) * 256] > 1).sum() for r in range(S.SUB_V) for t in range(S.SUB_TILES_PER_ROW)]
    above = [(counts[r, t * 256:(t + 1) * 256] > 6).sum() for r in range(S.SUB_V) for t in range(S.SUB_TILES_PER_ROW)]
    assert len(multi) >= 17 and counts.shape[1] % 256 == S.SUB_RAGGED
    assert (above[0], above[1]) == (48, 49) and (multi[0] - above[0], multi[1] - above[1]) == (20, 20)
    assert multi[2:5] == [128, 129, 256] and multi[7] == 0 and multi[10:12] == [20, 21]
    assert (counts[1, 256:512] == 3).all()
    assert {127, 128, 300} <= set(counts[1, 512:768].tolist())
    assert frozen.any() and (counts[:, frozen] > 1).any()
    for c in S.SUB_COUNTS:                                 # each count on the tie, an ulp below it and (as c + 1) an ulp above
        assert (counts == c).sum() >= 2 and (counts == c + 1).sum() >= 1, c
    ref = _oracle_run(oracle, d)
    hist = oracle.soil_trip_hist()
    assert np.array_equal(hist, S.trip_histogram(counts)), np.nonzero(hist != S.trip_histogram(counts))
    assert hist.sum() == counts.size and hist[127] == (counts >= 127).sum()
    flat = np.stack([ref[k].ravel() for k in S.WRITTEN], axis=1)
    assert len(np.unique(flat, axis=0)) == flat.shape[0]  # no two columns alike: a swapped slot shows


def test_substep_sample_covers_every_count_and_every_place(oracle):
    d, counts, frozen = S.substep_inputs()
    cols = S.substep_sample(counts, frozen)
    assert len(cols) <= 64 and len(set(cols)) == len(cols)
    live = [c for c in cols if not frozen[c[1]]]
    sampled = {int(counts[c]) for c in live}
    for c in S.SUB_COUNTS:
        assert c in sampled and c + 1 in sampled, (c, sorted(sampled))
    assert sum(counts[c] >= 300 for c in live) <= 3            # the 300-step columns: few enough for the time budget
    places = S.substep_places(counts, frozen, cols)
    assert {"lane", "tile", "straggler", "tile or straggler"} <= set(places), set(places)
    assert any(frozen[p] for v, p in cols)


def test_pow_bound_is_the_documented_one():
    import os
    import re
    import test_device_math_gpu as M
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "lisflood-code_amd", "csrc", "lf_math.h")).read()
    found = re.search(r"relative error <= ([0-9.e-]+) for \|y log2 x\| <= 50 and <= ([0-9.e-]+) beyond", text)
    assert found, "lf_math.h no longer states the bounds of lf_pow_pos in the words this test reads"
    assert S.POW_BOUND == max(float(found.group(1)), float(found.group(2)))
    assert M.POW_POS_REL < S.POW_BOUND <= M.POW_POS_REL_WIDE


@pytest.fixture(scope="module")
def near_edge(oracle):
    return S.near_edge_case(oracle)


def test_oracle_counts_equal_the_exact_reference_counts(near_edge):
    cols, R, counts, ref = near_edge["cols"], near_edge["R"], near_edge["counts"], near_edge["ref"]
    assert len(cols) == 3 * (S.NEAR_GENERIC + S.NEAR_PLANTED)
    left_out = int((~R["kept"]).sum())
    print("columns left out (the oracle's count differs or a perturbation of x^y changes it): %d of %d" % (left_out, len(cols)))
    assert left_out <= len(cols) // 100
    got = np.array([counts[c] for c in cols])
    assert np.array_equal(got[R["kept"]], np.minimum(R["nsub"][R["kept"]], 127))
    for gid, name in ((S.GENERIC, "soil_params columns"), (S.PLANTED, "planted columns")):
        sel = R["kept"] & (R["group"] == gid)
        print(S.bar_table("near-edge family, %s: the bar and the oracle's own distance from the exact reference" % name,
                          R["bar"][sel], R["oracle_distance"][sel]))
    assert (R["oracle_distance"][R["kept"]] <= R["bar"][R["kept"]]).all()
    # the bar of the soil_params columns is what the arithmetic allows, three orders below the 1e-9 of the parity tests:
    # the oracle's own rounding (E) and the documented error of x^y carried through the column (S)
    generic = R["kept"] & (R["group"] == S.GENERIC)
    assert generic.sum() >= 3 * S.NEAR_GENERIC - left_out
    assert R["E"][S.GENERIC].max() < 1e-13 and R["bar"][generic].max() < 1e-11
    orc = np.array([[ref[k][c] for k in S.WRITTEN] for c in cols])
    assert np.array_equal(np.isfinite(orc), np.isfinite(R["ref"]))   # (Sat1b = 0 / 0 where layer 1b has no depth)
