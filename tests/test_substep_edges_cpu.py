"""The CPU oracle's routing sub-step (oracle.RoutingSubstep.dynamic) against a numpy restatement of routing.py:512-603,
693-703, bit for bit, on inputs that take both sides and the ties of every comparison of the sub-step -- and the census,
the guard and the derived-statics facts that show the inputs are what tests/test_substep_edges_gpu.py needs
(tests/substep_edges.py).  No GPU: this is what makes the expected values of that file trustworthy."""
import numpy as np
import pytest

import module_edges as E
import substep_edges as S

SEED = 5
CONFIGS = [(family, split, irregular) for family in S.FAMILIES for split in (False, True) for irregular in (False, True)]
_ids = ["%s-%s-%s" % (f, "split" if s else "single", "irregular" if i else "regular") for f, s, i in CONFIGS]
_inputs = {}


def inputs(family):
    if family not in _inputs:
        _inputs[family] = S.substep_inputs(True, SEED, family)
    return _inputs[family]


def _same(got, want, what):
    assert E.same_bits(got, want), "%s: %s" % (what, E.first_difference(got, want))


def run(oracle, family, split, irregular, beta=S.BETA, sideflows=None):
    """-> per sub-step (the oracle's step, the restatement's outputs, its intermediates with the census' extras)"""
    key = (family, split, irregular, beta, sideflows is None)
    if key in _runs:
        return _runs[key]
    d = inputs(family)
    vals = S.statics(d, irregular)
    ref = S.reference_scalars(vals, beta, S.NSTEPS if sideflows is None else len(sideflows))
    out = []
    for step in S.oracle_run(oracle, d, split, irregular, beta, sideflows):
        want, mid = S.substep_reference(ref, step["before"], step["side"], split, step["qr1"], step["qr2"])
        out.append((step, want, S.census_mid(d, vals, step, mid, beta)))
    _runs[key] = out
    return out


_runs = {}


@pytest.mark.parametrize("family, split, irregular", CONFIGS, ids=_ids)
def test_oracle_is_the_reference_lines_and_the_inputs_take_every_branch(oracle, family, split, irregular):
    """every state and output vector after each of the five sub-steps has the bits of the restatement driven with the
    oracle's own router outputs; every census row is taken in the first sub-step (the rows that can only arise later: in
    some sub-step); no cell of a later sub-step sits on the M3Limit test"""
    total, guard, ill = {}, 0, 0
    names = S.STATE + S.OUT if split else ["ChanQKin", "ChanM3Kin", "ChanQ", "sumDisDay"] + S.OUT
    for s, (step, want, mid) in enumerate(run(oracle, family, split, irregular)):
        for k in names:
            _same(step["after"][k], want[k], (s, k))
        census = S.substep_census(mid)
        ill += S.substep_conditioning(mid, step["after"])
        for k, n in census.items():
            total[k] = total.get(k, 0) + n
        if s == 0:
            print("\n" + E.counts_table("sub-step 0, %s" % family, census))
            empty = [k for k, n in census.items() if n < 1 and k not in S.LATER_ROWS]
            assert not empty, E.counts_table("empty rows in the first sub-step: %s" % empty, census)
        else:
            guard += S.substep_guard(mid)
        if s == S.NSTEPS - 1:      # the fused forms compute the velocities in the last sub-step only
            last = {k: n for k, n in census.items() if k[:2] in ("k:", "l:", "m:")}
            assert min(last.values()) >= 1, E.counts_table("last sub-step", last)
    later = [k for k in S.LATER_ROWS if k in total and total[k] < 1]
    if split or irregular:         # (single routing resets a NaN sideflow; NaN then needs ChannelAlpha = 0)
        assert not later, E.counts_table("rows never taken: %s" % later, total)
    assert guard == 0, guard
    assert ill == 0, ill           # no ChanQ is a difference that the tolerance of the GPU file could not hold


@pytest.mark.parametrize("family", S.FAMILIES)
def test_guard_holds_for_the_other_runs_of_the_gpu_file(oracle, family):
    """a general beta (0.72), and the staggered sideflows (cases d, g, n in sub-steps 1, 2, 3): oracle == restatement there
    too, and nothing near the M3Limit test after the first sub-step"""
    d = inputs(family)
    for beta, sideflows in ((0.72, None), (S.BETA, d["staggered"])):
        guard = 0
        for s, (step, want, mid) in enumerate(run(oracle, family, True, False, beta, sideflows)):
            for k in S.STATE + S.OUT:
                _same(step["after"][k], want[k], (beta, s, k))
            guard += S.substep_guard(mid) if s else 0
            guard += S.substep_conditioning(mid, step["after"])
        assert guard == 0, (beta, guard)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_planted_ties_are_exact_and_the_expected_values_follow(oracle, family):
    """what the GPU file asserts bit for bit on the planted cells is there to assert: the sideflow per metre of the d cells
    is the planted number itself, the e cells sit below, on and one ulp above the limit, and Sideflow1Chan after the first
    sub-step is side on the ties' near side and ratio * side beyond"""
    d = inputs(family)
    step, want, mid = run(oracle, family, True, False)[0]
    c = d["cells"]
    side, s1 = mid["side"], step["after"]["Sideflow1Chan"]
    for name, x in (("d_plus", 9.9e-8), ("d_minus", -9.9e-8), ("d_tie", 1e-7), ("d_below", np.nextafter(1e-7, 0.0))):
        assert (side[c[name]] == x).all(), name
    assert (s1[c["d_plus"]] == 9.9e-8).all() and (s1[c["d_minus"]] == -9.9e-8).all() and (s1[c["d_below"]] == side[c["d_below"]]).all()
    assert (s1[c["d_tie"]] == 0.8 * 1e-7).all()                       # |side| < 1e-7 is false on the tie: ratio = 2048 / 2560
    ex = mid["excess"]
    assert (ex[c["e_below"]] == 448.0).all() and (ex[c["e_tie"]] == 512.0).all() and (ex[c["e_above"]] == np.nextafter(512.0, 1e3)).all()
    assert (s1[c["e_below"]] == 1e-4).all() and (s1[c["e_tie"]] == 1e-4).all()
    assert (s1[c["e_above"]] == (512.0 + 2.0 ** -43) / (768.0 + 2.0 ** -43) * 1e-4).all()
    assert (s1[c["f_tot0"]] == 0).all() and (s1[c["f_m3_0"]] == 0).all() and (s1[c["a"]] == 0).all()
    assert (mid["sinu_raw"][c["l_tie"]] == 1.0).all() and (mid["sinu_raw"][c["l_below"]] == 0.5).all()
    assert (step["after"]["ChanQKin"][c["g_main"] + c["g_tiny"]] == 0).all() and (step["after"]["Chan2QKin"][c["g_flood"]] > 0).all()
    # single routing resets the NaN sideflow, split routing carries it into the pit below
    single = run(oracle, family, False, False)
    assert all(np.isfinite(st["after"]["ChanQKin"]).all() for st, _, _ in single)
    last = run(oracle, family, True, False)[-1][0]["after"]["ChanQKin"]
    below = d["down"][c["n_upstream"]]
    assert np.isnan(last[c["n_pit"] + c["n_upstream"]]).all() and np.isnan(last[below]).all()
    assert int(np.isnan(last).sum()) == 6                               # ... and poisons nothing else
    # the inert candidates: -0.0 becomes +0.0 where the arithmetic says so
    for k in S.INERT_TESTED:
        x = last[c["b_minus"]] if k == "ChanQKin" else run(oracle, family, True, False)[-1][0]["after"][k][c["b_minus"]]
        assert (x == 0).all() and not np.signbit(x).any(), k


@pytest.mark.parametrize("family", S.FAMILIES)
def test_derived_statics_and_graph_shape(oracle, family):
    """the regular statics keep the five derived relations of k_check_derived bit-exact (the kernels recompute the derived
    vectors), the irregular ones break one (they read them); ChannelAlpha = 0 alone would not: 1 / 0 = inf is exact.  And the
    raster still gives each fused form its graph: deep more levels than a level block holds (8 at this size), shallow a few
    wide ones."""
    from lisflood_amd.kinematic_wave_parallel import Graph
    d = inputs(family)
    for irregular in (False, True):
        v = S.statics(d, irregular)
        kw = oracle.kinematicWave(d["codes"][d["mask"]].astype(np.float64), d["mask"], v["ChannelAlpha"], S.BETA, v["ChanLength"],
                                  S.DT, alpha_floodplains=v["ChannelAlpha2"])
        rel = S.derived_relations(v, kw.a_dx_div_dt_channel, kw.a_dx_div_dt_floodplains)
        if not irregular:
            assert all(r.all() for r in rel.values()), {k: int((~r).sum()) for k, r in rel.items()}
        else:
            assert (~rel["InvChanLength"]).sum() == 1 and not rel["InvChanLength"][d["irregular_cells"]["length"]]
            assert rel["InvChannelAlpha"].all() and np.isinf(v["InvChannelAlpha"][d["irregular_cells"]["alpha0"]]).all()
    g = Graph(ldd_raster=d["codes"])
    perm, ups_ptr, level_start = g.layout()
    widths = np.diff(level_start)
    assert g.num_pixels == S.N and sorted(perm.tolist()) == list(range(S.N))
    if family == "deep":
        assert g.num_levels > 3 * 8 and np.median(widths) >= 64, (g.num_levels, widths)
    else:
        assert 2 <= g.num_levels <= 16 and widths.max() > 1000, (g.num_levels, widths)
    # the isolated cells all lie in the last level, whose last workgroup (256 cells) is a partial one that carries some
    last = perm[level_start[-2]:]
    assert d["isolated"][last].sum() == d["isolated"].sum() >= 30
    assert last.size % 256 != 0 and d["isolated"][last[last.size // 256 * 256:]].any()
    g.close()
