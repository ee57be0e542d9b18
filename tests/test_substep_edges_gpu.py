"""-m gpu: every copy of the routing sub-step arithmetic on the device at its branch edges (inputs, census and expected
values: tests/substep_edges.py, pinned on the CPU by tests/test_substep_edges_cpu.py).

  * the stage kernels of lf_routing_substep (pixel and engine order) against the C oracle after every sub-step, at the
    routing tolerance of test_gpu_parity.py, NaN positions exactly, the planted ties bit for bit where no pow is involved;
  * every fused form -- time-major level kernel, one-wavefront cones (width 64 and 256), chain / supply cones, skewed
    wavefront over levels (fused_cell), several model steps per call, the members call -- against the sequential engine,
    bit for bit, the sign of a zero included.

Every run is 96 x 80 cells and five sub-steps; routers, oracle runs and the sequential engine's results are made once."""
import ctypes as C
import types

import numpy as np
import pytest

import module_edges as E
import substep_edges as S

pytestmark = pytest.mark.gpu

SEED = 5
SENTINEL, PAD = -777.25, 37
FORM_SWITCHES = ("LF_FUSED_TIME_MAJOR", "LF_FUSED_SPLIT", "LF_FUSED_LEVELS", "LF_FUSED_CONE_WIDTH", "LF_NO_INERT_SKIP",
                 "LF_NO_RECOMPUTE", "LF_GENERAL_POW", "LF_FUSED_WIDE", "LF_FUSED_SPLIT_MAX")


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    from lisflood_amd import kinematic_wave_parallel, routing
    return types.SimpleNamespace(kw=kinematic_wave_parallel, routing=routing, lib=_lib)


@pytest.fixture
def switches(monkeypatch):
    """every switch that picks a fused form or an arithmetic path unset; set(**kw) sets some for the test, which restores all"""
    for k in FORM_SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_(**kw):
        for k, x in kw.items():
            if x is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(x))
    return set_


_inputs, _oracle_runs, _sequential = {}, {}, {}


def inputs(family):
    if family not in _inputs:
        _inputs[family] = S.substep_inputs(True, SEED, family)
    return _inputs[family]


def oracle_steps(oracle, family, split, irregular, beta):
    key = (family, split, irregular, beta)
    if key not in _oracle_runs:
        _oracle_runs[key] = S.oracle_run(oracle, inputs(family), split, irregular, beta)
    return _oracle_runs[key]


def make_router(amd, d, vals, beta=S.BETA):
    """the router as routing.initialSecond builds it: alpha = ChannelAlpha(2), dx = ChanLength (reads LF_GENERAL_POW,
    LF_FUSED_LEVELS and LF_FUSED_CONE_WIDTH)"""
    g = amd.kw.Graph(ldd_raster=d["codes"])
    return amd.kw.kinematicWave(None, None, vals["ChannelAlpha"], beta, vals["ChanLength"], S.DT, graph=g,
                                alpha_floodplains=vals["ChannelAlpha2"])


def step_device(kw, vals, split, side, beta=S.BETA, nsteps=S.NSTEPS):
    from bench_support import RoutingStepDevice
    return RoutingStepDevice(kw, dict(vals, SideflowChanM3=side), split, beta, 1.0 / S.DT, S.DT * nsteps)


def all_vectors(r):
    from lisflood_amd.routing import _OUT, _STATE
    return {k: r.download(k) for k in _STATE + _OUT}


def assert_same(got, want, what):
    for k in want:
        assert E.same_bits(got[k], want[k]), "%s, %s: %s" % (what, k, E.first_difference(got[k], want[k]))


def sequential(amd, family, split, irregular, general, sideflows=None):
    """what NSTEPS x lf_routing_substep (engine order) leave: with the resident sideflow vector (sideflows = None: the first
    of the inputs') or with one vector uploaded before each sub-step -> name -> [N] pixel order"""
    key = (family, split, irregular, general, sideflows)
    if key not in _sequential:
        d = inputs(family)
        vals = S.statics(d, irregular)
        kw = make_router(amd, d, vals)
        r = step_device(kw, vals, split, d["sideflows"][0])
        if sideflows is None:
            r.run_sequential(S.NSTEPS)
        else:
            for side in d[sideflows]:
                r.dev["SideflowChanM3"].upload(np.ascontiguousarray(side[r.perm]))
                r.run_sequential(1)
        _sequential[key] = all_vectors(r)
        r.free()
        kw.close()
    return _sequential[key]


# ======================================================================================================================
# 1. the stage kernels against the oracle
# ======================================================================================================================
def _sequential_against_oracle(amd, oracle, family, split, irregular, engine_order, beta=S.BETA):
    from lisflood_amd.routing import SubstepVectors, result_names, substep_host_vectors
    d = inputs(family)
    vals = S.statics(d, irregular)
    kw = make_router(amd, d, vals, beta)
    perm = kw.graph.layout()[0].astype(np.int64) if engine_order else None
    sv = SubstepVectors(substep_host_vectors(vals, S.N, perm), S.N, beta, 1.0 / S.DT, S.DT * S.NSTEPS, split, engine_order)
    names = result_names(split)
    c = d["cells"]

    def download(k):
        x = sv.download(k)
        if perm is None:
            return x
        out = np.empty(S.N)
        out[perm] = x
        return out
    for s, step in enumerate(oracle_steps(oracle, family, split, irregular, beta)):
        side = d["sideflows"][s]
        sv.upload("SideflowChanM3", np.ascontiguousarray(side if perm is None else side[perm]))
        amd.lib.check(amd.lib.lib().lf_routing_substep(kw._h, C.byref(sv.args)))
        got = {k: download(k) for k in names}
        S.close_to_oracle(got, step["after"], names, vals, (family, s))
        if s == 0:
            # the ties, on the vectors that involve no pow: the split of the sideflow (cases d, e, and f, a beside them) ...
            if split:
                tie = [x for name in c if name[:2] in ("d_", "e_", "f_", "a") for x in c[name]]
                assert E.same_bits(got["Sideflow1Chan"][tie], step["after"]["Sideflow1Chan"][tie]), \
                    E.first_difference(got["Sideflow1Chan"][tie], step["after"]["Sideflow1Chan"][tie])
            # ... and TravelDistance = FlowVelocity * DtSec on the sinuosity cells (case l), whose factor is exactly 0.5, 1, 1
            cells = c["l_below"] + c["l_tie"] + c["l_above"]
            assert E.same_bits(got["TravelDistance"][cells], got["FlowVelocity"][cells] * (S.DT * S.NSTEPS))
            # (the three columns differ in PixelArea alone, so their velocities differ by the factor alone)
            fv = got["FlowVelocity"]
            assert E.same_bits(fv[c["l_below"]], 0.5 * fv[c["l_tie"]]) and E.same_bits(fv[c["l_above"]], fv[c["l_tie"]])
            assert (fv[c["l_tie"]] > 0).all()
    sv.free()
    kw.close()


@pytest.mark.parametrize("irregular", [False, True], ids=["regular", "irregular"])
@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
@pytest.mark.parametrize("engine_order", [False, True], ids=["pixel_order", "engine_order"])
@pytest.mark.parametrize("general", [False, True], ids=["fused_beta_3_5", "general_pow"])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_sequential_against_the_oracle(amd, oracle, switches, family, general, engine_order, split, irregular):
    """k_substep_sideflow / _main / _floodplain around the two router calls, sub-step by sub-step with its own sideflow vector:
    every vector the sub-step writes against the oracle after every sub-step (rtol 1e-9, atol 1e-12; CrossSection2Area atol
    1e-9 max|Chan2M3Start / ChanLength|), NaN exactly where the oracle has it, Sideflow1Chan of the planted ties bit for bit"""
    switches(LF_GENERAL_POW="1" if general else None)
    _sequential_against_oracle(amd, oracle, family, split, irregular, engine_order)


def test_sequential_against_the_oracle_general_beta(amd, oracle, switches):
    """beta = 0.72: every pow of the stage kernels and the router is OCML's"""
    _sequential_against_oracle(amd, oracle, "deep", True, False, True, beta=0.72)


# ======================================================================================================================
# 2. every fused copy against the sequential engine
# ======================================================================================================================
# name -> (family, switches read when the router is made, switches read by the call, last_fused_form())
FORMS = {
    "time_major": ("shallow", {}, dict(LF_FUSED_TIME_MAJOR=1), "time-major"),
    "cones": ("deep", {}, dict(LF_FUSED_TIME_MAJOR=0, LF_FUSED_SPLIT=0), "level blocks"),
    "cones_256": ("deep", dict(LF_FUSED_CONE_WIDTH=256), dict(LF_FUSED_TIME_MAJOR=0, LF_FUSED_SPLIT=0), "level blocks"),
    "chain_supply": ("deep", {}, dict(LF_FUSED_TIME_MAJOR=0, LF_FUSED_SPLIT=1, LF_NO_INERT_SKIP=1), "level blocks"),
    "levels_deep": ("deep", dict(LF_FUSED_LEVELS=1), dict(LF_FUSED_TIME_MAJOR=0), "levels"),
    "levels_shallow": ("shallow", dict(LF_FUSED_LEVELS=1), dict(LF_FUSED_TIME_MAJOR=0), "levels"),
}
FORM_CASES = [(form, general) for form in FORMS for general in (False, True) if not (general and form == "chain_supply")]


@pytest.mark.parametrize("irregular", [False, True], ids=["regular", "irregular"])
@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
@pytest.mark.parametrize("form, general", FORM_CASES, ids=["%s-%s" % (f, "general_pow" if g else "fused_beta_3_5") for f, g in FORM_CASES])
def test_fused_form_equals_sequential(amd, switches, form, general, split, irregular):
    """One fused call of five sub-steps against 5 x lf_routing_substep in engine order: every state and output vector bit for
    bit (same_bits: the sign of a zero counts), in the form's own switches, then with LF_NO_INERT_SKIP flipped and with
    LF_NO_RECOMPUTE=1 -- the same bits each time -- and the inert candidates of case b as the sequential engine leaves them.

    chain_supply: fused_impl (lf_router.hip) launches k_fused_cones_split instead of k_fused_cones only when
    all35 && !F.inert && cw == 64, i.e. the router solves beta = 3/5 with the quintic (beta 0.6, no LF_GENERAL_POW), no inert
    flags are in use (the graph has isolated cells, so LF_NO_INERT_SKIP=1) and the cones are one wavefront wide (no
    LF_FUSED_CONE_WIDTH); LF_FUSED_SPLIT=1 takes it whatever the number of cones.  No accessor tells the two cone kernels
    apart, so the conditions that can be seen from here are asserted."""
    import os
    family, at_creation, at_call, expect = FORMS[form]
    d = inputs(family)
    vals = S.statics(d, irregular)
    switches(LF_GENERAL_POW="1" if general else None)
    want = sequential(amd, family, split, irregular, general)
    switches(**at_creation)
    kw = make_router(amd, d, vals)
    switches(**at_call)
    if form == "chain_supply":
        assert "LF_GENERAL_POW" not in os.environ and "LF_FUSED_CONE_WIDTH" not in os.environ and kw.beta == 0.6
        assert os.environ["LF_NO_INERT_SKIP"] == "1" and os.environ["LF_FUSED_SPLIT"] == "1" and d["isolated"].any()
    skip0 = at_call.get("LF_NO_INERT_SKIP")
    for inert_skip, no_recompute in ((skip0, None), (None if skip0 else 1, None), (skip0, 1)):
        switches(LF_NO_INERT_SKIP=inert_skip, LF_NO_RECOMPUTE=no_recompute)
        r = step_device(kw, vals, split, d["sideflows"][0])
        r.run_fused(S.NSTEPS)
        got = all_vectors(r)
        r.free()
        assert kw.last_fused_form() == expect, (form, kw.last_fused_form())
        assert_same(got, want, (form, "LF_NO_INERT_SKIP", inert_skip, "LF_NO_RECOMPUTE", no_recompute))
        S.inert_cells_are_left_alone(d, got, want, split)
    kw.close()


STRIDE_FORMS = ["time_major", "cones", "chain_supply", "levels_deep"]


@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
@pytest.mark.parametrize("form", STRIDE_FORMS)
def test_sideflow_per_substep_equals_sequential(amd, switches, form, split):
    """sideflow stride N: the tiny sideflows (case d) arrive in sub-step 1, the negative ones (g) in sub-step 2, the NaN
    (n) in sub-step 3 -- the same bits as uploading each vector before its sequential sub-step"""
    family, at_creation, at_call, expect = FORMS[form]
    d = inputs(family)
    vals = S.statics(d)
    want = sequential(amd, family, split, False, False, "staggered")
    switches(**at_creation)
    kw = make_router(amd, d, vals)
    switches(**at_call)
    r = step_device(kw, vals, split, d["sideflows"][0])
    r.run_fused_sideflow_per_substep(list(d["staggered"]))
    got = all_vectors(r)
    r.free()
    assert kw.last_fused_form() == expect
    assert_same(got, want, form)
    assert np.isnan(got["ChanQKin"]).sum() == (6 if split else 0)
    kw.close()


@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
@pytest.mark.parametrize("family, time_major", [("shallow", 1), ("shallow", 0), ("deep", 0)])
def test_model_steps_in_one_call_equal_sequential(amd, switches, family, time_major, split):
    """lf_routing_model_steps_fused, 2 model steps x 3 sub-steps, each model step with its own sideflow vector (the planted
    one, then the staggered one that brings the NaN): every state vector and both rows of the discharge sums against the
    sequential engine run model step by model step with the sum zeroed in between"""
    d = inputs(family)
    vals = S.statics(d)
    sides = [d["sideflows"][0], d["staggered"][3]]
    kw = make_router(amd, d, vals)
    a = step_device(kw, vals, split, sides[0], nsteps=3)
    want_sums = []
    for side in sides:
        a.dev["SideflowChanM3"].upload(np.ascontiguousarray(side[a.perm]))
        a.dev["sumDisDay"].zero()
        a.run_sequential(3)
        want_sums.append(a.download("sumDisDay"))
    want = all_vectors(a)
    a.free()
    switches(LF_FUSED_TIME_MAJOR=time_major)
    b = step_device(kw, vals, split, sides[0], nsteps=3)
    sums = b.run_model_steps(3, sides)
    got = all_vectors(b)
    b.free()
    assert kw.last_fused_form() == ("time-major" if time_major else "level blocks")
    for m in range(2):
        assert E.same_bits(sums[m], want_sums[m]), (m, E.first_difference(sums[m], want_sums[m]))
    del got["sumDisDay"], want["sumDisDay"]
    assert_same(got, want, (family, time_major))
    kw.close()


# ---- the members call ------------------------------------------------------------------------------------------------
def _together(kw, vals, states, side_rows, split, members, stride):
    """all members in one lf_routing_substeps_fused_members call (as test_substep_members_gpu.together) -> name -> [M, stride]"""
    from lisflood_amd.routing import _OUT, _STATE, _STATIC, SubstepVectors, substep_host_vectors
    perm = kw.graph.layout()[0].astype(np.int64)
    srows = np.full((members, S.N + PAD), SENTINEL)
    srows[:, :S.N] = side_rows[:, perm]
    sv = SubstepVectors(substep_host_vectors(vals, S.N, perm, _STATIC), S.N, S.BETA, 1.0 / S.DT, S.DT * S.NSTEPS, split, True,
                        sideflow=srows, lengths={k: members * stride for k in _STATE + _OUT})
    for k in _STATE + _OUT:
        rows = np.full((members, stride), SENTINEL)
        rows[:, :S.N] = np.stack([st[k][perm] if k in st else np.zeros(S.N) for st in states])
        sv.upload(k, rows.reshape(-1))
    kw.routing_substeps_members(sv.args, S.NSTEPS, members, stride, 0, S.N + PAD)
    out = {k: sv.download(k).reshape(members, stride) for k in _STATE + _OUT}
    side_after = sv.download("SideflowChanM3").reshape(members, S.N + PAD)
    assert np.array_equal(side_after, srows, equal_nan=True)
    sv.free()
    return out


@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
@pytest.mark.parametrize("time_major", [1, 0], ids=["member_kernel", "fallback"])
def test_members_equal_their_single_calls(amd, switches, time_major, split):
    """lf_routing_substeps_fused_members, shallow, 3 members, member_stride = N + 37 with a sentinel in the padding: member 0
    the planted state with finite sideflows, member 1 the same with -0.0 in every tested vector of every inert candidate,
    member 2 with the NaN sideflows.  Time-major on: k_fused_level_steps_members; off: the members one after the other
    through the single call's schedule.  Each member bit-identical to lf_routing_substeps_fused on it alone, the padding
    untouched."""
    from lisflood_amd.routing import _OUT, _STATE
    d = inputs("shallow")
    vals = S.statics(d)
    kw = make_router(amd, d, vals)
    switches(LF_FUSED_TIME_MAJOR=time_major)
    base = {k: vals[k] for k in _STATE}
    minus = {k: a.copy() for k, a in base.items()}
    for cells in d["inert_cells"].values():
        for k in S.INERT_TESTED:
            minus[k][cells] = -0.0
    states = [base, minus, base]
    finite = d["sideflows"][0].copy()
    finite[d["nan_cells"]] = 1e-4 * S.LEN * S.DT
    assert np.isfinite(finite).all() and np.isnan(d["sideflows"][0]).sum() == 4
    side_rows = np.stack([finite, finite, d["sideflows"][0]])
    perm = kw.graph.layout()[0].astype(np.int64)
    want = []
    for m in range(3):
        r = step_device(kw, dict(vals, **states[m]), split, side_rows[m])
        r.run_fused(S.NSTEPS)
        want.append({k: r.dev[k].download() for k in _STATE + _OUT})
        r.free()
        assert kw.last_fused_form() == ("time-major" if time_major else "level blocks")
    got = _together(kw, vals, states, side_rows, split, 3, S.N + PAD)
    assert kw.last_fused_form() == ("time-major" if time_major else "level blocks")
    for k, rows in got.items():
        for m in range(3):
            assert E.same_bits(rows[m, :S.N], want[m][k]), (k, m, E.first_difference(rows[m, :S.N], want[m][k]))
        assert (rows[:, S.N:] == SENTINEL).all(), k
    assert np.isfinite(got["ChanQKin"][:2, :S.N]).all() and np.isnan(got["ChanQKin"][2, :S.N]).sum() == (6 if split else 0)
    if split:                                   # member 1's -0.0 made a difference where the candidate is skipped in member 0
        plus = np.flatnonzero(np.isin(perm, d["inert_cells"]["plus"]))
        assert (np.ascontiguousarray(got["ChanQKin"][0, plus]).view(np.uint64) == 0).all()
    kw.close()
