"""-m gpu: the routing sub-step on the ROW-BLOCK PARTITION at its branch edges and through cuts of every shape (inputs, cuts and
census: tests/dist_edges.py, asserted on the CPU by tests/test_dist_edges_cpu.py).

The reference is always the whole raster through NSTEPS x lf_routing_substep in engine order; tests/test_substep_edges_gpu.py
holds it to the oracle on the edges inputs, this file does on the others.  Every run on the partition -- sub-step by sub-step
(lf_substep_stage around the partitioned router calls, and the C composite lf_dist_routing_substep), the three fused forms of
lf_dist_fused_phase with the halo blocks of the slabs copied between the blocks, per-sub-step sideflows, several model steps
per call, a slab wider than the call -- is compared with it bit for bit, the sign of a zero included (module_edges.same_bits),
on every state and output vector.  All blocks of a partition live in one process on one device, six at the most."""
import types

import numpy as np
import pytest

import dist_edges as X
import module_edges as E
import substep_edges as S

pytestmark = pytest.mark.gpu

FORM_SWITCHES = ("LF_FUSED_TIME_MAJOR", "LF_FUSED_SPLIT", "LF_FUSED_LEVELS", "LF_FUSED_CONE_WIDTH", "LF_NO_INERT_SKIP",
                 "LF_NO_RECOMPUTE", "LF_GENERAL_POW", "LF_FUSED_WIDE", "LF_FUSED_SPLIT_MAX", "LF_ROUTE_CONES", "LF_ROUTE_LEVELS",
                 "LF_LEVEL_STATICS")
# name -> (switches read when the graphs are finalized, switches read by the call, last_fused_form() of every block)
FORMS = {
    "time_major": ({}, dict(LF_FUSED_TIME_MAJOR=1), "time-major"),
    "level_blocks": ({}, dict(LF_FUSED_TIME_MAJOR=0), "level blocks"),
    "levels": (dict(LF_FUSED_LEVELS=1), dict(LF_FUSED_TIME_MAJOR=0), "levels"),
}
NEW = [n for n in X.NAMES if n not in X.EDGES]
GENERAL_POW_ON = X.EDGES + tuple(n for n in X.NAMES if n.startswith("seam"))
_split = pytest.mark.parametrize("split", [False, True], ids=["single", "split"])


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    from lisflood_amd import dist, kinematic_wave_parallel
    return types.SimpleNamespace(kw=kinematic_wave_parallel, dist=dist, lib=_lib)


@pytest.fixture
def switches(monkeypatch):
    """every switch that picks a form or an arithmetic path unset; set(**kw) sets some for the test, which restores all"""
    for k in FORM_SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_(**kw):
        for k, x in kw.items():
            if x is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(x))
    return set_


def assert_same(got, want, what):
    for k in want:
        assert E.same_bits(got[k], want[k]), "%s, %s: %s" % (what, k, E.first_difference(got[k], want[k]))


def whole(amd, d, vals, split, side, nsteps=S.NSTEPS):
    """the whole raster on one router (reads LF_GENERAL_POW) -> (router, its RoutingStepDevice)"""
    from bench_support import RoutingStepDevice
    g = amd.kw.Graph(ldd_raster=d["codes"], land_mask=None if d["mask"].all() else d["mask"])
    kw = amd.kw.kinematicWave(None, None, vals["ChannelAlpha"], S.BETA, vals["ChanLength"], S.DT, graph=g,
                              alpha_floodplains=vals["ChannelAlpha2"])
    return kw, RoutingStepDevice(kw, dict(vals, SideflowChanM3=side), split, S.BETA, 1.0 / S.DT, S.DT * nsteps)


def all_vectors(r):
    from lisflood_amd.routing import _OUT, _STATE
    return {k: r.download(k) for k in _STATE + _OUT}


def model_step_sides(name):
    """the sideflow vectors of two model steps: the resident one, then (edges) the staggered one that brings the NaN"""
    d, _ = X.inputs(name)
    return [d["sideflows"][0], d["staggered"][3] if name in X.EDGES else d["sideflows"][1]]


_reference = {}


def reference(amd, name, split, irregular=False, general=False, kind="resident"):
    """what lf_routing_substep in engine order leaves on the whole raster -> name -> [N] pixel order.  kind: `resident` NSTEPS
    sub-steps with the first sideflow vector; `staggered` one vector of d['staggered'] uploaded before each; `model_steps` two
    model steps of NSTEPS with the vectors of model_step_sides and the sum zeroed in between (-> vectors, the two sums);
    `7_then_5` twelve sub-steps.  The caller has set LF_GENERAL_POW to match `general`."""
    key = (name, split, irregular, general, kind)
    if key not in _reference:
        d, _ = X.inputs(name)
        vals = S.statics(d, irregular)
        kw, r = whole(amd, d, vals, split, d["sideflows"][0])
        if kind == "resident":
            r.run_sequential(S.NSTEPS)
            out = all_vectors(r)
        elif kind == "7_then_5":
            r.run_sequential(12)
            out = all_vectors(r)
        elif kind == "staggered":
            for side in d["staggered"]:
                r.dev["SideflowChanM3"].upload(np.ascontiguousarray(side[r.perm]))
                r.run_sequential(1)
            out = all_vectors(r)
        else:
            sums = []
            for side in model_step_sides(name):
                r.dev["SideflowChanM3"].upload(np.ascontiguousarray(side[r.perm]))
                r.dev["sumDisDay"].zero()
                r.run_sequential(S.NSTEPS)
                sums.append(r.download("sumDisDay"))
            out = (all_vectors(r), sums)
        _reference[key] = out
        r.free()
        kw.close()
    return _reference[key]


def partition(name, split, irregular=False, blocks=None):
    """the blocks of an input on the device (reads LF_FUSED_LEVELS and LF_GENERAL_POW), with the first sideflow vector resident"""
    d, cut = X.inputs(name)
    return X.Partition(d, cut if blocks is None else blocks, S.statics(d, irregular), split, d["sideflows"][0])


def check_planted(name, got, want, split):
    """the partition has no inert skip, the reference has: the inert candidates are as the sequential engine leaves them"""
    if name in X.EDGES:
        S.inert_cells_are_left_alone(X.inputs(name)[0], got, want, split)


# ======================================================================================================================
# 1. the reference against the oracle, on the inputs that tests/test_substep_edges_gpu.py does not hold to it
# ======================================================================================================================
@_split
@pytest.mark.parametrize("name", NEW)
def test_reference_is_close_to_the_oracle(amd, oracle, switches, name, split):
    """lf_routing_substep on the whole raster, engine order, against the C oracle after every sub-step (rtol 1e-9, atol 1e-12,
    NaN positions exact); what it leaves after the last one is the reference of every test below"""
    from lisflood_amd.routing import result_names
    d, _ = X.inputs(name)
    vals = S.statics(d)
    kw, r = whole(amd, d, vals, split, d["sideflows"][0])
    names = result_names(split)
    for s, step in enumerate(S.oracle_run(oracle, d, split, sideflows=[d["sideflows"][0]] * S.NSTEPS)):
        r.run_sequential(1)
        S.close_to_oracle({k: r.download(k) for k in names}, step["after"], names, vals, (name, s))
    got = all_vectors(r)
    r.free()
    kw.close()
    assert_same(got, reference(amd, name, split), name)


# ======================================================================================================================
# 2. sub-step by sub-step
# ======================================================================================================================
SUBSTEP_CASES = [(n, False) for n in X.NAMES] + [(n, True) for n in X.EDGES]


@pytest.mark.parametrize("general", [False, True], ids=["fused_beta_3_5", "general_pow"])
@_split
@pytest.mark.parametrize("name, irregular", SUBSTEP_CASES, ids=["%s%s" % (n, "-irregular" if i else "") for n, i in SUBSTEP_CASES])
def test_substep_by_substep_in_loopback(amd, switches, name, irregular, split, general):
    """dist.loopback_substep: the stage kernels on every block's own cells around the partitioned router calls (level kernel,
    narrow runs, k_sweep_cones_dist; ghost slots behind the state vectors), five times"""
    switches(LF_GENERAL_POW="1" if general else None)
    want = reference(amd, name, split, irregular, general)
    P = partition(name, split, irregular)
    for _ in range(S.NSTEPS):
        amd.dist.loopback_substep(P.steps)
    got = P.all_vectors()
    P.free()
    assert_same(got, want, (name, irregular, split, general))
    check_planted(name, got, want, split)


@_split
@pytest.mark.parametrize("name", X.NAMES)
def test_whole_raster_as_one_block_through_the_composites(amd, switches, name, split):
    """one block that holds everything needs no communicator: lf_dist_routing_substep five times, lf_dist_routing_substeps_fused
    with the resident sideflow vector and (edges) with one vector per sub-step, lf_dist_routing_model_steps_fused"""
    d, _ = X.inputs(name)
    H = d["codes"].shape[0]
    want = reference(amd, name, split)
    P = partition(name, split, blocks=[(0, H)])
    for _ in range(S.NSTEPS):
        P.steps[0].substep()
    got = P.all_vectors()
    P.free()
    assert_same(got, want, (name, "lf_dist_routing_substep"))
    P = partition(name, split, blocks=[(0, H)])
    P.steps[0].substeps_fused(S.NSTEPS)
    got = P.all_vectors()
    assert P.forms()[0] is not None
    P.free()
    assert_same(got, want, (name, "lf_dist_routing_substeps_fused"))
    if name in X.EDGES:
        P = partition(name, split, blocks=[(0, H)])
        P.steps[0].substeps_fused(S.NSTEPS, P.steps[0].N, P.device_rows(d["staggered"])[0])
        got = P.all_vectors()
        P.free()
        assert_same(got, reference(amd, name, split, kind="staggered"), (name, "sideflow_stride = N"))
    want, want_sums = reference(amd, name, split, kind="model_steps")
    P = partition(name, split, blocks=[(0, H)])
    sums, sides = P.zeros(2), P.device_rows(model_step_sides(name))
    P.steps[0].model_steps_fused(S.NSTEPS, 2, sums[0], sides[0])
    got, got_sums = P.all_vectors(), [P.rows(sums, m) for m in range(2)]
    P.free()
    _same_model_steps(got, got_sums, want, want_sums, (name, "lf_dist_routing_model_steps_fused"))


def _same_model_steps(got, got_sums, want, want_sums, what):
    for m in range(2):
        assert E.same_bits(got_sums[m], want_sums[m]), (what, "sum of model step", m, E.first_difference(got_sums[m], want_sums[m]))
    assert_same({k: x for k, x in got.items() if k != "sumDisDay"}, {k: x for k, x in want.items() if k != "sumDisDay"}, what)


# ======================================================================================================================
# 3. the fused forms: every sub-step of a phase as one wavefront, the halo blocks of the slabs between the phases
# ======================================================================================================================
def _fused_run(amd, switches, name, form, split, irregular=False, general=False, no_recompute=False, lanes=False, stride=False):
    """one loopback_substeps_fused call of NSTEPS sub-steps in `form` -> the vectors; asserts the form every block took"""
    at_finalize, at_call, expect = FORMS[form]
    d, _ = X.inputs(name)
    switches(LF_GENERAL_POW="1" if general else None, LF_NO_RECOMPUTE=1 if no_recompute else None, **at_finalize)
    P = partition(name, split, irregular)
    switches(**at_call)
    if stride:
        amd.dist.loopback_substeps_fused(P.steps, S.NSTEPS, lanes, True, P.device_rows(d["staggered"]))
    else:
        amd.dist.loopback_substeps_fused(P.steps, S.NSTEPS, lanes)
    got, forms = P.all_vectors(), P.forms()
    multi = [g.fused_plan() is not None and bool((np.diff(g.fused_plan()["level"]) > 1).any()) for g in P.graphs]
    P.free()
    assert forms == [expect] * len(forms), (name, form, forms)
    if form == "level_blocks":        # k_fused_cones<DIST> ran: every block of every input has a level block of several units
        assert all(multi), (name, multi)
    if form == "levels":
        assert not any(multi), (name, multi)
    return got


FUSED_CASES = [(n, f, g) for n in X.NAMES for f in FORMS for g in (False, True) if not g or n in GENERAL_POW_ON]


@_split
@pytest.mark.parametrize("name, form, general", FUSED_CASES,
                         ids=["%s-%s-%s" % (n, f, "general_pow" if g else "fused_beta_3_5") for n, f, g in FUSED_CASES])
def test_fused_form_equals_sequential(amd, switches, name, form, general, split):
    """time-major (k_fused_level_steps<DIST>), level blocks (k_fused_cones<DIST> and the single levels beside them), levels
    (k_fused_substeps<DIST>): the blocks of a phase one after the other, then on lanes -- the same bits as the reference"""
    want = reference_with(amd, switches, name, split, general=general)
    for lanes in (False, True):
        got = _fused_run(amd, switches, name, form, split, general=general, lanes=lanes)
        assert_same(got, want, (name, form, split, general, "lanes", lanes))
        check_planted(name, got, want, split)


def reference_with(amd, switches, name, split, irregular=False, general=False, kind="resident"):
    switches(LF_GENERAL_POW="1" if general else None)
    return reference(amd, name, split, irregular, general, kind)


@_split
@pytest.mark.parametrize("form", list(FORMS))
def test_fused_form_without_recomputed_statics(amd, switches, form, split):
    """LF_NO_RECOMPUTE=1 on edges_deep: the derived statics streamed instead of recomputed, the same bits"""
    want = reference_with(amd, switches, "edges_deep", split)
    got = _fused_run(amd, switches, "edges_deep", form, split, no_recompute=True)
    assert_same(got, want, (form, split))
    check_planted("edges_deep", got, want, split)


@_split
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", X.EDGES)
def test_fused_form_with_irregular_statics(amd, switches, name, form, split):
    """the irregular statics (ChannelAlpha = 0, an InvChanLength off by an ulp): k_check_derived refuses the recomputation"""
    want = reference_with(amd, switches, name, split, irregular=True)
    got = _fused_run(amd, switches, name, form, split, irregular=True)
    assert_same(got, want, (name, form, split))
    check_planted(name, got, want, split)


@_split
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", X.EDGES)
def test_sideflow_per_substep_equals_sequential(amd, switches, name, form, split):
    """sideflow_stride = N on the partition: the tiny sideflows (case d) arrive in sub-step 1, the negative ones (g) in sub-step
    2, the NaN (n) in sub-step 3 -- the same bits as uploading each vector before its sequential sub-step"""
    want = reference_with(amd, switches, name, split, kind="staggered")
    got = _fused_run(amd, switches, name, form, split, stride=True)
    assert_same(got, want, (name, form, split))
    assert np.isnan(got["ChanQKin"]).sum() == (6 if split else 0)


@_split
@pytest.mark.parametrize("time_major", [1, 0], ids=["time_major", "level_blocks"])
@pytest.mark.parametrize("name", ["edges_deep", "edges_shallow", "seam_3"])
def test_model_steps_in_one_call_equal_sequential(amd, switches, name, time_major, split):
    """loopback_model_steps_fused, 2 model steps x 5 sub-steps in ONE pass over the phases, each model step with its own
    sideflow vector: every state vector and both discharge sums against the whole raster run model step by model step with the
    sum zeroed in between"""
    want, want_sums = reference_with(amd, switches, name, split, kind="model_steps")
    P = partition(name, split)
    switches(LF_FUSED_TIME_MAJOR=time_major)
    sums, sides = P.zeros(2), P.device_rows(model_step_sides(name))
    amd.dist.loopback_model_steps_fused(P.steps, S.NSTEPS, 2, sums, sides)
    got, got_sums, forms = P.all_vectors(), [P.rows(sums, m) for m in range(2)], P.forms()
    P.free()
    assert forms == ["time-major" if time_major else "level blocks"] * len(forms), forms
    _same_model_steps(got, got_sums, want, want_sums, (name, time_major, split))


@_split
@pytest.mark.parametrize("time_major", [1, 0], ids=["time_major", "level_blocks"])
@pytest.mark.parametrize("name", ["edges_shallow", "seam_3"])
def test_slab_stride_larger_than_the_call(amd, switches, name, time_major, split):
    """a model step of 7 sub-steps, then one of 5 on the same steps: the slabs keep their 7 sub-steps per slot, the second call
    uses 5 of them and its halo blocks carry all 7"""
    want = reference_with(amd, switches, name, split, kind="7_then_5")
    P = partition(name, split)
    switches(LF_FUSED_TIME_MAJOR=time_major)
    amd.dist.loopback_substeps_fused(P.steps, 7)
    amd.dist.loopback_substeps_fused(P.steps, 5, lanes=True)
    got, forms = P.all_vectors(), P.forms()
    P.free()
    assert forms == ["time-major" if time_major else "level blocks"] * len(forms), forms
    assert_same(got, want, (name, time_major, split))
