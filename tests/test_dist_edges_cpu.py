"""What tests/test_dist_edges_gpu.py relies on, without a device (tests/dist_edges.py): the census of what crosses the cuts of
every input, from the graphs and the values alone; the invariant that ties the table by which the fused kernels of the row-block
partition choose between a run and the list (ups_base) to the list itself (ups_idx_f), read from the very tables the routers
upload; and the oracle pinned bit for bit to the restatement of the sub-step on the inputs that tests/substep_edges.py does not
already pin."""
import numpy as np
import pytest

import dist_edges as X
import module_edges as E
import substep_edges as S

NEW = [n for n in X.NAMES if n not in X.EDGES]
_graphs, _runs = {}, {}


def graphs(name):
    if name not in _graphs:
        _graphs[name] = X.make_graphs(*X.inputs(name))
    return _graphs[name]


def run(oracle, name, split):
    """-> per sub-step (the oracle's step, the restatement's outputs, its intermediates)"""
    if (name, split) not in _runs:
        d, _ = X.inputs(name)
        ref = S.reference_scalars(S.statics(d), S.BETA)
        out = []
        for step in S.oracle_run(oracle, d, split):
            want, mid = S.substep_reference(ref, step["before"], step["side"], split, step["qr1"], step["qr2"])
            out.append((step, want, mid))
        _runs[name, split] = out
    return _runs[name, split]


def planted_exports(d, c):
    cases = [k for k, cells in d["cells"].items() if c["exports"][cells].any()]
    return len(cases), sum(int(c["exports"][cells].sum()) for cells in d["cells"].values())


@pytest.mark.parametrize("name", X.NAMES)
def test_census_of_what_crosses_the_cuts(name):
    """the cuts are where the inputs need them: planted cells and a NaN drain into another block (edges), cells have ghosts and
    local upstream cells together, ghosts on both sides, six ghosts (shallow), an in-degree of 8 as 3 ghosts above + 2 cells of
    the row + 3 ghosts below (fans), a block is one row high, an inner block sends and receives; the seams have their one cell"""
    d, blocks = X.inputs(name)
    c = X.block_census(d, blocks)
    gs = graphs(name)
    ghosts = c["above"] + c["below"]
    tables = [X.table_census(g) for g in gs]
    census = {
        "blocks": len(blocks), "blocks one row high": sum(1 for a, b in blocks if b - a == 1), "phases": gs[0].num_phases,
        "cells that drain into another block": int(c["exports"].sum()),
        "cells with ghost and local upstream cells": int(((ghosts > 0) & (c["local"] > 0)).sum()),
        "cells with ghosts on both sides": int(((c["above"] > 0) & (c["below"] > 0)).sum()),
        "most ghosts of a cell": int(ghosts.max()),
        "in-degree 8 as 3 + 2 + 3": int(((c["above"] == 3) & (c["local"] == 2) & (c["below"] == 3)).sum()),
        "cells whose list mixes same-phase positions and slab slots": sum(int(t["mixed"].sum()) for t in tables),
        "cells that take the short way": sum(int(t["short"].sum()) for t in tables),
        "consecutive positions that are not of one phase": sum(int(t["seam"].sum()) for t in tables),
        "exports upward": sum(g.n_export[0] for g in gs), "exports downward": sum(g.n_export[1] for g in gs),
    }
    if d["cells"]:
        census["planted cases that export"], census["planted cells that export"] = planted_exports(d, c)
        census["NaN cells that export"] = sum(1 for p in d["nan_cells"] if c["exports"][p])
    print("\n" + E.counts_table("%s, blocks %s" % (name, blocks), census))
    assert len(blocks) <= X.MAX_BLOCKS and all(g.num_phases == gs[0].num_phases for g in gs)
    assert sum(g.n_export[0] + g.n_export[1] for g in gs) == census["cells that drain into another block"]
    if name.startswith("seam"):
        assert census["consecutive positions that are not of one phase"] == 1 and census["phases"] == 2
        # ... in the second block: a cell of phase 1 whose first upstream cell is the last of phase 0 (a slab slot) and whose
        # second is the first of phase 1, in a unit behind the first of a level block of several units
        g, t = gs[1], tables[1]
        assert not tables[0]["seam"].any()
        # the planted NaN, -0.0 and beyond-fast-range discharge sit on the three cells that drain across the cut
        assert sorted(d["planted"].values()) == np.flatnonzero(c["exports"]).tolist()
        q = d["vals"]["ChanQKin"]
        assert np.isnan(q[d["planted"]["nan"]]) and np.signbit(q[d["planted"]["minus_zero"]]) and q[d["planted"]["minus_zero"]] == 0
        h = d["planted"]["huge"]
        assert d["vals"]["ChannelAlpha"][h] * d["vals"]["ChanLength"][h] / S.DT * q[h] ** S.BETA > 1e30     # beyond lf_fast_range
        p = int(np.flatnonzero(t["seam"])[0])
        ups_ptr, ups_idx = g.csr()
        phase = g.layout()[1]
        u = ups_idx[ups_ptr[p]:ups_ptr[p + 1]]
        assert phase[p] == 1 and phase[u].tolist() == [0, 1] and u[1] == u[0] + 1 == g.phase_range(1)[0]
        f = g.fused_tables()[1][ups_ptr[p]:ups_ptr[p + 1]]
        assert f[0] < 0 and f[1] == u[1]
        plan = g.fused_plan()
        unit = int(np.searchsorted(plan["level_start"], p, side="right")) - 1
        b = int(np.searchsorted(plan["level"], unit, side="right")) - 1
        assert plan["level"][b] < unit < plan["level"][b + 1], (unit, plan["level"])
        return
    assert census["blocks one row high"] >= 1
    inner = [g for g in gs[1:-1] if sum(g.n_export) > 0 and sum(g.n_ghost) > 0
             and all(g.n_export[s] + g.n_ghost[s] > 0 for s in (0, 1))]
    assert inner, [(g.n_export, g.n_ghost) for g in gs]
    if name == "edges_deep":
        assert census["planted cases that export"] >= 24 and census["planted cells that export"] >= 42
        assert census["NaN cells that export"] >= 1 and census["phases"] >= 4
    elif name == "edges_shallow":
        assert census["planted cases that export"] >= 19 and census["planted cells that export"] >= 21
        assert census["cells with ghost and local upstream cells"] >= 50 and census["cells with ghosts on both sides"] >= 5
        assert census["most ghosts of a cell"] >= 6
        assert census["exports upward"] > 0 and census["exports downward"] > 0
        assert any(min(g.n_export) > 0 and min(g.n_ghost) > 0 for g in gs[1:-1])
    else:
        assert census["in-degree 8 as 3 + 2 + 3"] >= 1
        assert (name == "fans") == bool(d["mask"].all())


def test_some_input_has_four_phases():
    assert max(graphs(name)[0].num_phases for name in X.NAMES) >= 4


@pytest.mark.parametrize("name", X.NAMES)
def test_short_way_only_for_runs_of_the_own_phase(name):
    """Every block, every position: where the fused kernels read the upstream cells as a run (ups_base >= 0 and the run ends
    inside the local cells), every entry of the cell's fused list is a same-phase position; and a list of consecutive
    same-phase positions is read as a run.  (Before ups_base took the phases into account this failed on the three seams --
    position 7, 16 and 67 of their second block -- and nowhere else.)"""
    for k, g in enumerate(graphs(name)):
        t = X.table_census(g)
        wrong = np.flatnonzero(t["short"] & ~t["local_run"])
        assert wrong.size == 0, (name, "block", k, "positions that would read a slab value from the parity buffers", wrong[:8])
        missed = np.flatnonzero(t["local_run"] & ~t["short"])
        assert missed.size == 0, (name, "block", k, "runs that go through the list", missed[:8])
        # the table is the one the list-driven CPU executor does not look at: where it says run, the run is the list
        ups_ptr, _ = g.csr()
        idx_f, base = g.fused_tables()[1], g.ups_base()
        for p in np.flatnonzero(t["short"]):
            a, b = ups_ptr[p], ups_ptr[p + 1]
            assert (idx_f[a:b] == base[p] + np.arange(b - a)).all(), (name, k, p)


@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
@pytest.mark.parametrize("name", NEW)
def test_oracle_is_the_reference_lines_on_the_new_inputs(oracle, name, split):
    """every state and output vector after each sub-step has the bits of the restatement driven with the oracle's own router
    outputs, and at most 1 % of the cells have a ChanQ too ill-conditioned for the tolerance of the GPU file"""
    d, _ = X.inputs(name)
    names = S.STATE + S.OUT if split else ["ChanQKin", "ChanM3Kin", "ChanQ", "sumDisDay"] + S.OUT
    ill = []
    for s, (step, want, mid) in enumerate(run(oracle, name, split)):
        for k in names:
            assert E.same_bits(step["after"][k], want[k]), "%s: %s" % ((s, k), E.first_difference(step["after"][k], want[k]))
        ill.append(S.substep_conditioning(mid, step["after"]))
        nan = np.flatnonzero(np.isnan(step["after"]["ChanQKin"]))        # the planted NaN and the pit below it, nothing else
        p = d.get("planted", {}).get("nan")
        assert nan.tolist() == ([] if p is None else sorted([p, int(d["down"][p])])), nan
    print("\n%s, %s: ill-conditioned ChanQ per sub-step %s of %d cells" % (name, "split" if split else "single", ill, d["mask"].sum()))
    assert max(ill) <= d["mask"].sum() // 100, ill


@pytest.mark.parametrize("name", ["fans", "fans_masked"])
def test_the_sums_of_the_centres_on_cut_rows_depend_on_their_order(oracle, name):
    """at least half of the star centres on one-row blocks with three or more upstream cells sum discharges (the oracle's
    ChanQKin after the first sub-step) that give another double in some other order"""
    d, _ = X.inputs(name)
    q = run(oracle, name, True)[0][0]["after"]["ChanQKin"]
    many = [(c, ups) for c, ups in d["centres"] if len(ups) >= 3]
    sensitive = sum(1 for _, ups in many if X.order_sensitive(q[ups]))
    print("\n%s: %d of %d centres on cut rows with >= 3 upstream cells are order-sensitive" % (name, sensitive, len(many)))
    assert len(many) >= 20 and 2 * sensitive >= len(many), (sensitive, len(many))
