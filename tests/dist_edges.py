"""Inputs and cuts that send the routing sub-step on the ROW-BLOCK PARTITION (csrc/lf_dist.hip: lf_dist_routing_substep, the
fused forms, their slabs and halo blocks) through the branch edges of tests/substep_edges.py and through cuts of every shape: a
census of what crosses the cuts from the graphs alone, the condition under which the fused kernels read a cell's upstream
cells as a run instead of from its list, and what tests/test_dist_edges_gpu.py needs to build a partition on one device.  A
plain helper module: tests/test_dist_edges_cpu.py asserts the census and the table invariant and pins the oracle for the new
inputs, tests/test_dist_edges_gpu.py runs every input through every form of the sub-step on the partition.

Inputs (all in the dict shape of substep_edges.substep_inputs, so its statics / oracle_run / substep_reference apply):
  edges_deep, edges_shallow   substep_inputs(True, 5, family) unchanged, cut where most planted cells drain across a cut;
  fans, fans_masked           route_edges' main_shallow(_masked) raster, one-row blocks on rows of star centres: a centre of
                              in-degree 8 then has 3 ghosts above, 2 cells of its own row and 3 ghosts below; random values, the
                              discharges of the cells feeding those centres spread over 2^+-12 so that the order of the sum shows;
  seam_0, seam_3, seam_20     the 4 x 4 raster below (+ k rows), blocks (0, 2) and (2, 4 + k): the pit at local (1, 1) of the second
                              block has its upstream cells at CONSECUTIVE positions of two phases -- the last cell of phase 0 and
                              the first of phase 1 --, a run in the layout that is no run of one phase.  Random values, and on
                              the three cells that drain across the cut a NaN, a -0.0 and a beyond-fast-range discharge.
"""
import itertools

import numpy as np

import substep_edges as S

SEED = 5
SEAM = np.array([[5, 5, 5, 5],
                 [5, 5, 2, 5],
                 [8, 2, 1, 8],
                 [8, 5, 7, 8]], np.uint8)
SEAM_ROWS = (0, 3, 20)
SEAM_PLANTED = {"nan": (2, 0), "minus_zero": (1, 2), "huge": (2, 3)}    # (row, column): the three cells that drain across the cut
NAMES = ("edges_deep", "edges_shallow", "fans", "fans_masked") + tuple("seam_%d" % k for k in SEAM_ROWS)
EDGES = NAMES[:2]
FAN_CUTS = [1, 28, 29, 85, 86]          # one-row blocks: row 0 (the northern neighbours of the centres of row 1), rows 28 and 85
SPREAD = 12                             # the discharges feeding the centres on cut rows: times 2^U(-SPREAD, SPREAD)
FRONT_ROWS, BACK_ROWS = range(3, 10), range(87, 94)
MAX_CUTS, MAX_BLOCKS = 5, 6


def seam_codes(k):
    """the seam raster with k rows below: columns 0, 2 and 3 drain north, column 1 south (its last cell is the pit)"""
    codes = np.concatenate([SEAM, np.tile(np.array([8, 2, 8, 8], np.uint8), (k, 1))])
    if k:
        codes[3, 1] = 2
        codes[-1, 1] = 5
    return codes


# ---- the graph of an input in pixel ids ------------------------------------------------------------------------------
def topology(d):
    """-> dict: down [N] (pixel id, -1: pit), row [N] (raster row of a pixel), ups (list of ascending arrays)"""
    if "topology" not in d:
        m = d["mask"].reshape(-1)
        pid = np.cumsum(m) - 1
        dn = S.downstream(d["codes"])
        assert m[dn[m & (dn >= 0)]].all()                  # no cell drains into a missing value
        down = np.where(dn[m] >= 0, pid[np.maximum(dn[m], 0)], -1)
        N = down.size
        order = np.argsort(down, kind="stable")
        starts = np.searchsorted(down[order], np.arange(N + 1))
        d["topology"] = dict(down=down, row=np.flatnonzero(m) // d["codes"].shape[1], ups=[order[starts[p]:starts[p + 1]] for p in range(N)])
    return d["topology"]


def blocks_of(H, cuts):
    edges = [0] + list(cuts) + [H]
    return list(zip(edges[:-1], edges[1:]))


def block_census(d, blocks):
    """what crosses the cuts, from the raster alone -> dict: block [N], exports [N] bool (the downstream cell lies in another
    block), above / local / below [N] (upstream cells in the block above, in the cell's own, in the block below)"""
    t = topology(d)
    down, row = t["down"], t["row"]
    block = np.searchsorted([r1 for _, r1 in blocks], row, side="right")
    link = down >= 0
    exports = np.zeros(down.size, bool)
    exports[link] = block[down[link]] != block[link]
    cnt = lambda sel: np.bincount(down[link & sel], minlength=down.size)
    db = np.zeros(down.size, np.int64)
    db[link] = block[link] - block[down[link]]             # -1: the cell lies in the block above its downstream cell
    return dict(block=block, exports=exports, above=cnt(db == -1), local=cnt(db == 0), below=cnt(db == 1))


def search_cuts(d):
    """at most MAX_CUTS cuts among the rows around the planted cells (FRONT_ROWS, BACK_ROWS) with a block one row high, such
    that as many planted cells as possible drain into another block; of equal sets the first in the order of
    itertools.combinations.  (A cell's downstream cell lies in its own or a neighbouring row, so it drains across cut r iff the
    lower of the two rows is r: the score of a set of cuts is a sum over its cuts.)"""
    t = topology(d)
    planted = np.array(sorted(p for cells in d["cells"].values() for p in cells))
    dn = t["down"][planted]
    ok = dn >= 0
    r0, r1 = t["row"][planted[ok]], t["row"][dn[ok]]
    crossing = np.maximum(r0, r1)[r0 != r1]
    weight = np.bincount(crossing, minlength=d["codes"].shape[0] + 1)
    rows = list(FRONT_ROWS) + list(BACK_ROWS)
    best, best_cuts = -1, None
    for n in range(2, MAX_CUTS + 1):
        for cuts in itertools.combinations(rows, n):
            if not any(b - a == 1 for a, b in zip(cuts[:-1], cuts[1:])):
                continue
            score = int(weight[list(cuts)].sum())
            if score > best:
                best, best_cuts = score, list(cuts)
    return best_cuts


# ---- inputs ----------------------------------------------------------------------------------------------------------
def random_inputs(name, codes, mask, seed, spread_cells=()):
    """random values as test_dist_fused_gpu._case makes them (synthetic.router_params / model_step_values, 10 % of the cells no
    kinematic channel), the discharge capped and the run's scalars as substep_inputs has them, the two discharges of
    `spread_cells` multiplied by 2^U(-SPREAD, SPREAD) (the volumes follow)"""
    from lisflood_amd import synthetic as syn
    N = int(mask.sum())
    rng = np.random.default_rng(seed)
    p = syn.router_params(N, seed=seed + 1)
    p["Q0"] = np.minimum(p["Q0"], 400.0)                   # see substep_inputs: ChanQ must stay a well-conditioned difference
    v, _ = syn.model_step_values(N, p, seed=seed + 2)
    v = {k: np.array(a, copy=True) for k, a in v.items()}
    del v["SideflowChanM3"]
    v["IsChannelKinematic"] = rng.random(N) < 0.9
    for k in ("CrossSection2Area", "Sideflow1Chan", "ChanQ"):
        v[k] = np.zeros(N)
    v["sumDisDay"] = rng.uniform(0.0, 3.0, N)
    cells = np.asarray(sorted(spread_cells), np.int64)
    if cells.size:
        for q, m3, alpha in (("ChanQKin", "ChanM3Kin", "ChannelAlpha"), ("Chan2QKin", "Chan2M3Kin", "ChannelAlpha2")):
            v[q][cells] *= 2.0 ** rng.uniform(-SPREAD, SPREAD, cells.size)
            v[m3][cells] = v[alpha][cells] * v["ChanLength"][cells] * v[q][cells] ** S.BETA
    side = np.stack([syn.lateral_inflow(N, 50 * seed + s) for s in range(S.NSTEPS)])
    d = dict(family=name, seed=seed, split=True, codes=codes, mask=mask, vals=v, irregular={}, cells={}, nan_cells=[], inert_cells={},
             sideflows=side * (v["ChanLength"] * S.DT)[None, :], Beta=S.BETA, DtRouting=S.DT, NoRoutSteps=S.NSTEPS)
    t = topology(d)
    has_ups = np.array([u.size > 0 for u in t["ups"]])
    d.update(down=t["down"], has_ups=has_ups, isolated=~has_ups & (t["down"] < 0))
    return d


def fan_centres(g, cuts):
    """the star centres of a route_edges graph on the one-row blocks of `cuts` -> (centre pixel, its upstream pixels) each"""
    rows = [a for a, b in blocks_of(g["H"], cuts) if b - a == 1]
    raster = np.flatnonzero(g["mask"].reshape(-1))
    return [(st["centre"], st["ups"]) for st in g["sites"] if raster[st["centre"]] // g["W"] in rows]


_inputs = {}


def inputs(name):
    """-> (the input dict, its row blocks)"""
    if name not in _inputs:
        if name in EDGES:
            d = S.substep_inputs(True, SEED, name[6:])
            cuts = search_cuts(d)
        elif name.startswith("fans"):
            import route_edges as R
            g = R.build_graph("main_shallow" + name[4:])
            cuts = FAN_CUTS
            feeders = sorted(set(u for _, ups in fan_centres(g, cuts) for u in ups))
            d = random_inputs(name, g["codes"], g["mask"], SEED, feeders)
            d["centres"] = fan_centres(g, cuts)
        else:
            codes = seam_codes(int(name[5:]))
            d = random_inputs(name, codes, np.ones(codes.shape, bool), SEED)
            cuts = [2]
            # a NaN and a beyond-fast-range discharge one cell above a pit of the first block, a -0.0 at the head of the flow
            # path through the seam cell: states the edges inputs have on planted cells that drain nowhere
            v, where = d["vals"], {k: r * codes.shape[1] + c for k, (r, c) in SEAM_PLANTED.items()}
            v["IsChannelKinematic"][list(where.values())] = True
            v["ChanQKin"][where["nan"]], v["ChanQKin"][where["minus_zero"]] = np.nan, -0.0
            v["ChanQKin"][where["huge"]] = S.HUGE_Q
            v["ChanM3Kin"][where["huge"]] = v["ChannelAlpha"][where["huge"]] * v["ChanLength"][where["huge"]] * S.HUGE_Q ** S.BETA
            d["planted"] = where
        _inputs[name] = (d, blocks_of(d["codes"].shape[0], cuts))
        assert len(cuts) <= MAX_CUTS and d["codes"].shape[0] <= 96 and d["codes"].shape[1] <= 80
    return _inputs[name]


def order_sensitive(addends):
    """does some other order of the same addends give another double than their sum from the left?"""
    x = [float(a) for a in addends]
    left = lambda seq: float(np.add.accumulate(np.asarray(seq, np.float64))[-1])
    want = left(x)
    orders = itertools.permutations(x) if len(x) <= 6 else (np.random.default_rng(i).permutation(x) for i in range(200))
    return any(left(list(o)) != want for o in orders)


# ---- the partition's graphs (host only) ------------------------------------------------------------------------------
def block_slices(d, blocks):
    """the pixel range of every row block"""
    first = np.concatenate([[0], np.cumsum(d["mask"].sum(axis=1))])
    return [slice(int(first[r0]), int(first[r1])) for r0, r1 in blocks]


def make_graphs(d, blocks):
    """the settled DistGraphs of the blocks; the masks go in where the raster has missing values"""
    from lisflood_amd import dist as D
    codes, H = d["codes"], d["codes"].shape[0]
    m = None if d["mask"].all() else d["mask"]
    row = lambda a, r: None if a is None or r < 0 or r >= H else a[r]
    graphs = [D.DistGraph(codes[r0:r1], None if m is None else m[r0:r1], row(codes, r0 - 1), row(m, r0 - 1), row(codes, r1), row(m, r1))
              for r0, r1 in blocks]
    D.settle_phases_local(graphs)
    return graphs


def short_way(g):
    """[N] bool by position: the DIST instantiations of k_fused_substeps, k_fused_cones and k_fused_level_steps read the cell's
    upstream cells as the run [base, base + count) of the parity buffers / LDS / history: base >= 0 && base + count <= n, on
    the table the routers upload"""
    base = g.ups_base().astype(np.int64)
    count = np.diff(g.csr()[0]).astype(np.int64)
    return (base >= 0) & (base + count <= g.num_pixels)


def table_census(g):
    """by position, from the fused tables: `short` (short_way), `local_run` (every entry of ups_idx_f is a same-phase position
    and they are consecutive), `mixed` (same-phase positions and slab slots together), `seam` (consecutive positions in the
    per-call list that are not of one phase)"""
    ups_ptr, ups_idx = g.csr()
    idx_f = g.fused_tables()[1]
    n = g.num_pixels
    short = short_way(g)
    local_run, mixed, seam = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    for p in range(n):
        a, b = int(ups_ptr[p]), int(ups_ptr[p + 1])
        e, f = ups_idx[a:b].astype(np.int64), idx_f[a:b].astype(np.int64)
        run = lambda x: bool((x == x[0] + np.arange(x.size)).all()) if x.size else True
        local_run[p] = bool((f >= 0).all()) and run(f)
        mixed[p] = bool((f >= 0).any() and (f < 0).any())
        seam[p] = e.size > 0 and run(e) and int(e[-1]) < n and bool((f < 0).any())
    return dict(short=short, local_run=local_run, mixed=mixed, seam=seam)


# ---- the partition on one device (tests/test_dist_edges_gpu.py) ------------------------------------------------------
class Partition:
    """the blocks of an input on one device: graphs, routers and DistRoutingSteps; free() releases all of it"""

    def __init__(self, d, blocks, vals, split, sideflow, nsteps=S.NSTEPS, beta=S.BETA):
        from lisflood_amd import dist as D
        assert len(blocks) <= MAX_BLOCKS
        self.slices = block_slices(d, blocks)
        self.graphs = make_graphs(d, blocks)
        self.routers = [D.DistRouter(g, vals["ChannelAlpha"][s], beta, vals["ChanLength"][s], S.DT, alpha_floodplains=vals["ChannelAlpha2"][s])
                        for g, s in zip(self.graphs, self.slices)]
        self.steps = [D.DistRoutingStep(r, dict({k: a[s] for k, a in vals.items()}, SideflowChanM3=sideflow[s]), split, beta, 1.0 / S.DT,
                                        S.DT * nsteps) for r, s in zip(self.routers, self.slices)]
        self.arrays = []

    def device_rows(self, rows):
        """rows [M, N] in pixel order -> per block a device array [M, N_k] in the block's engine order"""
        from lisflood_amd._lib import DeviceArray
        out = [DeviceArray.from_host(np.ascontiguousarray(np.stack([r[s][st.perm] for r in rows]))) for st, s in zip(self.steps, self.slices)]
        self.arrays += out
        return out

    def zeros(self, m):
        from lisflood_amd._lib import DeviceArray
        out = [DeviceArray((m, st.N)).zero() for st in self.steps]
        self.arrays += out
        return out

    def upload(self, name, x):
        for st, s in zip(self.steps, self.slices):
            st.dev[name].upload(np.ascontiguousarray(x[s][st.perm]), prefix=True)

    def download(self, name):
        return np.concatenate([st.download(name) for st in self.steps])

    def rows(self, arrays, m):
        """row m of per-block [M, N_k] engine-order device arrays -> [N] pixel order"""
        out = []
        for st, a in zip(self.steps, arrays):
            row = np.empty(st.N)
            row[st.perm] = a.download()[m]
            out.append(row)
        return np.concatenate(out)

    def all_vectors(self):
        from lisflood_amd.routing import _OUT, _STATE
        return {k: self.download(k) for k in _STATE + _OUT}

    def forms(self):
        return [r.last_fused_form() for r in self.routers]

    def free(self):
        for a in self.arrays:
            a.free()
        for st in self.steps:
            st.free()
        for r in self.routers:
            r.close()
        for g in self.graphs:
            g.close()
        self.arrays, self.steps, self.routers, self.graphs = [], [], [], []
