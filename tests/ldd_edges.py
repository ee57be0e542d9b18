"""Inputs, restatements and censuses for the LDD reductions and labellings -- accuflux (k_accu_level, k_accu_narrow,
k_accu_cones in csrc/lf_router.hip), the one-hop upstream sum (k_upstream_sum, k_upstream_sum_raster), lddrepair / lddmask,
downstream, subcatchment / catchment by pointer jumping and the catchment totals (csrc/lf_ldd.hip).  A plain helper module:
tests/test_ldd_edges_cpu.py shows without a GPU that the inputs are what they claim and that the restatements are right,
tests/test_ldd_edges_gpu.py holds every kernel to the restatements bit for bit.

Every one of these operations is additions in a documented order or integer logic, so the restatements below are plain
Python walks -- one IEEE addition, one rounding, per `+` -- and nothing is compared to a tolerance.  The graphs, their
topology (from the raster alone), the engine's layout and the launch regions are those of tests/route_edges.py (DESIGN.md
section 4.1.1); three rasters of single-column chains are added for pointer jumping and registered beside them.
"""
import math

import numpy as np

import route_edges as E
from module_edges import spots

U = 2.0 ** -53
BIG = E.BIG
NVS = (1, 2, 3, 4)
# levels per chunk of k_accu_cones<NV, CW>: 49152 / (CW (8 + 8 NV)), at least 2 and at most 64
LC = {cw: {nv: max(2, min(64, 49152 // (cw * (8 + 8 * nv)))) for nv in NVS} for cw in (64, 256)}
assert LC == {64: {1: 48, 2: 32, 3: 24, 4: 19}, 256: {1: 12, 2: 8, 3: 6, 4: 4}}


def gamma(k):
    """the bound of recursive summation: k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


# ---- launch configurations -------------------------------------------------------------------------------------------
# route_edges.CONFIGS, LF_ROUTE_LEVELS = LC and LC + 1 of every NV at 64, and the same at 256 (the issue names 4, 5, 12, 13
# there; 6 .. 9 give NV = 2 and 3 their one-chunk and chunk-plus-one blocks too)
CONFIGS = {k: dict(v) for k, v in E.CONFIGS.items()}
for _n in (19, 20, 24, 25, 32, 33, 48, 49):
    CONFIGS["levels%d" % _n] = dict(env={"LF_ROUTE_LEVELS": str(_n)}, lmax=_n, wide=E.DEFAULT_WIDE, cw=64)
for _n in (4, 5, 6, 7, 8, 9, 12, 13):
    CONFIGS["cones256_levels%d" % _n] = dict(env={"LF_ROUTE_CONE_WIDTH": "256", "LF_ROUTE_LEVELS": str(_n)}, lmax=_n,
                                             wide=E.DEFAULT_WIDE, cw=256)
CONE_GRAPHS = ["fan3", "fan8", "main_deep", "main_shallow", "many", "main_deep_masked", "main_shallow_masked"]
DEEP = ("main_deep", "main_deep_masked")      # 87 levels: the graphs that have every chunk shape and inflow path


def blocks(name, config):
    """[(first level, levels)] of the level blocks of a configuration, None for one launch per level"""
    cfg = CONFIGS[config]
    if cfg["lmax"] == 0:
        return None
    reg, nb = E.regions(E.layout_of(name)[2], cfg["lmax"], cfg["wide"])
    first = np.flatnonzero((reg == "top") | (reg == "wide"))
    assert first.size == nb
    return [(int(k), int(n)) for k, n in zip(first, np.diff(np.r_[first, reg.size]))]


def launches(name, config):
    """-> (launches of one accuflux sweep, of them one-level launches): a launch per block where a block has several
    levels, else (no plan) a launch per level above 1024 cells and per run of narrower ones"""
    b = blocks(name, config)
    if b is not None and any(nl > 1 for _, nl in b):
        return len(b), sum(nl == 1 for _, nl in b)
    reg, _ = E.regions(E.layout_of(name)[2], 0, E.SEGMENT_WIDE)
    wide = int((reg == "wide").sum())
    return wide + int(((reg == "narrow") & np.r_[True, reg[:-1] != "narrow"]).sum()), wide


def chunk_shapes(name, config, nv):
    """blocks of several levels by chunk shape: nl == LC (one full chunk), nl == LC + 1 (a full chunk and a ragged one of one
    level), nl > LC (several chunks), and among those the ones whose LAST chunk has one level"""
    b = blocks(name, config)
    lc = LC[CONFIGS[config]["cw"]][nv]
    nls = [nl for _, nl in b or [] if nl > 1]
    return dict(eq=sum(nl == lc for nl in nls), plus1=sum(nl == lc + 1 for nl in nls), gt=sum(nl > lc for nl in nls),
                ragged1=sum(nl > lc and nl % lc == 1 for nl in nls), below=sum(nl < lc for nl in nls))


def claimed_shapes(config, nv):
    """the chunk shapes a (configuration, NV) is there for, on the 87 levels of main_deep"""
    cfg = CONFIGS[config]
    if cfg["lmax"] == 0 or cfg["wide"] != E.DEFAULT_WIDE:      # (LF_FUSED_WIDE=100 cuts the blocks where the levels are wide)
        return ()
    lc = LC[cfg["cw"]][nv]
    return ("eq",) if cfg["lmax"] == lc else (("plus1", "gt") if cfg["lmax"] == lc + 1 else (("gt",) if cfg["lmax"] > lc + 1 else ()))


def nan_levels(name, config, nv):
    """inflow path -> level k whose first cell gets the NaN: the level after k is "mid" (inside a chunk: inflow from the
    chunk's LDS rows), "chunk" (the first level of a later chunk: inflow from PREV) or "block" (the first level of a later
    block of several levels: inflow read from memory).  "mid" is the middle of the first chunk of the first such block, the
    others the first level of their kind; {} without level blocks."""
    cfg, out = CONFIGS[config], {}
    b = blocks(name, config)
    if b is None or not any(nl > 1 for _, nl in b):
        return out
    lc = LC[cfg["cw"]][nv]
    for k0, nl in b:
        if nl == 1:
            continue
        out.setdefault("mid", k0 + max(1, min(nl - 1, lc) // 2) - 1)
        for j in range(nl):
            if k0 + j and (j == 0 or j % lc == 0):
                out.setdefault("block" if j == 0 else "chunk", k0 + j - 1)
    return out


# ---- graphs ----------------------------------------------------------------------------------------------------------
def _lengths(top):
    return [1, 2, 3, 4, 5] + [2 ** e + d for e in range(3, top + 1) for d in (-1, 0, 1)]


# single-column chains draining south, column c a chain of L_c land cells under missing values
CHAINS = {"chains_full": _lengths(10), "chains_half": _lengths(9), "chains_tiny": [1, 2, 1, 1, 2, 2, 1]}


def _build_chains(name):
    lengths = CHAINS[name]
    H, W = max(lengths), len(lengths)
    codes, mask = np.full((H, W), 5, np.uint8), np.zeros((H, W), bool)
    for c, L in enumerate(lengths):
        mask[H - L:, c] = True
        codes[H - L:H - 1, c] = 2
    return dict(name=name, codes=codes, mask=mask, sites=[], H=H, W=W, N=int(mask.sum()), lengths=lengths)


def graph(name):
    """route_edges.graph, the chain rasters registered beside its graphs (so that topology and layout_of serve them too)"""
    if name in CHAINS and name not in E._graphs:
        E._graphs[name] = _build_chains(name)
    return E.graph(name)


def chain_cell(g, c, i):
    """pixel id of the cell i below the head of chain c (i = L - 1: its pit)"""
    pid = np.cumsum(g["mask"].reshape(-1)) - 1
    return int(pid[(g["H"] - g["lengths"][c] + i) * g["W"] + c])


def lists(g):
    """(down, ups, order upstream first) as Python lists"""
    if "lists" not in g:
        down, ups, dist = E.topology(g)
        g["lists"] = (down.tolist(), [u.tolist() for u in ups], np.argsort(-dist, kind="stable").tolist())
    return g["lists"]


def positions(name):
    perm = E.layout_of(name)[0]
    pos = np.empty(perm.size, np.int64)
    pos[perm] = np.arange(perm.size)
    return pos


_linked = {}


def linked_graph():
    """main_shallow with two feeders of some confluences cut off (they become pits) and tied back by zero-length structure
    links (Graph(virtual_down=...)): dict(codes [N] float64 of the cut LDD, mask, vd [N], down / ups of the CUT LDD, layout,
    linked [N] by position)"""
    if not _linked:
        from lisflood_amd.kinematic_wave_parallel import Graph
        g = E.graph("main_shallow")
        assert g["mask"].all()
        codes, vd = g["codes"].copy().reshape(-1), np.full(g["N"], -1, np.int64)
        picked = [st for st in g["sites"] if st["role"] in ("top", "mid") and st["indeg"] >= 3][::7]
        for st in picked:
            for u in st["ups"][:2]:
                codes[u], vd[u] = 5, st["centre"]
        cut = dict(name="linked", codes=codes.reshape(g["H"], g["W"]), mask=g["mask"], sites=[], H=g["H"], W=g["W"], N=g["N"])
        G = Graph(codes.astype(np.float64), g["mask"], virtual_down=vd)
        cut.update(vd=vd, layout=G.layout() + (G.max_upstream,), linked=G.links(), structures=len(picked))
        G.close()
        E.topology(cut)
        _linked.update(cut)
    return _linked


# ---- the restatements ------------------------------------------------------------------------------------------------
def restated_accuflux(g, x):
    """level by level from the headwaters; per cell s = 0.0, s += acc[u] over the upstream cells in ascending pixel id, then
    acc = s + x: sequential IEEE additions, one rounding each"""
    down, ups, order = lists(g)
    xs, acc = np.asarray(x, np.float64).tolist(), [0.0] * g["N"]
    for p in order:
        s = 0.0
        for u in ups[p]:
            s = s + acc[u]
        acc[p] = s + xs[p]
    return np.array(acc, np.float64)


def exact_accuflux(g, x, got):
    """math.fsum of x over every cell's whole upstream tree -> (that sum, |got - sum| with the difference taken inside fsum --
    rounded once, where the rounded sum alone is up to half an ulp off --, fsum of |x| over the tree, tree size)"""
    down, ups, order = lists(g)
    xs = np.asarray(x, np.float64).tolist()
    N = g["N"]
    members, total, err, mass, size = [None] * N, np.empty(N), np.empty(N), np.empty(N), np.empty(N, np.int64)
    gs = np.asarray(got, np.float64).tolist()
    for p in order:
        m = [xs[p]]
        for u in ups[p]:
            m += members[u]
            members[u] = None
        members[p] = m
        mass[p], size[p] = math.fsum(abs(v) for v in m), len(m)
        finite = math.isfinite(mass[p])                                     # (the bound is for finite inputs)
        total[p] = math.fsum(m) if finite else math.nan
        err[p] = abs(math.fsum(m + [-gs[p]])) if finite else math.nan
    return total, err, mass, size


def restated_upstream(g, x):
    """the one-hop sum over the upstream cells in ascending pixel id, started from 0.0"""
    down, ups, order = lists(g)
    xs, out = np.asarray(x, np.float64).tolist(), [0.0] * g["N"]
    for p in range(g["N"]):
        s = 0.0
        for u in ups[p]:
            s = s + xs[u]
        out[p] = s
    return np.array(out, np.float64)


def restated_downstream(g, x):
    """a copy of the downstream cell's value; a pit reads itself"""
    down = lists(g)[0]
    x = np.asarray(x)
    out = x.copy()
    for p in range(g["N"]):
        if down[p] >= 0:
            out[p] = x[down[p]]
    return out


def restated_subcatchment(g, points):
    """the first non-zero point on the walk downstream, the cell itself included; 0 without one"""
    down, pts = lists(g)[0], np.asarray(points).tolist()
    out = np.zeros(g["N"], np.int64)
    for p in range(g["N"]):
        q = p
        while q >= 0:
            if pts[q] != 0:
                out[p] = pts[q]
                break
            q = down[q]
    return out


def restated_catchment(g, points):
    """the last non-zero point on the walk downstream: the enclosing point wins"""
    down, pts = lists(g)[0], np.asarray(points).tolist()
    out = np.zeros(g["N"], np.int64)
    for p in range(g["N"]):
        q, lab = p, 0
        while q >= 0:
            if pts[q] != 0:
                lab = pts[q]
            q = down[q]
        out[p] = lab
    return out


def restated_pit(codes):
    out, n = np.zeros(len(codes), np.int64), 0
    for i, c in enumerate(codes):
        if c == 5:
            n += 1
            out[i] = n
    return out


def restated_totals(g, x):
    """the restated accuflux at the outlet, read back by every cell of its tree"""
    down = lists(g)[0]
    acc = restated_accuflux(g, x)
    out = np.empty(g["N"])
    for p in range(g["N"]):
        q = p
        while down[q] >= 0:
            q = down[q]
        out[p] = acc[q]
    return out


def jump_rounds(g, points):
    """k_jump_step launches of converge_jumps (csrc/lf_ldd.hip) on this LDD and these points: an odd count leaves the
    result in the second buffer, an even one in the first"""
    down = E.topology(g)[0]
    me = np.arange(g["N"])
    jump = np.where((down < 0) | (np.asarray(points) != 0), me, down)
    rounds = 0
    while True:
        nxt = jump[jump]
        rounds += 1
        if (nxt == jump).all():
            return rounds
        jump = nxt


_SOUND = set(range(1, 10))


def _sound(ras):
    """PCRaster's repair of a raster of codes (0: missing value): a cell whose downstream neighbour is off the map or a
    missing value becomes a pit (tests/golden/pcr_naive.py: _sound)"""
    H, W = len(ras), len(ras[0])
    out = np.zeros((H, W), np.uint8)
    for r in range(H):
        for c in range(W):
            k = ras[r][c]
            if k == 0:
                continue
            if k != 5:
                dr, dc = E._SHIFT[k]
                r2, c2 = r + dr, c + dc
                if not (0 <= r2 < H and 0 <= c2 < W) or ras[r2][c2] == 0:
                    k = 5
            out[r, c] = k
    return out


def restated_lddrepair(raster):
    """on a whole uint8 raster: codes that are not 1..9 are missing values (0 in the result)"""
    return _sound([[int(v) if int(v) in _SOUND else 0 for v in row] for row in np.asarray(raster)])


def restated_lddmask(raster, keep):
    """cells outside `keep` become missing values, then the same repair"""
    return _sound([[int(v) if int(v) in _SOUND and k != 0 else 0 for v, k in zip(row, krow)]
                   for row, krow in zip(np.asarray(raster), np.asarray(keep))])


def restated_upstream_raster(ldd, w):
    """per cell the sum of w over the neighbours that drain into it, in the order NW, N, NE, W, E, SW, S, SE, from 0.0"""
    H, W = ldd.shape
    l, ws = ldd.tolist(), w.tolist()
    out = np.zeros((H, W))
    for r in range(H):
        for c in range(W):
            s = 0.0
            for dr, dc, code in E.NBRS:
                r2, c2 = r + dr, c + dc
                if 0 <= r2 < H and 0 <= c2 < W and l[r2][c2] == code:
                    s = s + ws[r2][c2]
            out[r, c] = s
    return out


# ---- deals of the graph operations ----------------------------------------------------------------------------------
ORDERED = ("asc", "mirror", "own2")           # what a planted confluence carries, in turn
VECTOR_DEALS = ("ordered", "random", "signed_zero", "random_b")   # vector v of a sweep of several vectors is deal v
_deals = {}


def deal(name, kind, k=None):
    """-> dict(x [N] pixel order (read-only), plants [(kind, cell)], fans [(centre, sources, what)]).  Seeded; built once.
    random / random_b: uniform fill in (-1, 3).
    ordered: on the one-star trees and the top stars of graph(name)["sites"], in every in-degree they have: the sources
      carry 2^53, 1, 1, .. in ascending pixel id and the centre 0 ("asc": the result is 2^53), the mirrored order ("mirror":
      2^53 + (k - 1) rounded to even), or the centre an own x of 2 ("own2": upstream first, the cell last: 2^53 + 2).
    signed_zero: -0.0 on isolated pits and on whole one-star trees, +inf and -inf on two sources of one confluence.
    nan_at_first: the random fill with NaN at the first position of level k."""
    key = (name, kind, k)
    if key in _deals:
        return _deals[key]
    g = graph(name)
    N = g["N"]
    down, ups, dist = E.topology(g)
    seed = {"random": 11, "random_b": 12, "ordered": 13, "signed_zero": 14, "nan_at_first": 11}[kind]
    x = np.random.default_rng(seed).uniform(-1.0, 3.0, N)
    plants, fans = [], []

    def put(cell, v, what):
        x[cell] = v
        plants.append((what, int(cell)))

    if kind == "ordered":
        seen = {}
        for st in g["sites"]:
            role, j = st["role"], st["indeg"]
            n = seen.setdefault((role, j), 0)
            if role not in ("star", "top") or j == 0 or (role == "top" and n >= 3):
                continue
            seen[role, j] += 1
            what = ORDERED[n % 3]
            vals = [BIG] + [1.0] * (j - 1)
            for u, v in zip(st["ups"], vals[::-1] if what == "mirror" else vals):
                assert g["indeg"][u] == 0
                put(u, v, "source")
            put(st["centre"], 2.0 if what == "own2" else 0.0, what)
            fans.append((st["centre"], list(st["ups"]), what))
    elif kind == "signed_zero":
        iso = np.flatnonzero((down < 0) & (g["indeg"] == 0))
        # (a fixed place and its mirror near the end of the list, as module_edges.spots deals them)
        for p in sorted({p for i in range(8) for p in spots(i, iso.size, stride=5)}) if iso.size else ():
            put(iso[p], -0.0, "negzero_pit")
        stars = [st for st in g["sites"] if st["role"] == "star" and st["indeg"] >= 1]
        for i in sorted({p for i in range(3) for p in spots(i, len(stars), stride=2)}) if stars else ():
            st = stars[i]
            for u in st["ups"]:
                put(u, -0.0, "negzero_source")
            put(st["centre"], -0.0, "negzero_star")
        free = [st for st in g["sites"] if st["indeg"] >= 2 and st["role"] in ("top", "star")
                and st["centre"] not in {c for _, c in plants}]
        for st in [s for s in free if s["role"] == "top"][:1] + [s for s in free if s["role"] == "star"][-1:]:
            put(st["ups"][0], np.inf, "plus_inf")
            put(st["ups"][1], -np.inf, "minus_inf")
            plants.append(("inf_confluence", int(st["centre"])))
    elif kind == "nan_at_first":
        perm, _, ls, _ = E.layout_of(name)
        put(int(perm[ls[k]]), np.nan, "nan")
    x.setflags(write=False)
    _deals[key] = dict(name=name, kind=kind, x=x, plants=plants, fans=fans)
    return _deals[key]


_restated = {}


def restated(name, op, kind, k=None):
    """the restatement `op` ("accuflux", "upstream", "totals") of a deal, computed once and left unchanged"""
    key = (name, op, kind, k)
    if key not in _restated:
        fn = {"accuflux": restated_accuflux, "upstream": restated_upstream, "totals": restated_totals}[op]
        with np.errstate(all="ignore"):
            out = fn(graph(name), deal(name, kind, k)["x"])
        out.setflags(write=False)
        _restated[key] = out
    return _restated[key]


def deal_census(name, d, config):
    """planted kind -> launch region -> cells, from the values' places and the layout alone"""
    cfg = CONFIGS[config]
    ls = E.layout_of(name)[2]
    reg, _ = E.regions(ls, cfg["lmax"], cfg["wide"])
    pos, out = positions(name), {}
    for what, cell in d["plants"]:
        r = reg[E.level_of(ls, pos[cell])]
        out.setdefault(what, {})
        out[what][r] = out[what].get(r, 0) + 1
    return out


def indegree_census(name, config):
    """(in-degrees inside a block of several levels, in-degrees on such a block's first level) -> cells"""
    _, ups_ptr, ls, _ = E.layout_of(name)
    cfg = CONFIGS[config]
    reg, _ = E.regions(ls, cfg["lmax"], cfg["wide"])
    cnt = np.diff(ups_ptr)
    cell_region = reg[E.level_of(ls, np.arange(cnt.size))]
    return tuple({int(j): int(n) for j, n in enumerate(np.bincount(cnt[cell_region == r], minlength=9)) if n} for r in ("inside", "top"))


# ---- points for the labellings --------------------------------------------------------------------------------------
POINT_DEALS = ("none", "pits", "above_pit", "heads", "nested", "extreme")


def points(name, kind):
    """[N] int64 point ids.  On the chain rasters: no points, a point on every pit, one cell above every other pit, on the head of
    every chain, three nested points with ids of their own on every chain of five cells or more, ids of 2^31 - 1 and -1 in
    the middle of chains beside small ones, and ("too_big") one id of 2^31.  "scatter" (any graph): one cell in 40."""
    g = graph(name)
    pts = np.zeros(g["N"], np.int64)
    if kind == "scatter":
        rng = np.random.default_rng(21)
        sel = rng.choice(g["N"], max(1, g["N"] // 40), replace=False)
        pts[sel] = rng.integers(1, 9, sel.size)
        return pts
    for c, L in enumerate(g["lengths"]):
        if kind == "pits":
            pts[chain_cell(g, c, L - 1)] = c + 1
        elif kind == "above_pit" and L >= 2 and c % 2 == 0:
            pts[chain_cell(g, c, L - 2)] = c + 1
        elif kind == "heads":
            pts[chain_cell(g, c, 0)] = c + 1
        elif kind == "nested" and L >= 5:
            for n, i in enumerate((L // 4, L // 2, L - 2)):
                pts[chain_cell(g, c, i)] = 3 * c + n + 1
        elif kind == "extreme" and L >= 2:
            pts[chain_cell(g, c, (L - 1) // 2)] = (2 ** 31 - 1, -1, 7)[c % 3]
            if L >= 4 and c % 2 == 0:
                pts[chain_cell(g, c, L - 2)] = (-1, 5, 2 ** 31 - 1)[c % 3]
        elif kind == "too_big" and c == len(g["lengths"]) // 2:
            pts[chain_cell(g, c, L // 2)] = 2 ** 31
    return pts


def lane_mix(name, pts):
    """wavefronts (64 consecutive engine positions from a multiple of 64) of k_jump_init by what their lanes do: dict(
    point: wavefronts with a lane that stops at a point, bare: of those, the ones with no lane that keeps its parent,
    mixed: wavefronts that hold at once a lane stopping at a point, a lane keeping its parent and a pit)"""
    g = graph(name)
    perm = E.layout_of(name)[0]
    down = E.topology(g)[0]
    n = (perm.size + 63) // 64 * 64
    pit, pt = np.zeros(n, bool), np.zeros(n, bool)
    pit[:perm.size], pt[:perm.size] = down[perm] < 0, np.asarray(pts)[perm] != 0
    keeps = np.zeros(n, bool)
    keeps[:perm.size] = ~pit[:perm.size] & ~pt[:perm.size]
    pit, pt, keeps = (a.reshape(-1, 64).any(axis=1) for a in (pit, pt, keeps))
    return dict(point=int(pt.sum()), bare=int((pt & ~keeps).sum()), mixed=int((pt & keeps & pit).sum()))


# ---- rasters for lddrepair / lddmask -------------------------------------------------------------------------------
REPAIR_SHAPES = [(1, 1), (1, 9), (9, 1), (15, 17), (16, 16), (257, 1)]      # ... and 255, 256 and 257 cells
_PLANTS = (0, 10, 255, 5)


def repair_rasters(shape):
    """[(ldd uint8 [H, W], keep uint8 [H, W])] of one shape.  A raster carries ONE code k = 1..9 on every cell (so every code
    lies at each corner and on each edge, and no raster has a cycle), with cells of 0, 10, 255 and 5 planted at a fixed place
    and at its mirror: the cell that points at one of them is the cell pointing into code 0 / 10 / 255 / a pit.  keep: seeded,
    three cells in ten false, true as 1, 2 or 255."""
    H, W = shape
    n, out = H * W, []
    rng = np.random.default_rng(31 + n)
    if n == 1:
        codes = [np.array([[v]], np.uint8) for v in list(range(11)) + [255]]
    else:
        codes = []
        for k in range(1, 10):
            r = np.full(n, k, np.uint8)
            for j, v in enumerate(_PLANTS):
                for p in ([(2, 4, 6, 7)[j]] if n == 9 else spots(j + 1, n, stride=37)):
                    r[p] = v
            codes.append(r.reshape(H, W))
    for i, r in enumerate(codes):
        keep = np.where(rng.random((H, W)) < 0.7, rng.choice(np.array([1, 2, 255], np.uint8), (H, W)), 0).astype(np.uint8)
        if n == 1:
            keep[0, 0] = i % 2
        out.append((r, keep))
    return out


def repair_census(rasters):
    """over the rasters of one shape: cells that point into a 0, a 10, a 255, a pit and off the map, by code; the (kept cell,
    kept target) pairs of the cells that point at a cell of the map; kept pits"""
    into, pairs, kept_pits, corners = {}, {}, 0, set()
    for r, keep in rasters:
        H, W = r.shape
        for a in range(H):
            for b in range(W):
                k = int(r[a, b])
                if (a in (0, H - 1)) and (b in (0, W - 1)):
                    corners.add(((a > 0), (b > 0), k))
                if k == 5 and keep[a, b]:
                    kept_pits += 1
                if k not in E._SHIFT:
                    continue
                a2, b2 = a + E._SHIFT[k][0], b + E._SHIFT[k][1]
                if not (0 <= a2 < H and 0 <= b2 < W):
                    into["off"] = into.get("off", 0) + 1
                    continue
                t = int(r[a2, b2])
                into[t if t in _PLANTS else "flows"] = into.get(t if t in _PLANTS else "flows", 0) + 1
                key = (bool(keep[a, b]), bool(keep[a2, b2]))
                pairs[key] = pairs.get(key, 0) + 1
    return dict(into=into, pairs=pairs, kept_pits=kept_pits, corners=corners)


# ---- rasters for the raster upstream sum ---------------------------------------------------------------------------
UPSTREAM_SHAPES = [(H, W) for H in (1, 15, 16, 17, 33) for W in (1, 63, 64, 65, 129)]
TILE_H, TILE_W = 16, 64                        # kTY, kTX (csrc/lf_modules.hip)
VARIANTS = ("asc@16,64", "mirror@15,63", "cancel@16,64")


def upstream_raster(shape, variant):
    """-> (ldd uint8 [H, W], w [H, W], centres [(row, column, sources)]).  Seeded fill of codes 0..10 and 255 and weights in
    (-1, 3); the rows and columns on both sides of the tile seams (15 | 16, 63 | 64) and along the raster's edges carry the
    codes 1..9 in turn, so every direction crosses a seam and leaves the raster; an ordered sum of all the neighbours that
    exist is centred on the tile corner -- (16, 64), whose sources lie in four tiles, or (15, 63) -- and on (0, 0) and
    (H - 1, W - 1): "asc" 2^53, 1, 1, .. in the order NW, N, NE, W, E, SW, S, SE (the sum is 2^53), "mirror" the reverse,
    "cancel" 1, 2^53, -2^53, 1, .. (the sum of eight is 5; N and NE swapped give 6); the weights of all cells of code 0 and
    255 are NaN and must reach nobody, those of code 10 are -0.0."""
    H, W = shape
    v = VARIANTS.index(variant)
    rng = np.random.default_rng(1000 * H + 10 * W + v)
    ldd = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 255], np.uint8), (H, W))
    w = rng.uniform(-1.0, 3.0, (H, W))
    for r in {0, H - 1, TILE_H - 1, TILE_H} & set(range(H)):          # (every fourth cell keeps its seeded code)
        sel = (np.arange(W) + r) % 4 != 3
        ldd[r, sel] = (1 + (np.arange(W) + r) % 9)[sel]
    for c in {0, W - 1, TILE_W - 1, TILE_W} & set(range(W)):
        sel = (np.arange(H) + c) % 4 != 1
        ldd[sel, c] = (1 + (np.arange(H) + c + 4) % 9)[sel]
    centres = []
    centre = (TILE_H - 1, TILE_W - 1) if v == 1 else (TILE_H, TILE_W)
    for r, c in [centre, (0, 0), (H - 1, W - 1)]:
        # (a corner within two cells of the sum on the tile corner would take its sources: it stays as it is)
        if not (r < H and c < W) or any(max(abs(r - x[0]), abs(c - x[1])) <= 2 for x in centres):
            continue
        src = [(r + dr, c + dc, code) for dr, dc, code in E.NBRS if 0 <= r + dr < H and 0 <= c + dc < W]
        vals = [BIG] + [1.0] * (len(src) - 1) if v != 2 else ([1.0, BIG, -BIG] + [1.0] * 5)[:len(src)]
        for (r2, c2, code), val in zip(src, vals[::-1] if v == 1 else vals):
            ldd[r2, c2], w[r2, c2] = code, val
        centres.append((r, c, len(src)))
    w[(ldd == 0) | (ldd == 255)] = np.nan
    w[ldd == 10] = -0.0
    return ldd, w, centres


def upstream_raster_census(ldd):
    """-> (codes that cross a tile seam, codes that leave the raster by edge: N, S, W, E)"""
    H, W = ldd.shape
    seam, off = set(), dict(N=set(), S=set(), W=set(), E=set())
    for r in range(H):
        for c in range(W):
            k = int(ldd[r, c])
            if k not in E._SHIFT:
                continue
            r2, c2 = r + E._SHIFT[k][0], c + E._SHIFT[k][1]
            if r2 < 0:
                off["N"].add(k)
            if r2 >= H:
                off["S"].add(k)
            if c2 < 0:
                off["W"].add(k)
            if c2 >= W:
                off["E"].add(k)
            if 0 <= r2 < H and 0 <= c2 < W and (r // TILE_H != r2 // TILE_H or c // TILE_W != c2 // TILE_W):
                seam.add(k)
    return seam, off
