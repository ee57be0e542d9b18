"""Inputs that put the cell of a plain router call (kinematic_wave_parallel.py:160-184, kinematic_wave_parallel_tools.py:48-92)
on both sides -- and on the ties -- of every comparison it makes, on graphs that send cells of every in-degree 0..8 through
every launch region, a census that shows it from the values alone, and a numpy restatement of solve1Pixel and the sweep.  A
plain helper module: tests/test_route_edges_cpu.py pins the C oracle to the restatement bit for bit and asserts the shapes
of the graphs, tests/test_route_edges_gpu.py runs the same inputs through every copy of the cell on the device.

The graphs are hand-built from one element, the 3 x 3 STAR: a centre cell and those of its eight neighbours that drain
into it; the others are pits.  Stars stacked in a strip of three raster columns make a TREE: the centre of a star drains
through its south neighbour into the north neighbour of the star below, the centre of the lowest star is the pit.  So
  * the centre of a tree's top star has only source cells above it (its inflow is known exactly),
  * the centre of a one-star tree is a pit with up to eight source cells draining in (in-degree 8 exists nowhere else: a
    D8 cell whose eight neighbours drain into it has no neighbour left to drain to),
  * a neighbour that does not drain into its centre is an isolated pit (in-degree 0, last level).
The engine puts a cell on level NL - 1 - (distance to its pit), so every pit lies on the last level and a tree of T stars
(some with a fourth row) reaches 3 T - 1 or more levels up.

Planted cells have dx = 1024 m and the router dt = 4096 s, so a = alpha dx / dt = alpha / 4 and lateral dx are exact; every
tie is exact in the inputs and none depends on the result of a pow.  Cells that give NaN or more than 1e30 sit on pits or
one cell above a pit, so they spoil nothing else.
"""
import math

import numpy as np

DT = 4096.0
DX = 1024.0
CALLS = 3
TOL = 1e-12                                   # NEWTON_TOL, kinematic_wave_parallel_tools.py:26
MAX_ITERS = 3000
FAST_MIN, FAST_MAX = 1e-30, 1e30              # lf_fast_range (csrc/lf_math.h)
BIG = 2.0 ** 53
A_LOST = 1e-33                                # a router constant whose a q^beta is lost against any c >= 1
_SHIFT = {2: (1, 0), 3: (1, 1), 6: (0, 1), 9: (-1, 1), 8: (-1, 0), 7: (-1, -1), 4: (0, -1), 1: (1, -1)}  # synthetic.IX_ADDS
# the eight neighbours of a centre in ascending pixel id: (row, column) offset and the code that drains it into the centre
NBRS = ((-1, -1, 3), (-1, 0, 2), (-1, 1, 1), (0, -1, 6), (0, 1, 4), (1, -1, 9), (1, 0, 8), (1, 1, 7))
NORTH, SOUTH = 1, 6
SIDES = (0, 2, 3, 4, 5, 7)

up = lambda x: float(np.nextafter(x, np.inf))
dn = lambda x: float(np.nextafter(x, -np.inf))


# ---- graphs ----------------------------------------------------------------------------------------------------------
def _raster(H, W, strips):
    """strips[s]: the trees of raster columns 3 s .. 3 s + 2 from the top; a tree is a list of stars from the top, a star
    (in-degree of its centre, rotation of the choice of neighbours, rows: 3 or 4).  -> codes [H, W], sites (one per star:
    raster indices of the centre and of the neighbours draining in, ascending; role top / mid / bottom / star)"""
    codes = np.full((H, W), 5, np.uint8)
    sites = []
    for s, trees in enumerate(strips):
        c, r = 3 * s + 1, 0
        assert c + 1 < W
        for tree in trees:
            T = len(tree)
            for t, (j, rot, rows) in enumerate(tree):
                bottom = t == T - 1
                rc = r + 1
                assert rc + 1 < H, (s, r, H)
                order = [SIDES[(rot + i) % 6] for i in range(6)]
                if not bottom:
                    assert 1 <= j <= 7 and rows in (3, 4)
                    chosen = [NORTH] + order[:j - 1]
                    for e in range(1, rows):
                        codes[r + e, c] = 2                      # centre, south neighbour (and the fourth row) drain south
                elif T > 1:
                    assert 1 <= j <= 8 and rows == 3
                    chosen = [NORTH] + ([SOUTH] + order)[:j - 1]
                else:
                    assert 0 <= j <= 8 and rows == 3
                    chosen = [(rot + i) % 8 for i in range(j)]
                for i in chosen:
                    dr, dc, code = NBRS[i]
                    codes[rc + dr, c + dc] = code
                role = "star" if T == 1 else ("top" if t == 0 else ("bottom" if bottom else "mid"))
                sites.append(dict(centre=rc * W + c, ups=sorted((rc + NBRS[i][0]) * W + c + NBRS[i][1] for i in chosen),
                                  indeg=len(chosen), role=role))
                r += rows
        assert r <= H
    return codes, sites


class _Dealer:
    """deals the in-degrees out role by role, so that every role sees every in-degree its place allows, up to kmax"""

    def __init__(self, kmax):
        self.kmax, self.n = kmax, dict(top=0, mid=0, bottom=0, star=0)
        self.rng, self.perm = np.random.default_rng(100 + kmax), {}

    def star(self, role, rows=3):
        n = self.n[role]
        self.n[role] += 1
        def turn(m):                           # round after round of all m values, each round in an order of its own: no
            if n % m == 0:                     # in-degree keeps to the levels of one residue
                self.perm[role] = self.rng.permutation(m)
            return int(self.perm[role][n % m])
        if role in ("top", "mid"):
            j = 1 + turn(min(self.kmax, 7))
        elif role == "bottom":
            j = 1 + turn(self.kmax)
        else:
            j = turn(self.kmax + 1)
        return (j, (n // 3) % (8 if role == "star" else 6), rows)

    def tree(self, T, long_rows=()):
        if T == 1:
            return [self.star("star")]
        return [self.star("top" if t == 0 else ("bottom" if t == T - 1 else "mid"), 4 if t in long_rows else 3) for t in range(T)]


def _strip(H, deal, heights, long_every=0, s=0):
    """the trees of one strip: one tree per entry of `heights` while they fit into H rows, then one-star trees"""
    trees, r = [], 0
    for T in heights:
        long_rows = [t for t in range(T - 1) if long_every and (s + t) % long_every == 0]
        need = 3 * T + len(long_rows)
        if r + need > H:
            break
        trees.append(deal.tree(T, long_rows))
        r += need
    while r + 3 <= H:
        trees.append(deal.tree(1))
        r += 3
    return trees


def build_graph(name):
    """-> dict(name, codes [H, W], mask [H, W], sites with PIXEL ids, H, W, N).  fan1..fan8: largest in-degree exactly k, trees
    of 1 to 8 stars (26 levels); main_deep / main_shallow: 96 x 80, trees of 16 to 28 stars / of one to three stars;
    many: 300 x 300, 5000 trees of two stars; *_masked: some isolated pits are missing values."""
    masked = name.endswith("_masked")
    base = name[:-7] if masked else name
    if base.startswith("fan"):
        k = int(base[3:])
        H, nstrips = 33, 24
        deal = _Dealer(k)
        strips = [_strip(H, deal, [8 - s % 8], 3, s) for s in range(nstrips)]
    elif base == "main_deep":
        H, nstrips = 96, 26
        deal = _Dealer(8)
        strips = [_strip(H, deal, [28 - s % 13], 7, s) for s in range(nstrips)]
    elif base == "main_shallow":
        H, nstrips = 96, 26
        deal = _Dealer(8)
        strips = [_strip(H, deal, [(1, 2, 3, 1, 2, 1)[(s + i) % 6] for i in range(40)], 0, s) for s in range(nstrips)]
    elif base == "many":
        H, nstrips = 300, 100
        deal = _Dealer(8)
        strips = [_strip(H, deal, [2] * 50, 0, s) for s in range(nstrips)]
    else:
        raise KeyError(name)
    W = 3 * nstrips + (2 if base.startswith("main") else 0)
    codes, sites = _raster(H, W, strips)
    mask = np.ones((H, W), bool)
    if masked or base.startswith("fan"):
        # isolated pits as missing values, nothing else changes: every fifth one (masked), or two of three (the fans: their
        # last level then has fewer than 1024 cells, so that an in-degree-8 pit also runs in a narrow run)
        down = downstream(codes)
        iso = np.flatnonzero((down < 0) & (np.bincount(down[down >= 0], minlength=H * W) == 0))
        iso = np.setdiff1d(iso, [st["centre"] for st in sites])      # (the centre of a star nothing drains into stays)
        mask.reshape(-1)[iso[::5] if masked else iso[np.arange(iso.size) % 3 != 0]] = False
    pid = np.cumsum(mask.reshape(-1)) - 1
    for st in sites:
        assert mask.reshape(-1)[st["centre"]] and mask.reshape(-1)[st["ups"]].all()
        st["centre"] = int(pid[st["centre"]])
        st["ups"] = [int(pid[u]) for u in st["ups"]]
    return dict(name=name, codes=codes, mask=mask, sites=sites, H=H, W=W, N=int(mask.sum()))


GRAPHS = ["fan%d" % k for k in range(1, 9)] + ["main_deep", "main_shallow", "many", "main_deep_masked", "main_shallow_masked"]
_graphs = {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = build_graph(name)
    return _graphs[name]


def downstream(codes):
    """[H W] raster index a cell drains into (-1: pit) of an all-land [H, W] raster of keypad codes"""
    down = np.full(codes.size, -1, np.int64)
    for code, (dr, dc) in _SHIFT.items():
        r, c = np.nonzero(codes == code)
        down[r * codes.shape[1] + c] = (r + dr) * codes.shape[1] + (c + dc)
    return down


def topology(g):
    """from the raster alone: down [N] (pixel ids, -1: pit), ups (list of ascending arrays), dist [N] to the pit"""
    if "down" not in g:
        m = g["mask"].reshape(-1)
        pid = np.cumsum(m) - 1
        d = downstream(g["codes"])
        assert m[d[m & (d >= 0)]].all()              # no cell drains into a missing value
        down = np.where(d[m] >= 0, pid[np.maximum(d[m], 0)], -1)
        N = down.size
        order = np.argsort(down, kind="stable")
        starts = np.searchsorted(down[order], np.arange(N + 1))
        ups = [order[starts[p]:starts[p + 1]] for p in range(N)]
        dist, cur = np.zeros(N, np.int64), down.copy()
        for _ in range(N):
            alive = cur >= 0
            if not alive.any():
                break
            dist[alive] += 1
            cur[alive] = down[cur[alive]]
        g.update(down=down, ups=ups, dist=dist, indeg=np.array([u.size for u in ups]))
    return g["down"], g["ups"], g["dist"]


# ---- planted rows ----------------------------------------------------------------------------------------------------
# name -> (alpha, Q0, lateral inflow times dx): a cell of its own.  a = alpha / 4.
TAME = {      # finite results: anywhere
    "tie_on": (0.0, 0.0, TOL), "tie_on_fast": (1.0, 0.0, TOL), "c_zero": (1.0, 0.0, 0.0), "c_negzero": (-1.0, 0.0, -0.0), "c_negative": (1.0, 1.0, -1.0),
    "c_1e-30": (1.0, 0.0, FAST_MIN), "c_below_1e-30": (1.0, 0.0, dn(FAST_MIN)), "c_above_1e-30": (1.0, 0.0, up(FAST_MIN)),
    "a_1e-30": (4 * FAST_MIN, 1.0, 1.0), "a_below_1e-30": (4 * dn(FAST_MIN), 1.0, 1.0), "a_above_1e-30": (4 * up(FAST_MIN), 1.0, 1.0),
    "a_1e30": (4 * FAST_MAX, 0.0, 1e29), "a_below_1e30": (4 * dn(FAST_MAX), 0.0, 1e29), "a_above_1e30": (4 * up(FAST_MAX), 0.0, 1e29),
    "q_plus0": (1.0, 0.0, 1.0), "q_minus0": (1.0, -0.0, 1.0), "q_1e-31": (1.0, 1e-31, 1.0),
    "q_1e-30": (1.0, FAST_MIN, 1.0), "q_below_1e-30": (1.0, dn(FAST_MIN), 1.0), "q_above_1e-30": (1.0, up(FAST_MIN), 1.0),
    "floor": (4e31, 0.0, 1.0),                 # a beyond the fast range, t > 1: Newton is clamped to 1e-12 and floored to 0
    "first_guess": (1.0, 0.0, up(TOL)),        # the first guess closes within 1e-12: no Newton step, a positive value
    "a_lost": (4 * A_LOST, 0.0, 3.0),          # t <= 1 beyond the fast range: returns c itself
}
WILD = {      # NaN or beyond 1e30: on pits and one cell above a pit only
    "tie_above": (0.0, 0.0, up(TOL)), "a_zero": (0.0, 0.0, 1.0), "a_negative": (-1.0, 1.0, 1.0), "a_nan": (np.nan, 1.0, 1.0),
    "q_negative": (1.0, -1.0, 1.0), "q_inf": (1.0, np.inf, 1.0), "lat_nan": (1.0, 1.0, np.nan),
    "q_1e30": (1.0, FAST_MAX, 1.0), "q_below_1e30": (1.0, dn(FAST_MAX), 1.0), "q_above_1e30": (1.0, up(FAST_MAX), 1.0),
    "q_1e31": (1.0, 1e31, 1.0),
    "c_1e30": (1.0, 0.0, FAST_MAX), "c_below_1e30": (1.0, 0.0, dn(FAST_MAX)), "c_above_1e30": (1.0, 0.0, up(FAST_MAX)),
    "c_1e31": (1.0, 0.0, 1e31),
    "big_a_t_gt_1": (4e31, 0.0, 10.0 ** 30.5),  # a and c beyond the fast range, t > 1, the root 0.147
}
OWN = dict(TAME, **WILD)
# what the reference does with each in the FIRST call at beta = 3/5 (solve1Pixel's branch; "nan" / "zero" = the result)
EXPECT = {"tie_on": "le_tol zero", "tie_on_fast": "le_tol zero", "conf_tie_on_fast": "le_tol zero", "c_zero": "le_tol zero", "c_negzero": "le_tol zero", "c_negative": "le_tol zero",
          "c_1e-30": "le_tol zero", "c_below_1e-30": "le_tol zero", "c_above_1e-30": "le_tol zero",
          "tie_above": "t<=1 loop0 nan", "a_zero": "t<=1 loop0 nan", "a_nan": "t>1 loop0 nan", "q_negative": "t>1 loop0 nan",
          "q_inf": "t<=1 loop0 nan", "lat_nan": "t>1 loop0 nan", "floor": "t>1 floor zero", "first_guess": "t>1 loop0", "a_lost": "t<=1", "big_a_t_gt_1": "t>1",
          "a_below_1e-30": "t<=1", "a_above_1e30": "t>1", "c_above_1e30": "t<=1", "c_1e31": "t<=1",
          "a_1e-30": "t<=1", "a_above_1e-30": "t<=1", "a_1e30": "t>1", "a_below_1e30": "t>1", "a_negative": "t<=1",
          "c_1e30": "t<=1", "c_below_1e30": "t<=1", "q_plus0": "t<=1", "q_minus0": "t<=1", "q_1e-31": "t<=1", "q_1e-30": "t<=1",
          "q_below_1e-30": "t<=1", "q_above_1e-30": "t<=1", "q_1e30": "t<=1", "q_below_1e30": "t<=1", "q_above_1e30": "t<=1",
          "q_1e31": "t<=1", "fan_source": "t<=1",
          "conf_tie_on": "le_tol zero", "conf_tie_above": "t<=1 loop0 nan", "fan_asc": "t<=1", "fan_mirror": "t<=1", "fan_asc_lat": "t<=1"}
CONFLUENCE = ("fan_asc", "fan_mirror", "conf_tie_on", "conf_tie_above", "own", "conf_tie_on_fast", "fan_asc_lat")   # what a one-star tree is planted with, in turn
PER_DEGREE = dict(star=7, top=12, mid=7, bottom=0)   # how many stars of a role and in-degree are planted: the first ones
TOP = ("fan_asc", "fan_mirror", "conf_tie_on", None, "conf_tie_on_fast", "fan_asc_lat")                             # ... and the top star of a taller tree


def inputs(name, beta=0.6, seed=1, shift=0):
    """-> dict: alpha, dx, Q0 [N], lat [CALLS, N] (pixel order), beta, dt, `rows` (kind, cell, in-degree, role: every planted
    cell), `planted` [N] bool, `fans` (centre, its sources, kind).  `shift` deals the same rows out to other cells (the
    routers of a joint sweep, the members of an ensemble); the graph and the places stay."""
    from lisflood_amd import synthetic as syn
    g = graph(name)
    N = g["N"]
    down, ups, dist = topology(g)
    p = syn.router_params(N, seed=seed + 10 * shift, beta=beta, dt=DT)
    alpha, dx, Q0 = p["alpha"].copy(), p["dx"].copy(), p["Q0"].copy()
    lat = np.stack([syn.lateral_inflow(N, 40 * seed + 7 * shift + s) for s in range(CALLS)])
    planted = np.zeros(N, bool)
    rows, fans = [], []

    def put(cell, kind, a, q, ldx, role):
        assert not planted[cell], (kind, cell)
        planted[cell] = True
        alpha[cell], dx[cell], Q0[cell] = a, DX, q
        lat[:, cell] = ldx / DX
        rows.append((kind, int(cell), int(g["indeg"][cell]), role))

    own_tame, own_all = sorted(TAME), sorted(TAME) + sorted(WILD)
    n_own = [shift]

    def put_own(cell, role, wild):
        kinds = own_all if wild else own_tame
        kind = kinds[n_own[0] % len(kinds)]
        n_own[0] += 1
        put(cell, kind, *OWN[kind], role)

    per_deg = {}
    for st in g["sites"]:
        role, j, c, u = st["role"], st["indeg"], st["centre"], st["ups"]
        n = per_deg.setdefault((role, j), 0)
        per_deg[role, j] += 1
        if n >= PER_DEGREE[role]:
            continue
        if role == "star":
            what = CONFLUENCE[(n + shift) % len(CONFLUENCE)] if j else "own"
        elif role == "top":
            what = TOP[(n + shift) % len(TOP)]
        elif role == "mid" and n % 3 == 0 and len(u) > 1:   # the sources beside a star in the middle of a tree: tame rows
            for x in u:
                if g["indeg"][x] == 0:
                    put_own(x, "mid source", False)
            continue
        else:
            continue
        if what is None:
            continue
        if what == "own":                            # a pit and the cells one above it: every row, the wild ones too
            for x in u:
                put_own(x, "above pit", True)
            if j == 0:
                put_own(c, "pit", True)
            else:
                put(c, "below_own", 1.0, 1.0, 1.0, role)
        elif what in ("fan_asc", "fan_mirror", "fan_asc_lat"):
            # the sources return their inflow, the confluence c itself: 2^53, 1, 1, .. in ascending pixel id or mirrored; "lat":
            # with an inflow of 2 of its own, which a sum started from the constant term instead of 0.0 gets wrong
            # ((2^53 + 1 + ..) + 2 = 2^53 + 2, but (2 + 2^53) + 1 rounds up to 2^53 + 4)
            vals = [BIG] + [1.0] * (j - 1)
            if what == "fan_mirror":
                vals = vals[::-1]
            for x, v in zip(u, vals):
                put(x, "fan_source", 4 * A_LOST, 0.0, v, role)
            put(c, what, 4 * A_LOST, 0.0, 2.0 if what == "fan_asc_lat" else 0.0, role)
            fans.append((c, list(u), what))
        else:
            if what == "conf_tie_above" and role != "star":
                what = "conf_tie_on"
            for x in u:
                put(x, "c_zero", *OWN["c_zero"], role)
            # (alpha = 0 makes the two sides of the tie 0 and NaN; "fast": a in the fast range, where the fused forms
            # decide the tie themselves instead of handing the cell to lf_solve_cell)
            put(c, what, 1.0 if what == "conf_tie_on_fast" else 0.0, 0.0, up(TOL) if what == "conf_tie_above" else TOL, role)
    # behind the upstream run of an ordered sum of odd in-degree: the second value of its last pair load, which
    # sweep_cell_state discards -- where that is a free source cell of the level above, it returns 2^60
    perm, ups_ptr, ls, _ = layout_of(name)
    pos = np.empty(N, np.int64)
    pos[perm] = np.arange(N)
    behind_run = 0
    for c, u, what in fans:
        b = int(ups_ptr[pos[c] + 1])
        x = int(perm[b])
        if len(u) % 2 and behind_run < 8 and level_of(ls, b) == level_of(ls, pos[c]) - 1 and not planted[x] and g["indeg"][x] == 0:
            put(x, "behind_a_run", 4 * A_LOST, 0.0, 2.0 ** 60, "source")
            behind_run += 1
    # isolated pits, evenly spread over the raster: every row of its own twice
    iso = np.flatnonzero((down < 0) & (g["indeg"] == 0) & ~planted)
    take = iso[np.linspace(0, iso.size - 1, 2 * len(own_all)).astype(int)]
    assert np.unique(take).size == take.size
    for x in take:
        put_own(x, "isolated pit", True)
    return dict(name=name, alpha=alpha, dx=dx, Q0=Q0, lat=lat, beta=beta, dt=DT, rows=rows, planted=planted, fans=fans, shift=shift)


# ---- the reference restated ------------------------------------------------------------------------------------------
def _pow(x, y):
    """libm pow, as the oracle calls it"""
    try:
        return math.pow(x, y)
    except OverflowError:
        return math.inf
    except ValueError:
        return math.nan


def solve1pixel(c, a, ba, beta):
    """kinematic_wave_parallel_tools.py:59-87 on IEEE doubles -> (discharge, branch, Newton steps, floored)"""
    f = np.float64
    c, a, ba = f(c), f(a), f(ba)
    if c <= TOL:
        return 0.0, "le_tol", 0, False
    inv_beta, b_minus_1 = f(1) / f(beta), f(beta) - f(1)
    t = ba * f(_pow(c, b_minus_1))
    if t <= 1:
        branch, secant = "t<=1", c / (f(1) + t)
    else:
        branch, secant = "t>1", c / (f(1) + f(_pow(t, inv_beta)))
    other = f(_pow((c - secant) / a, inv_beta))
    q = (secant + other) / f(2)
    err = q + a * f(_pow(q, beta)) - c
    previous, count = f(-1.0), 0
    while abs(err) > TOL and q != previous and count < MAX_ITERS:
        previous = q
        q = q - err / (f(1) + ba * f(_pow(q, b_minus_1)))
        q = q if q >= TOL or q != q else f(TOL)      # builtins.max(q, NEWTON_TOL): a NaN q stays
        err = q + a * f(_pow(q, beta)) - c
        count += 1
    floored = bool(q == TOL)
    return (0.0 if floored else float(q)), branch, count, floored


def restated_call(g, inp, Q, lat):
    """one kinematicWaveRouting call restated (kinematic_wave_parallel.py:160-184): Q [N] is updated in place.  -> per cell
    the constant c the solve saw, the branch it took ("le_tol", "t<=1", "t>1"), Newton steps, whether it ended on the floor"""
    down, ups, dist = topology(g)
    N, beta = g["N"], inp["beta"]
    with np.errstate(all="ignore"):
        a = inp["alpha"] * inp["dx"] / inp["dt"]                                   # :127
        ba = beta * a
        const = a * np.array([_pow(x, beta) for x in Q]) + lat * inp["dx"]          # :163, 175
        c_seen = np.empty(N)
        branch, steps, floored = np.empty(N, object), np.zeros(N, np.int64), np.zeros(N, bool)
        for p in np.argsort(-dist, kind="stable"):                                 # upstream cells first
            s = np.float64(0.0)
            for u in ups[p]:                                                        # ascending pixel id, tools.py:57-58
                s = s + Q[u]
            c = s + const[p]
            c_seen[p] = c
            Q[p], branch[p], steps[p], floored[p] = solve1pixel(c, a[p], ba[p], beta)
    return dict(c=c_seen, branch=branch, steps=steps, floored=floored, a=a)


def census(inp, info, Q_after):
    """first call: kind -> in-degree -> what the reference did with the planted cells of that kind ("branch [loop0] [floor]
    [nan|zero]", one string per cell)"""
    out = {}
    for kind, cell, indeg, role in inp["rows"]:
        s = info["branch"][cell]
        if info["branch"][cell] != "le_tol" and info["steps"][cell] == 0:
            s += " loop0"
        if info["floored"][cell]:
            s += " floor"
        q = Q_after[cell]
        if q != q:
            s += " nan"
        elif q == 0:
            s += " zero"
        out.setdefault(kind, {}).setdefault(indeg, []).append(s)
    return out


def near_a_branch(inp, info, Q_before, rel=1e-9):
    """unplanted cells of one call whose c, a or old discharge lies within `rel` of a bound of the fast range, or whose c lies
    within `rel` of the 1e-12 tie: there the last ulp of a pow could move a cell across a branch"""
    with np.errstate(all="ignore"):
        near = np.zeros(Q_before.size, bool)
        for x in (info["c"], info["a"], Q_before):
            for b in (FAST_MIN, FAST_MAX):
                near |= np.abs(x - b) <= rel * b
        near |= np.abs(info["c"] - TOL) <= rel * TOL
    return np.flatnonzero(near & ~inp["planted"])


def bits_equal(a, b):
    """bit for bit, NaN equal to NaN (whatever its payload); +0.0 and -0.0 differ"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# ---- where the cells lie in a launch schedule ------------------------------------------------------------------------
SEGMENT_WIDE = 1024      # kNarrowMax (csrc/lf_sweep.h): with one launch per level, a level above this is a wide level
DEFAULT_WIDE = 262144    # level blocks: a level above this is a block of its own (csrc/lf_blocks.h)


def regions(level_start, lmax, wide):
    """[NL] region of every level under a schedule.  lmax = 0: one launch per level (LF_ROUTE_CONES=0): "wide" above 1024
    cells, else "narrow".  lmax >= 2: level blocks of up to lmax levels of at most `wide` cells (csrc/lf_blocks.h): "top" for
    the first level of a block of several levels, "inside" for its other levels, "wide" for a block of one level.
    -> (regions, number of blocks)"""
    NL = len(level_start) - 1
    width = np.diff(level_start)
    if lmax == 0:
        return np.where(width > SEGMENT_WIDE, "wide", "narrow").astype(object), None
    out, k, blocks = np.empty(NL, object), 0, 0
    while k < NL:
        nl = 1
        if width[k] <= wide:
            while k + nl < NL and nl < lmax and width[k + nl] <= wide:
                nl += 1
        out[k:k + nl] = "inside"
        out[k] = "top" if nl > 1 else "wide"
        k += nl
        blocks += 1
    return out, blocks


def level_of(level_start, pos):
    return np.searchsorted(level_start, pos, side="right") - 1


def wide_shapes(ups_ptr, level_start, is_wide):
    """the shapes of the wide levels at which the upstream-range arithmetic of k_level can go wrong (a wavefront = 64
    consecutive cells of a level counted from its first cell), as tests/test_level_counts_gpu.py counts them"""
    cnt = np.diff(ups_ptr.astype(np.int64))
    have = dict(levels=0, not_64=0, not_256=0, start_off_64=0, eight=0, odd=0, straddle=0, tail=0, eight_and_odd_in_one_wavefront=0)
    for k in np.flatnonzero(is_wide):
        first, n = int(level_start[k]), int(level_start[k + 1] - level_start[k])
        have["levels"] += 1
        have["not_64"] += n % 64 != 0
        have["not_256"] += n % 256 != 0
        have["start_off_64"] += first % 64 != 0
        c = np.zeros((n + 63) // 64 * 64, np.int64)
        c[:n] = cnt[first:first + n]
        c = c.reshape(-1, 64)
        have["eight"] += int((c == 8).sum())
        have["odd"] += int((c % 2 == 1).sum())
        have["straddle"] += int(((c[:-1, 63] > 0) & (c[1:, 0] > 0)).sum())
        have["tail"] += int(n % 64 != 0 and c[-1].sum() > 0)
        have["eight_and_odd_in_one_wavefront"] += int((((c == 8).sum(axis=1) > 0) & ((c % 2 == 1).sum(axis=1) > 0)).sum())
    return have


# the launch configurations of the tests: environment (read when the router is created, LF_ROUTE_CONES at every call), and the
# schedule it gives: levels per block (0: one launch per level), the width above which a level is a block of its own, cone width
CONFIGS = {
    "segments": dict(env={"LF_ROUTE_CONES": "0"}, lmax=0, wide=SEGMENT_WIDE, cw=64),
    "default": dict(env={}, lmax=256, wide=DEFAULT_WIDE, cw=64),
    "levels4": dict(env={"LF_ROUTE_LEVELS": "4"}, lmax=4, wide=DEFAULT_WIDE, cw=64),
    "levels7": dict(env={"LF_ROUTE_LEVELS": "7"}, lmax=7, wide=DEFAULT_WIDE, cw=64),
    "wide100": dict(env={"LF_FUSED_WIDE": "100"}, lmax=256, wide=100, cw=64),
    "cones256": dict(env={"LF_ROUTE_CONE_WIDTH": "256"}, lmax=256, wide=DEFAULT_WIDE, cw=256),
}


def layout_of(name):
    """(perm, ups_ptr, level_start, largest in-degree) of the engine's layout of a graph: host only"""
    g = graph(name)
    if "layout" not in g:
        from lisflood_amd.kinematic_wave_parallel import Graph
        G = Graph(ldd_raster=g["codes"], land_mask=None if g["mask"].all() else g["mask"])
        g["layout"] = G.layout() + (G.max_upstream,)
        G.close()
    return g["layout"]


def region_census(name, config, inp=None):
    """region ("wide", "narrow", "top", "inside") -> in-degree -> cells, and the same for the ordered-sum confluences of `inp`"""
    perm, ups_ptr, ls, _ = layout_of(name)
    cfg = CONFIGS[config]
    reg, _ = regions(ls, cfg["lmax"], cfg["wide"])
    cnt = np.diff(ups_ptr)
    cell_region = reg[level_of(ls, np.arange(cnt.size))]
    cells, fans = {}, {}
    for r in ("wide", "narrow", "top", "inside"):
        cells[r] = {int(j): int(n) for j, n in enumerate(np.bincount(cnt[cell_region == r], minlength=9)) if n}
    if inp is not None:
        pos = np.empty(perm.size, np.int64)
        pos[perm] = np.arange(perm.size)
        for c, u, what in inp["fans"]:
            d = fans.setdefault(cell_region[pos[c]], {})
            d[len(u)] = d.get(len(u), 0) + 1
    return cells, fans
