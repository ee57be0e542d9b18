"""Inputs that take the soil column kernel (csrc/lf_soil.hip: k_soil_fused, k_soil_stragglers) to the edges of its branches
and of its three places for a column's Courant sub-steps, a numpy restatement of soilColumnsWaterBalance
(soilloop.py:131-354) for the inputs that need no x^y, a census of the branches taken, and a 240-bit restatement of
lfo_soil_columns.  A plain helper module in the pattern of tests/module_edges.py: tests/test_soil_edges_cpu.py pins the C
oracle to the restatements without a GPU, tests/test_soil_edges_gpu.py runs the same inputs through every form of the kernel.

Four families of inputs, all seeded:

  a. pow-free     V = 4, L = 3: every soil layer at or below WRes, at or above WS, or without pore space, the relative
                  saturation of layer 1 exactly 0 or >= 1, one sub-step per column.  Every x^y of the column then has x in
                  {0, 1}, which libm's pow and the device's lf_pow_pos give exactly, everything else is + - * / sqrt under
                  -ffp-contract=off: the device must give the oracle's bits.  All values are small binary fractions, so
                  the ties are exact.  Columns are drawn from menus that hold the tie values and kept when the restatement
                  finds them pow-free (rejection sampling, vectorised); the census counts each side of each comparison.
  b. paddy        the same with two paddy fractions (mask rows 0 and 1, one of them empty over a whole tile, or the second
                  empty everywhere so that the fraction is skipped) and the 22 written arrays prefilled with a sentinel.
  c. sub-steps    layer 2 saturated, layers 1a / 1b at WRes, no rain, no evaporation: the conductivity of layer 2 is KSat2
                  exactly and Courant / CourantCrit = KSat2 / 32 exactly, so KSat2 = 32 n (or one ulp beside it) plants
                  the sub-step count; substep_layout() places chosen counts at chosen lanes of chosen tiles.
  d. near edges   synthetic.soil_params columns and columns a hair away from saturation and from WRes, against exact_column().
"""
import numpy as np

from module_edges import bmax, bmin

WRITTEN = ("AvailableWaterForInfiltration DSLR ESAct PrefFlow Infiltration W1a W1b W1 W2 Theta1a Theta1b Theta2 Sat1a "
           "Sat1b Sat1 Sat2 SeepTopToSubA SeepTopToSubB SeepSubToGW UZOutflow UZ GwPercUZLZ").split()
STATE = "DSLR W1a W1b W1 W2 UZ".split()                   # written arrays that are read first
PURE_OUT = [k for k in WRITTEN if k not in STATE]
SENTINEL = -12345.0625
LAYERS = ("1a", "1b", "2")
L_FIELDS = ("PoreSpaceNotZero1a PoreSpaceNotZero1b PoreSpaceNotZero2 KSat1a KSat1b KSat2 GenuInvM1a GenuInvM1b GenuInvM2 "
            "GenuM1a GenuM1b GenuM2 WRes1a WRes1b WRes1 WRes2 WWP1a WWP1b WWP1 WWP2 WFC1a WFC1b WFC1 WFC2 SoilDepth1a "
            "SoilDepth1b SoilDepth2 WS1a WS1b WS1 WS2 StoreMaxPervious").split()
N_FIELDS = "Rain SnowMelt b_Xinanjiang PowerInfPot PowerPrefFlow UpperZoneK GwPercStep isFrozenSoil".split()
V_IN = "LeafDrainage Interception ESMax".split()
# The bound B of the bar: what csrc/lf_math.h documents for lf_pow_pos beyond |y log2 x| = 50 ("<= 1.1e-14 beyond"), the
# larger of its two figures.  POW_POS_REL_WIDE of tests/test_device_math_gpu.py (1.3e-14) is that figure with the margin
# its assertion leaves; tests/test_soil_edges_cpu.py reads the header and fails when the two stop agreeing with this one.
POW_BOUND = 1.1e-14
MP_PREC = 240


def clone(d):
    return {k: (v.copy() if hasattr(v, "copy") else v) for k, v in d.items()}


def rel_distance(got, ref):
    """|got - ref| relative to max(|ref|, 1 mm); inf where exactly one of the two is not finite"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        dist = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    both_nan = np.isnan(got) & np.isnan(ref)
    same_inf = np.isinf(got) & np.isinf(ref) & (got == ref)
    return np.where(both_nan | same_inf, 0.0, np.where(np.isfinite(dist), dist, np.inf))


# ======================================================================================================================
# a / b. the pow-free family
# ======================================================================================================================
POWFREE_N = 300                       # two tiles per vegetation row, the second ragged
_COLUMN_DRAWS = "W1a W1b W2 W1 ESMax DSLR UZ LeafDrainage Interception".split()


def _pick(rng, menu, shape):
    return np.asarray(menu, np.float64)[rng.integers(0, len(menu), shape)]


def _strict_raise_pair():
    """(w, wres) with w < wres and w - (w - wres) < wres in fp64: the bare-soil evaporation takes es1a = w - wres < 0 from
    layer 1a and only the clamp max(w1a - es1a, WRes1a) brings the layer to WRes1a exactly (soilloop.py:159)"""
    rng = np.random.default_rng(1)
    for _ in range(10000):                                 # (w < wres / 2: closer than that the difference is exact)
        wres, w = float(rng.uniform(10.0, 20.0)), float(rng.uniform(0.1, 3.0))
        if w - (w - wres) < wres:
            return w, wres
    raise AssertionError("no such pair")


def powfree_inputs(N=POWFREE_N, seed=3, drained_fraction=0.25, paddy=None):
    """-> dict by the reference's argument names.  paddy: None, "two" (both paddy fractions run; mask row 0 is empty over
    the second tile) or "second_empty" (mask row 1 empty everywhere: the fraction is skipped).  With paddy the written arrays
    hold SENTINEL wherever the reference does not run (the six state arrays there too: nothing reads them)."""
    rng = np.random.default_rng(seed)
    V, L = 4, 3
    d = dict(DtDay=1.0, CourantCrit=0.5, AvWaterThreshold=1.0, DrainedFraction=drained_fraction)
    lu = np.array([0, 1, 2, 1], np.int64)
    d["index_landuse_all"] = lu
    d["is_irrigated"] = np.array([False, True, True, False])
    d["is_paddy_irrig"] = np.zeros(V, bool)
    d["paddy_inactive"] = np.zeros((1, N), bool)
    wstar, rstar = _strict_raise_pair()
    special = np.zeros((L, N), bool)
    for name in LAYERS:
        # 0-2: pore space with (WRes, WS) = (16, 80), (0, 64), (8, 40); 3: no depth; 4: WS = 0
        kind = np.asarray([0, 0, 0, 1, 1, 2, 2, 3, 4])[rng.integers(0, 9, (L, N))]
        wres = np.choose(kind, [16.0, 0.0, 8.0, 16.0, 0.0])
        ws = np.choose(kind, [80.0, 64.0, 40.0, 80.0, 0.0])
        depth = np.where(kind == 3, 0.0, _pick(rng, [128, 256, 512], (L, N)))
        if name == "1a":                                   # a few columns whose WRes1a is no binary fraction (see above)
            special[:, 5::41] = True
            wres, ws = np.where(special, rstar, wres), np.where(special, rstar + 64.0, ws)
            depth = np.where(special, 256.0, depth)
        pore = (depth != 0) & (ws != 0)
        d["WRes" + name], d["WS" + name], d["SoilDepth" + name], d["PoreSpaceNotZero" + name] = wres, ws, depth, pore
        d["KSat" + name] = np.where(pore, (ws - wres) * _pick(rng, [0, .125, .25, .5, .5], (L, N)), _pick(rng, [0, 4, 8], (L, N)))
        d["GenuM" + name] = _pick(rng, [.125, .25, .5], (L, N))
        d["GenuInvM" + name] = 1 / d["GenuM" + name]
        d["WWP" + name] = wres + 4
        d["WFC" + name] = d["WWP" + name] + _pick(rng, [8, 16], (L, N))
    for k in ("WS", "WRes", "WFC", "WWP"):
        d[k + "1"] = d[k + "1a"] + d[k + "1b"]
    d["StoreMaxPervious"] = _pick(rng, [0, 2, 8, 64, 128], (L, N))
    d["Rain"] = _pick(rng, [0, 0, .5, 1, 2, 8, 96], N)
    d["SnowMelt"] = _pick(rng, [0, 0, 0, .5, 1], N)
    d["isFrozenSoil"] = rng.random(N) < 0.15
    d["b_Xinanjiang"] = _pick(rng, [.25, .5], N)
    d["PowerInfPot"] = _pick(rng, [1, 2, 3], N)
    d["PowerPrefFlow"] = _pick(rng, [1, 2, 4], N)
    d["UpperZoneK"] = _pick(rng, [0, .25, .5, 1, 2], N)
    d["GwPercStep"] = _pick(rng, [0, .5, 1, 4, 200], N)
    g = lambda k: d[k][lu]

    def draw():
        c = {}
        for name in LAYERS:
            wres, ws = g("WRes" + name), g("WS" + name)
            below = np.where(special[lu], wstar, wres - 2) if name == "1a" else wres - 2
            opts = np.stack([below, wres, wres, ws, ws, ws + 4, ws + 8, ws + 64])
            c["W" + name] = np.take_along_axis(opts, rng.integers(0, 8, (1, V, N)), 0)[0]
        c["W1a"] = np.where(special[lu], wstar, c["W1a"])            # ... and enough in 1b for w1 / WS1 > 1
        c["W1b"] = np.where(special[lu], g("WS1b") + 128, c["W1b"])
        own = np.stack([g("WRes1") - 2, g("WRes1"), g("WRes1") + 1, g("WRes1") + 64])
        c["W1"] = np.where(rng.random((V, N)) < 0.7, c["W1a"] + c["W1b"], np.take_along_axis(own, rng.integers(0, 4, (1, V, N)), 0)[0])
        c["ESMax"] = _pick(rng, [0, 0, 1, 2, 4, 8, 32, 64, 128], (V, N))
        c["DSLR"] = _pick(rng, [0, 0, 1, 3, 8], (V, N))
        c["UZ"] = _pick(rng, [0, 1, 2, 8], (V, N))
        c["LeafDrainage"] = _pick(rng, [0, .5, 1], (V, N))
        c["Interception"] = _pick(rng, [0, .5, 1, 4], (V, N))
        return c

    # the fall-back column -- saturated, nothing evaporates -- is pow-free whatever the parameters
    cur = draw()
    cur.update(W1a=g("WS1a"), W1b=g("WS1b"), W2=g("WS2"), W1=g("WS1a") + g("WS1b"), ESMax=np.zeros((V, N)))
    done = np.zeros((V, N), bool)
    for _ in range(96):
        c = draw()
        _, mid = powfree_reference(dict(d, **c))
        take = mid["powfree"] & ~done
        for k in _COLUMN_DRAWS:
            cur[k] = np.where(take, c[k], cur[k])
        done |= take
    d.update(cur)
    d["powfree_drawn"] = float(done.mean())
    for k in PURE_OUT:
        d[k] = np.full((V, N), SENTINEL)
    if paddy:
        d["is_paddy_irrig"] = np.array([False, True, True, False])
        mask = rng.random((2, N)) < 0.5
        mask[0, 256:] = False
        if paddy == "second_empty":
            mask[1, :] = False
        d["paddy_inactive"] = mask
        runs = powfree_active(d)
        for k in STATE:
            d[k] = np.where(runs, d[k], SENTINEL)
    return d


def powfree_active(d):
    """[V,N] bool: the columns soilColumnsWaterBalance runs (soilloop.py:107-113; a skipped paddy fraction does not use up
    a row of paddy_inactive)"""
    V, N = d["W1a"].shape
    act = np.ones((V, N), bool)
    row = 0
    for v in range(V):
        if d["is_paddy_irrig"][v]:
            m = np.asarray(d["paddy_inactive"][row], bool)
            if not m.any():
                act[v] = False
                continue
            act[v] = m
            row += 1
    return act


def _sat_degree(w, pore, wres, ws):
    with np.errstate(all="ignore"):
        s = bmax(bmin((w - wres) / (ws - wres), 1.), 0.)
    return np.where(pore, s, 0.)


def powfree_reference(d):
    """soilloop.py:131-354 for a column whose x^y all have x in {0, 1} (x^y = x there) and that takes one sub-step, in
    numpy, with the reference's builtins min / max.  -> (the 22 written arrays, intermediates); mid["powfree"] marks
    the columns for which the assumption holds; the written arrays keep their input values where the reference skips."""
    lu = d["index_landuse_all"]
    g = lambda k: np.asarray(d[k], np.float64)[lu]
    n = lambda k: np.asarray(d[k], np.float64)[None, :]
    dt, V = d["DtDay"], len(lu)
    frozen = np.broadcast_to(np.asarray(d["isFrozenSoil"], bool)[None, :], d["W1a"].shape)
    pore = {l: np.asarray(d["PoreSpaceNotZero" + l], bool)[lu] for l in LAYERS}
    m, o = {}, {}
    with np.errstate(all="ignore"):
        m["awi_raw"] = (n("Rain") + n("SnowMelt")) + d["LeafDrainage"] - d["Interception"]           # :131
        awi = bmax(m["awi_raw"], 0.)
        m["awi"] = awi
        dslr = np.where(awi > d["AvWaterThreshold"], 1., d["DSLR"] + dt)                          # :137-140
        m["es_pot"] = d["ESMax"] * (np.sqrt(dslr) - np.sqrt(dslr - 1))                              # :151
        m["room"] = d["W1"] - g("WRes1")
        esact = np.where(frozen, 0., bmax(bmin(m["es_pot"], m["room"]), 0.))
        m["supply1a"] = d["W1a"] - g("WRes1a")
        es1a, es1b = bmin(esact, m["supply1a"]), bmax(esact - m["supply1a"], 0.)
        m["w1a_evap"], m["w1b_evap"] = d["W1a"] - es1a, d["W1b"] - es1b
        w1a = np.where(frozen, d["W1a"], bmax(m["w1a_evap"], g("WRes1a")))
        w1b = np.where(frozen, d["W1b"], bmax(m["w1b_evap"], g("WRes1b")))
        w1 = w1a + w1b                                                                              # :163
        m["fill1"] = w1 / g("WS1")
        relsat = np.where(pore["1a"], bmin(m["fill1"], 1.0), 0.0)                                    # :168
        ok = (relsat == 0) | (relsat == 1)
        satfrac = 1.0 - (1.0 - relsat)                                                              # (1 - relsat) ** b
        infpot = np.where(frozen, 0.0, g("StoreMaxPervious") * (1. - satfrac) * dt)                 # ... ** PowerInfPot
        pref = relsat * awi                                                                         # relsat ** PowerPrefFlow
        awi = awi - pref
        m["awi_left"], m["infpot"] = awi, infpot
        inf = bmax(bmin(awi, infpot), 0.)                                                           # :201
        m["test1a"] = w1a + inf
        w1a = bmin(g("WS1a"), m["test1a"])
        m["overflow"] = bmax(m["test1a"] - g("WS1a"), 0.)
        w1b = w1b + m["overflow"]
        w2 = np.asarray(d["W2"], np.float64)
        w, k, av = dict(zip(LAYERS, (w1a, w1b, w2))), {}, {}
        courant = None
        for l in LAYERS:                                                                            # :223-249
            s = _sat_degree(w[l], pore[l], g("WRes" + l), g("WS" + l))
            ok &= (s == 0) | (s == 1)
            t = 1. - (1. - s)                                                                       # 1 - (1 - s ** (1/m)) ** m
            k[l] = g("KSat" + l) * np.sqrt(s) * (t * t)
            av[l] = w[l] - g("WRes" + l)
            c = np.where(av[l] == 0, 0., k[l] * dt / av[l])
            courant = c if courant is None else bmax(courant, c)
        m["nsub"] = bmax(1., np.ceil(courant / d["CourantCrit"]))
        ok &= m["nsub"] == 1
        m["cap1"], m["cap2"] = g("WS1b") - w1b, g("WS2") - w2
        m["k"], m["av"] = {l: k[l] * dt for l in LAYERS}, av
        sa, sb, sg = bmin(m["k"]["1a"], m["cap1"]), bmin(m["k"]["1b"], m["cap2"]), bmin(m["k"]["2"], av["2"])
        zero = np.zeros_like(sa)
        sa, sb, sg = (np.where(frozen, zero, x) for x in (sa, sb, sg))                              # :313-316
        w1a = w1a - sa                                                                              # :319-325
        w1b = w1b + sa - sb
        w2 = w2 + sb - sg
        w1 = w1a + w1b
        m["w1a_over"] = w1a - g("WS1a")
        inf = inf - bmax(m["w1a_over"], 0.)
        w1a = bmin(w1a, g("WS1a"))
        o.update(DSLR=dslr, ESAct=esact, PrefFlow=pref, AvailableWaterForInfiltration=awi, Infiltration=inf, W1a=w1a, W1b=w1b,
                 W1=w1, W2=w2, SeepTopToSubA=sa, SeepTopToSubB=sb, SeepSubToGW=sg)
        for l, x in zip(LAYERS, (w1a, w1b, w2)):                                                    # :330-336
            o["Theta" + l] = np.where(pore[l], x / g("SoilDepth" + l), 0.)
            o["Sat" + l] = (x - g("WWP" + l)) / (g("WFC" + l) - g("WWP" + l))
        o["Sat1"] = (w1 - g("WWP1")) / (g("WFC1") - g("WWP1"))
        uz = np.asarray(d["UZ"], np.float64)                                                        # :340-354
        uzout = bmin(n("UpperZoneK") * uz, uz)
        uz = bmax(uz - uzout, 0.)
        drained = (np.asarray(d["is_irrigated"], bool) & ~np.asarray(d["is_paddy_irrig"], bool) & (d["DrainedFraction"] > 0))[:, None]
        uzout = np.where(drained, uzout + d["DrainedFraction"] * sg, uzout)
        uz = np.where(drained, uz + ((1 - d["DrainedFraction"]) * sg + pref), uz + (sg + pref))
        m["uz_before_perc"] = uz
        perc = bmin(n("GwPercStep"), uz)
        o.update(UZOutflow=uzout, GwPercUZLZ=perc, UZ=bmax(uz - perc, 0.))
    m.update(frozen=frozen, pore=pore, relsat=relsat, inf_first=bmax(bmin(m["awi_left"], infpot), 0.), sa=sa, sb=sb,
             drained=np.broadcast_to(drained, frozen.shape), uz_in=np.asarray(d["UZ"], np.float64),
             uzk=np.broadcast_to(n("UpperZoneK"), frozen.shape), gwp=np.broadcast_to(n("GwPercStep"), frozen.shape),
             irrigated=np.broadcast_to((np.asarray(d["is_irrigated"], bool) & ~np.asarray(d["is_paddy_irrig"], bool))[:, None], frozen.shape))
    act = powfree_active(d)
    m["active"], m["params"] = act, {k: g(k) for k in ("WRes1a", "WRes1b", "WS1a")}
    m["powfree"] = ok & np.all([np.isfinite(o[k]) for k in WRITTEN], axis=0)
    for k in WRITTEN:
        o[k] = np.where(act, o[k], d[k]) if k in d else o[k]
    return o, m


def powfree_census(mid):
    """how many of the columns that run take each side and each tie of the comparisons of soilColumnsWaterBalance"""
    m = mid
    act, thaw = m["active"], m["active"] & ~m["frozen"]
    n = lambda x, w=act: int(np.count_nonzero(x & w))
    c = {}

    def three(label, a, b, w=act):
        c[label % "<"], c[label % "=="], c[label % ">"] = n(a < b, w), n(a == b, w), n(a > b, w)
    three("rain + melt + drainage - interception %s 0", m["awi_raw"], 0.)
    three("available water %s AvWaterThreshold", m["awi"], 1.0)
    c["frozen"], c["not frozen"] = n(m["frozen"]), n(~m["frozen"])
    three("potential evaporation %s W1 - WRes1", m["es_pot"], m["room"], thaw)
    c["W1 - WRes1 < 0"] = n(m["room"] < 0, thaw)
    three("evaporation %s supply of 1a", bmax(bmin(m["es_pot"], m["room"]), 0.), m["supply1a"], thaw)
    c["w1a raised to WRes1a"] = n(m["w1a_evap"] < m["params"]["WRes1a"], thaw)
    c["w1b raised to WRes1b"] = n(m["w1b_evap"] < m["params"]["WRes1b"], thaw)
    c["no pore space in 1a"], c["pore space in 1a"] = n(~m["pore"]["1a"]), n(m["pore"]["1a"])
    three("w1 / WS1 %s 1", m["fill1"], 1.0, act & m["pore"]["1a"])
    lim = act & (m["inf_first"] > 0)
    c["infiltration = available water"] = n(m["awi_left"] <= m["infpot"], lim)
    c["infiltration = its capacity"] = n(m["awi_left"] > m["infpot"], lim)
    c["available water and capacity both 0"] = n((m["awi_left"] == 0) & (m["infpot"] == 0))
    three("w1a + infiltration %s WS1a", m["test1a"], m["params"]["WS1a"])
    c["w1b > WS1b after an overflow from 1a"] = n((m["overflow"] > 0) & (m["cap1"] < 0))
    c["SeepTopToSubA < 0"], c["SeepTopToSubB < 0"] = n(m["sa"] < 0), n(m["sb"] < 0)
    c["infiltration corrected for w1a > WS1a"] = n((m["w1a_over"] > 0) & (m["inf_first"] > 0))
    for l, limit in zip(LAYERS, (m["cap1"], m["cap2"], m["av"]["2"])):
        c["available %s == 0" % l], c["available %s != 0" % l] = n(m["av"][l] == 0), n(m["av"][l] != 0)
        three("k%s DtDay %%s its limit" % l, m["k"][l], limit)
    three("UpperZoneK %s 1", m["uzk"], 1.0)
    c["UZ == 0"], c["UZ > 0"] = n(m["uz_in"] == 0), n(m["uz_in"] > 0)
    c["drained"], c["not irrigated"] = n(m["drained"]), n(~m["irrigated"])
    c["irrigated, not drained"] = n(m["irrigated"] & ~m["drained"])
    three("GwPercStep %s uz", m["gwp"], m["uz_before_perc"])
    for l in LAYERS:
        c["Theta%s without pore space" % l] = n(~m["pore"][l])
    return c


def powfree_case(drained_fraction=0.25, paddy=None):
    """-> (inputs, restated outputs, census) of one parameter set"""
    d = powfree_inputs(drained_fraction=drained_fraction, paddy=paddy)
    out, mid = powfree_reference(d)
    return d, out, powfree_census(mid), mid


# census entries that a parameter set cannot have: DrainedFraction == 0 drains nothing, DrainedFraction > 0 leaves no
# irrigated fraction undrained unless it is a paddy fraction (which the irrigated flag then does not count)
POWFREE_SETS = {
    "drained": dict(kw=dict(drained_fraction=0.25), empty=("irrigated, not drained",)),
    "drained_fraction_0": dict(kw=dict(drained_fraction=0.0), empty=("drained",)),
    "paddy_two": dict(kw=dict(paddy="two"), empty=("drained", "irrigated, not drained")),
    "paddy_second_empty": dict(kw=dict(paddy="second_empty"), empty=("drained", "irrigated, not drained")),
}


# ======================================================================================================================
# c. the sub-step-count family
# ======================================================================================================================
TILE = 256                     # kTile
SUB_V, SUB_TILES_PER_ROW, SUB_RAGGED = 3, 7, 77
SUB_N = (SUB_TILES_PER_ROW - 1) * TILE + SUB_RAGGED      # 21 tiles: a full straggler group of 16 (rows 0, 1 and 2) and 5 more
SUB_COUNTS = (1, 2, 6, 7, 126, 127, 128, 300)


def substep_layout(seed=17):
    """-> (n [V,N] int64, ulp [V,N] in {-1, 0, +1}, frozen [N] bool): KSat2 = 32 n moved by `ulp` ulps, so the column takes
    n + (ulp > 0) sub-steps.  Tile t = row * 7 + pixel tile.  With the default trip cap of 6, counts >= 7 are stragglers:
      t0   exactly 48 stragglers (kStragCap) and 20 in-tile multi-sub-step columns (kColsPerWave: one full task)
      t1   49 stragglers (one stays in the tile) and 20 others: 21 in the tile
      t2   exactly 128 multi-sub-step columns (kLoopCap: one full round), t3: 129, t4: all 256
      t5   a mix, with frozen pixels (pixel tile 5: tiles 5, 12 and 19)
      t6   the ragged last tile of row 0
      t7   none; t8: every column 3 sub-steps; t9: 127, 128 and 300 together; t10: 20 and t11: 21 multi-sub-step columns
      t12- sprinkled counts, 126 / 127 / 128 among them"""
    rng = np.random.default_rng(seed)
    V, N = SUB_V, SUB_N
    n = np.ones((V, N), np.int64)
    ulp = np.zeros((V, N), np.int64)

    def place(tile, counts, ulps=None):
        row, pt = divmod(tile, SUB_TILES_PER_ROW)
        width = SUB_RAGGED if pt == SUB_TILES_PER_ROW - 1 else TILE
        lanes = rng.permutation(width)[:len(counts)]
        n[row, pt * TILE + lanes] = counts
        ulp[row, pt * TILE + lanes] = rng.integers(-1, 1, len(counts)) if ulps is None else ulps   # -1 or 0: the count stays n

    small = lambda k: rng.choice([2, 3, 4, 5, 6], k)
    big = lambda k: rng.choice([7, 8, 9, 12, 20, 40], k)
    place(0, np.concatenate([big(48), small(20)]))
    place(1, np.concatenate([big(49), small(20)]))
    place(2, small(128)); place(3, small(129)); place(4, small(256))
    place(5, np.concatenate([small(30), big(30), [126, 127]]))
    place(6, np.concatenate([small(10), big(10), [2, 6, 7, 1]]), ulps=None)
    place(8, np.full(256, 3), ulps=np.zeros(256, np.int64))
    place(9, [127, 128, 300, 127, 128, 126, 2, 7], ulps=[0, 0, 0, -1, -1, 0, 0, 0])
    place(10, small(20)); place(11, small(21))
    # every listed count exactly on n, one ulp below (still n) and one ulp above (n + 1), in two tiles of different groups
    for tile in (13, 18):
        cs = [c for c in SUB_COUNTS if c != 300] + [300]
        place(tile, np.repeat(cs, 3), ulps=np.tile([-1, 0, 1], len(cs)))
    for tile in (12, 14, 15, 16, 17, 19, 20):
        k = int(rng.integers(5, 60))
        place(tile, np.concatenate([small(k), big(k // 2), rng.choice([126, 127, 128], 2)]))
    frozen = np.zeros(N, bool)
    frozen[5 * TILE + rng.permutation(TILE)[:24]] = True
    return n, ulp, frozen


def substep_counts(n, ulp):
    return n + (ulp > 0)


def substep_inputs(seed=17):
    """-> (dict by the reference's argument names, counts [V,N], frozen [N]).  WRes = 16, WS = 80 in every layer, W2 = WS2,
    W1a = WRes1a, W1b = WRes1b, no rain, no evaporation, CourantCrit = 0.5: Courant / CourantCrit = (KSat2 / 64) / 0.5.
    GenuM2, UZ, UpperZoneK and GwPercStep are random, so no two columns give the same outputs."""
    rng = np.random.default_rng(seed + 1)
    n, ulp, frozen = substep_layout(seed)
    V, N = n.shape
    d = dict(DtDay=1.0, CourantCrit=0.5, AvWaterThreshold=1.0, DrainedFraction=0.25)
    d["index_landuse_all"] = np.arange(V, dtype=np.int64)
    d["is_irrigated"] = np.array([False, False, True])
    d["is_paddy_irrig"] = np.zeros(V, bool)
    d["paddy_inactive"] = np.zeros((1, N), bool)
    for name in LAYERS:
        d["WRes" + name], d["WS" + name] = np.full((V, N), 16.0), np.full((V, N), 80.0)
        d["SoilDepth" + name] = np.full((V, N), 256.0)
        d["PoreSpaceNotZero" + name] = np.ones((V, N), bool)
        d["KSat" + name] = rng.uniform(5.0, 50.0, (V, N))
        d["GenuM" + name] = rng.uniform(0.1, 0.3, (V, N))
        d["GenuInvM" + name] = 1 / d["GenuM" + name]
        d["WWP" + name], d["WFC" + name] = np.full((V, N), 24.0), np.full((V, N), 56.0)
    ks = 32.0 * n
    d["KSat2"] = np.where(ulp > 0, np.nextafter(ks, np.inf), np.where(ulp < 0, np.nextafter(ks, 0.0), ks))
    for k in ("WS", "WRes", "WFC", "WWP"):
        d[k + "1"] = d[k + "1a"] + d[k + "1b"]
    d["StoreMaxPervious"] = np.full((V, N), 64.0)
    d["W1a"], d["W1b"], d["W2"] = np.full((V, N), 16.0), np.full((V, N), 16.0), np.full((V, N), 80.0)
    d["W1"] = d["W1a"] + d["W1b"]
    d["DSLR"] = 1.0 + np.floor(rng.uniform(0.0, 6.0, (V, N)))
    d["UZ"] = rng.uniform(0.0, 20.0, (V, N))
    for k in V_IN:
        d[k] = np.zeros((V, N))
    d["Rain"], d["SnowMelt"], d["isFrozenSoil"] = np.zeros(N), np.zeros(N), frozen
    d["b_Xinanjiang"], d["PowerInfPot"] = rng.uniform(0.1, 0.8, N), rng.uniform(1.0, 3.0, N)
    d["PowerPrefFlow"], d["UpperZoneK"] = rng.uniform(1.0, 6.0, N), rng.uniform(0.01, 0.3, N)
    d["GwPercStep"] = rng.uniform(0.1, 1.5, N)
    for k in PURE_OUT:
        d[k] = np.zeros((V, N))
    return d, substep_counts(n, ulp), frozen


def trip_histogram(counts, nbins=128):
    """hist[k] = columns with k sub-steps, the last bin holds k >= nbins - 1 (lfo_soil_trip_hist, lf_soil_substep_histogram)"""
    return np.bincount(np.minimum(np.asarray(counts).ravel(), nbins - 1), minlength=nbins).astype(np.int64)


def substep_sample(counts, frozen, trip_cap=6, limit=64):
    """-> list of (row, pixel): for each count of SUB_COUNTS (and the n + 1 of its one-ulp-above column) columns that are
    not frozen, among them one-sub-step columns (run in their lane), counts <= trip_cap (the tile's LDS rounds), counts
    above it in a tile with fewer than 48 of them (stragglers) and the 49th of tile 1 wherever it lies; two with 300
    and one with 301 sub-steps; a frozen column."""
    V, N = counts.shape
    live = ~np.broadcast_to(frozen[None, :], counts.shape)
    picks = []
    for c in sorted(set(SUB_COUNTS) | {k + 1 for k in SUB_COUNTS}):
        where = np.argwhere((counts == c) & live)
        take = 2 if c >= 300 else 3
        if c == 301:
            take = 1
        for idx in (where[:: max(1, len(where) // take)][:take] if len(where) else []):
            picks.append((int(idx[0]), int(idx[1])))
    picks += [(0, int(p)) for p in np.nonzero(frozen)[0][:2]]
    t1 = np.argwhere((counts[0, TILE:2 * TILE] > trip_cap))[:, 0][-2:] + TILE
    picks += [(0, int(p)) for p in t1]
    out = []
    for p in picks:
        if p not in out:
            out.append(p)
    assert len(out) <= limit, len(out)
    return out


# ======================================================================================================================
# d. generic and near-edge columns
# ======================================================================================================================
NEAR_GENERIC, NEAR_PLANTED = 100, 20          # pixels: 3 * 100 columns of soil_params and 3 * 20 planted ones


def near_edge_inputs(seed=5):
    """soil_params(NEAR_GENERIC + NEAR_PLANTED, seed) whose last NEAR_PLANTED pixels (no rain, no evaporation, not frozen,
    unless said otherwise) hold, case k at pixel NEAR_GENERIC + k in every vegetation row:
      0-2   layer 1a / 1b / 2 one ulp below WS           3-5   one ulp above WRes
      6-8   w - WRes = 2^-40 of the pore space           9     every layer one ulp below WS
      10    w1 / WS1 one ulp below 1                      11    1a and 1b exactly saturated (w1 / WS1 == 1), 2 an ulp below
      12-15 rain that brings W1a to WS1a exactly (in the oracle's arithmetic), to an ulp below and to an ulp above it
      16-19 layers at two and three ulps below WS"""
    from lisflood_amd import synthetic as syn
    N = NEAR_GENERIC + NEAR_PLANTED
    d = syn.soil_params(NEAR_GENERIC, seed=seed)
    extra = syn.soil_params(NEAR_PLANTED, seed=seed + 1, frozen_frac=0.0, zero_pore_frac=0.0)   # all three layers there
    # At saturation the conductivity has an infinite slope ((1e-16)^m is 2.5 % at m = 0.1), so a column an ulp below WS whose
    # Courant / CourantCrit lies within a few per cent of an integer has no count to compare: KSat of the planted pixels
    # puts the ratio of a saturated layer at 1.5 (two sub-steps), far from both neighbours
    for name in LAYERS:
        extra["KSat" + name] = 1.5 * d["CourantCrit"] * (extra["WS" + name] - extra["WRes" + name])
    for k, x in d.items():
        if isinstance(x, np.ndarray) and x.ndim and x.shape[-1] == NEAR_GENERIC:
            d[k] = np.concatenate([x, extra[k]], axis=-1)
    lu = d["index_landuse_all"]
    p0 = NEAR_GENERIC
    sl = slice(p0, N)
    d["Rain"][sl], d["SnowMelt"][sl] = 0.0, 0.0
    for k in ("LeafDrainage", "Interception", "ESMax"):
        d[k][:, sl] = 0.0
    ws = lambda l, p: d["WS" + l][lu, p]
    wres = lambda l, p: d["WRes" + l][lu, p]

    def down(x, k=1):
        for _ in range(k):
            x = np.nextafter(x, -np.inf)
        return x
    for i, l in enumerate(LAYERS):
        d["W" + l][:, p0 + i] = down(ws(l, p0 + i))
        d["W" + l][:, p0 + 3 + i] = np.nextafter(wres(l, p0 + 3 + i), np.inf)
        p = p0 + 6 + i
        d["W" + l][:, p] = wres(l, p) + (ws(l, p) - wres(l, p)) * 2.0 ** -40
        d["W" + l][:, p0 + 9] = down(ws(l, p0 + 9))
        d["W" + l][:, p0 + 16 + i] = down(ws(l, p0 + 16 + i), 2)
        d["W" + l][:, p0 + 19] = down(ws(l, p0 + 19), 3)
    p = p0 + 10
    for v in range(len(lu)):
        a, b, s1 = float(ws("1a", p)[v]), float(ws("1b", p)[v]), float(d["WS1"][lu[v], p])
        d["W1a"][v, p] = a
        for _ in range(64):                                # the largest W1b with (W1a + W1b) / WS1 < 1
            b = float(np.nextafter(b, -np.inf))
            if (a + b) / s1 < 1.0:
                break
        d["W1b"][v, p] = b
    p = p0 + 11
    d["W1a"][:, p], d["W1b"][:, p], d["W2"][:, p] = ws("1a", p), ws("1b", p), down(ws("2", p))
    import math
    for k, shift in zip(range(12, 16), (0, 0, -1, 1)):
        p = p0 + k
        d["Rain"][p] = 6.0 + k
        for v in range(len(lu)):
            a, s1 = float(ws("1a", p)[v]), float(d["WS1"][lu[v], p])
            w1b, store = float(d["W1b"][v, p]), float(d["StoreMaxPervious"][lu[v], p])
            w1a = a - 3.0
            for _ in range(60):                            # fixed point of W1a = WS1a - infiltration(W1a), libm's pow
                rel = min((w1a + w1b) / s1, 1.0)
                satfrac = 1.0 - math.pow(1.0 - rel, float(d["b_Xinanjiang"][p]))
                infpot = store * math.pow(1.0 - satfrac, float(d["PowerInfPot"][p]))
                awi = d["Rain"][p] - math.pow(rel, float(d["PowerPrefFlow"][p])) * d["Rain"][p]
                inf = max(min(awi, infpot), 0.0)
                if w1a + inf == a:
                    break
                w1a = a - inf
            for _ in range(abs(shift)):
                w1a = float(np.nextafter(w1a, np.inf if shift > 0 else -np.inf))
            d["W1a"][v, p] = w1a
    d["W1"] = d["W1a"] + d["W1b"]
    return d


# ======================================================================================================================
# e. one column of lfo_soil_columns at MP_PREC bits
# ======================================================================================================================
def column_inputs(d, v, p):
    """the scalars of column (vegetation row v, pixel p) of an input dict, by name (exact doubles)"""
    j = int(d["index_landuse_all"][v])
    c = {k: float(d[k][j, p]) for k in L_FIELDS if not k.startswith("Pore")}
    c.update({k: bool(d[k][j, p]) for k in L_FIELDS if k.startswith("Pore")})
    c.update({k: float(d[k][p]) for k in N_FIELDS if k != "isFrozenSoil"})
    c["isFrozenSoil"] = bool(d["isFrozenSoil"][p])
    c.update({k: float(d[k][v, p]) for k in V_IN + STATE})
    for k in ("DtDay", "AvWaterThreshold", "CourantCrit"):
        c[k] = float(d[k])
    c["DrainedFraction"] = float(d["DrainedFraction"])
    c["drained"] = bool(d["is_irrigated"][v]) and not bool(d["is_paddy_irrig"][v]) and c["DrainedFraction"] > 0
    return c


def oracle_column_counts(oracle, d):
    """[V,N] sub-step counts of the C oracle (clamped to 127), one single-column call each: lfo_soil_trip_hist of a call
    with V = N = 1 has one entry.  Paddy masks are not applied (every column is run)."""
    V, N = d["W1a"].shape
    counts = np.zeros((V, N), np.int64)
    for v in range(V):
        for p in range(N):
            one = {}
            for k, x in d.items():
                if k in L_FIELDS or k in N_FIELDS:
                    one[k] = np.array(np.asarray(x)[..., p:p + 1], order="C")
                elif k in V_IN or k in WRITTEN:
                    one[k] = np.array(np.asarray(x)[v:v + 1, p:p + 1], order="C")   # a copy: the call writes
                else:
                    one[k] = x
            one["index_landuse_all"] = np.asarray(d["index_landuse_all"])[v:v + 1]
            one["is_irrigated"] = np.asarray(d["is_irrigated"])[v:v + 1]
            one["is_paddy_irrig"], one["paddy_inactive"] = np.zeros(1, bool), np.zeros((1, 1), bool)
            oracle.soil_columns(one)
            counts[v, p] = int(np.nonzero(oracle.soil_trip_hist())[0][0])
    return counts


def pow_draws(seed=0):
    """the perturbations of the bar: None (exact), all +B, all -B and four streams of random signs"""
    return [None, +1, -1] + [np.random.default_rng(seed + 100 + i) for i in range(4)]


def exact_column(c, delta=None, bound=POW_BOUND):
    """lfo_soil_columns for one column in mpmath at MP_PREC bits from the exact double inputs.  delta: None, +1 / -1 (every
    x^y with x not in {0, 1} is multiplied by 1 + bound / 1 - bound) or a numpy Generator (random signs); the perturbed
    power is clamped to <= 1, as x^y is for the kernel's bases in (0, 1).  -> (dict of the 22 outputs as floats, nsub)"""
    import mpmath
    mp = mpmath.mp
    old = mp.prec
    mp.prec = MP_PREC
    try:
        f = mpmath.mpf
        zero, one = f(0), f(1)

        def power(x, y):
            if x == 0 or x == 1:
                return x
            r = mpmath.power(x, y)
            if delta is not None:
                sign = delta if isinstance(delta, int) else (1 if delta.integers(0, 2) else -1)
                r = min(r * (1 + sign * f(bound)), one)
            return r

        def unsat_k(w, l):
            if c["PoreSpaceNotZero" + l]:
                s = max(min((w - f(c["WRes" + l])) / (f(c["WS" + l]) - f(c["WRes" + l])), one), zero)
            else:
                s = zero
            t = 1 - power(1 - power(s, f(c["GenuInvM" + l])), f(c["GenuM" + l]))
            return f(c["KSat" + l]) * mpmath.sqrt(s) * t * t

        def div(a, b):                                     # IEEE: x / 0 = +-inf, 0 / 0 = NaN (Sat of a layer without depth)
            if b == 0:
                return mpmath.nan if a == 0 else (mpmath.inf if a > 0 else -mpmath.inf)
            return a / b

        dt, frozen = f(c["DtDay"]), c["isFrozenSoil"]
        o = {}
        awi = max((f(c["Rain"]) + f(c["SnowMelt"])) + f(c["LeafDrainage"]) - f(c["Interception"]), zero)
        dslr = one if awi > f(c["AvWaterThreshold"]) else f(c["DSLR"]) + dt
        w1a, w1b = f(c["W1a"]), f(c["W1b"])
        if frozen:
            esact = zero
        else:
            esact = f(c["ESMax"]) * (mpmath.sqrt(dslr) - mpmath.sqrt(dslr - 1))
            esact = max(min(esact, f(c["W1"]) - f(c["WRes1"])), zero)
            supply = w1a - f(c["WRes1a"])
            es1a, es1b = min(esact, supply), max(esact - supply, zero)
            w1a, w1b = max(w1a - es1a, f(c["WRes1a"])), max(w1b - es1b, f(c["WRes1b"]))
        w1 = w1a + w1b
        relsat = min(w1 / f(c["WS1"]), one) if c["PoreSpaceNotZero1a"] else zero
        satfrac = 1 - power(1 - relsat, f(c["b_Xinanjiang"]))
        infpot = zero if frozen else f(c["StoreMaxPervious"]) * power(1 - satfrac, f(c["PowerInfPot"])) * dt
        pref = power(relsat, f(c["PowerPrefFlow"])) * awi
        awi -= pref
        inf = max(min(awi, infpot), zero)
        test1a = w1a + inf
        w1a = min(f(c["WS1a"]), test1a)
        w1b += max(test1a - f(c["WS1a"]), zero)
        w2 = f(c["W2"])
        k = [unsat_k(w1a, "1a"), unsat_k(w1b, "1b"), unsat_k(w2, "2")]
        av = [w1a - f(c["WRes1a"]), w1b - f(c["WRes1b"]), w2 - f(c["WRes2"])]
        courant = max(zero if a == 0 else kk * dt / a for kk, a in zip(k, av))
        nsub = max(1, int(mpmath.ceil(courant / f(c["CourantCrit"]))))
        cap1, cap2 = f(c["WS1b"]) - w1b, f(c["WS2"]) - w2
        sa = sb = sg = zero
        dtsub = dt / nsub
        wt = [w1a, w1b, w2]
        for s in range(nsub):
            if s > 0:
                k = [unsat_k(wt[0], "1a"), unsat_k(wt[1], "1b"), unsat_k(wt[2], "2")]
            fa, fb, fg = min(k[0] * dtsub, cap1), min(k[1] * dtsub, cap2), min(k[2] * dtsub, av[2])
            av = [av[0] - fa, av[1] + fa - fb, av[2] + fb - fg]
            wt = [av[0] + f(c["WRes1a"]), av[1] + f(c["WRes1b"]), av[2] + f(c["WRes2"])]
            cap1, cap2 = f(c["WS1b"]) - wt[1], f(c["WS2"]) - wt[2]
            sa, sb, sg = sa + fa, sb + fb, sg + fg
        if frozen:
            sa = sb = sg = zero
        w1a -= sa
        w1b = w1b + sa - sb
        w2 = w2 + sb - sg
        w1 = w1a + w1b
        inf -= max(w1a - f(c["WS1a"]), zero)
        w1a = min(w1a, f(c["WS1a"]))
        o.update(DSLR=dslr, ESAct=esact, PrefFlow=pref, AvailableWaterForInfiltration=awi, Infiltration=inf, W1a=w1a, W1b=w1b,
                 W1=w1, W2=w2, SeepTopToSubA=sa, SeepTopToSubB=sb, SeepSubToGW=sg)
        for l, x in zip(LAYERS, (w1a, w1b, w2)):
            o["Theta" + l] = x / f(c["SoilDepth" + l]) if c["PoreSpaceNotZero" + l] else zero
            o["Sat" + l] = div(x - f(c["WWP" + l]), f(c["WFC" + l]) - f(c["WWP" + l]))
        o["Sat1"] = div(w1 - f(c["WWP1"]), f(c["WFC1"]) - f(c["WWP1"]))
        uz = f(c["UZ"])
        uzout = min(f(c["UpperZoneK"]) * uz, uz)
        uz = max(uz - uzout, zero)
        if c["drained"]:
            uzout += f(c["DrainedFraction"]) * sg
            uz += (1 - f(c["DrainedFraction"])) * sg + pref
        else:
            uz += sg + pref
        perc = min(f(c["GwPercStep"]), uz)
        o.update(UZOutflow=uzout, GwPercUZLZ=perc, UZ=max(uz - perc, zero))
        return {key: float(o[key]) for key in WRITTEN}, nsub
    finally:
        mp.prec = old


def exact_reference(d, columns, oracle_out, oracle_counts=None, group=None):
    """The exact reference and the bar of `columns` (a list of (row, pixel)) of the inputs d.
    oracle_out: the 22 arrays the C oracle made of d; oracle_counts [V,N]: its sub-step counts, if the family knows them;
    group [n] of small ints: E is taken within each group of columns, so that columns whose oracle result is itself
    uncertain (an ulp below saturation) do not loosen the bar of the others.
    -> dict: ref [n,22], S [n,22] (largest deviation over pow_draws, relative to max(|x|, 1 mm)), E [groups,22] (the
    oracle's largest distance from ref per output), bar [n,22] = 2 S + 4 E[group], kept [n] bool (False: the count differs
    from the oracle's or between draws, the column is compared with nothing), nsub [n], group [n]"""
    n = len(columns)
    ref, S = np.zeros((n, len(WRITTEN))), np.zeros((n, len(WRITTEN)))
    kept, nsub = np.ones(n, bool), np.zeros(n, np.int64)
    for i, (v, p) in enumerate(columns):
        c = column_inputs(d, v, p)
        draws = pow_draws(seed=1000 * v + p)
        base, nsub[i] = exact_column(c)
        ref[i] = [base[k] for k in WRITTEN]
        if oracle_counts is not None and oracle_counts[v, p] != min(nsub[i], 127):
            kept[i] = False
        for delta in draws[1:]:
            out, ns = exact_column(c, delta)
            if ns != nsub[i]:
                kept[i] = False
            S[i] = np.maximum(S[i], rel_distance([out[k] for k in WRITTEN], ref[i]))
    orc = np.array([[oracle_out[k][v, p] for k in WRITTEN] for v, p in columns])
    dist = rel_distance(orc, ref)
    group = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    E = np.zeros((int(group.max()) + 1 if n else 1, len(WRITTEN)))
    for gid in range(E.shape[0]):
        sel = kept & (group == gid)
        if sel.any():
            E[gid] = dist[sel].max(axis=0)
    return dict(ref=ref, S=S, E=E, bar=2 * S + 4 * E[group], kept=kept, nsub=nsub, oracle_distance=dist, group=group)


GENERIC, PLANTED = 0, 1            # the groups of the near-edge family


def near_edge_case(oracle):
    """The near-edge family with its references, built once per test module: inputs d, the oracle's outputs `ref` and
    per-column counts, every column as (row, pixel) in `cols`, and exact_reference() of them with E taken separately over
    the soil_params pixels (GENERIC) and the planted ones (PLANTED)"""
    d = near_edge_inputs()
    ref = clone(d)
    oracle.soil_columns(ref)
    hist = oracle.soil_trip_hist()
    V, N = d["W1a"].shape
    cols = [(v, p) for v in range(V) for p in range(N)]
    counts = oracle_column_counts(oracle, d)
    assert np.array_equal(trip_histogram(counts), hist)
    group = np.array([GENERIC if p < NEAR_GENERIC else PLANTED for v, p in cols])
    return dict(d=d, ref=ref, hist=hist, cols=cols, counts=counts, R=exact_reference(d, cols, ref, counts, group))


def substep_places(counts, frozen, cols, trip_cap=6):
    """where each sampled column of the sub-step family runs under the default trip cap: "lane" (one sub-step, or frozen),
    "tile" (2 .. trip_cap sub-steps: the tile's LDS rounds), "straggler" (above the cap in a tile with at most 48 such
    columns) or "tile or straggler" (above the cap in a tile with more: which 48 leave is not determined)"""
    V, N = counts.shape
    live = ~np.broadcast_to(frozen[None, :], counts.shape)
    out = []
    for v, p in cols:
        t = p // TILE
        above = int(((counts[v, t * TILE:(t + 1) * TILE] > trip_cap) & live[v, t * TILE:(t + 1) * TILE]).sum())
        if not live[v, p] or counts[v, p] == 1:
            out.append("lane")
        elif counts[v, p] <= trip_cap:
            out.append("tile")
        else:
            out.append("straggler" if above <= 48 else "tile or straggler")
    return out


def bar_table(title, bar, dist):
    """per output: the largest bar, the largest distance and their largest ratio (for -s runs and DESIGN.md)"""
    lines = [title, "  %-30s %10s %10s %8s" % ("output", "bar", "distance", "ratio")]
    for k, name in enumerate(WRITTEN):
        with np.errstate(all="ignore"):
            ratio = np.where(bar[:, k] > 0, dist[:, k] / bar[:, k], np.where(dist[:, k] > 0, np.inf, 0.0))
        lines.append("  %-30s %10.2e %10.2e %8.3f" % (name, bar[:, k].max(), dist[:, k].max(), ratio.max()))
    return "\n".join(lines)
