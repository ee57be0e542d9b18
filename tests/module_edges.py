"""Inputs that put elements on both sides -- and on the ties -- of every comparison in the element-wise module kernels
and the lake / reservoir sites, a census that shows it from the values alone, and numpy restatements of the reference
lines the C oracle follows.  A plain helper module: tests/test_module_edges_cpu.py pins the oracle to the restatements
bit for bit (so the expected values are trustworthy before a GPU is involved), tests/test_module_edges_gpu.py runs the
same inputs through the HIP kernels.

Every builder is seeded, plants its edge values at fixed places (a place near the front of a vector and its mirror near
the end, so the last, partial workgroup carries them too) and fills the rest with random values.  Planted ties are exact
in the inputs themselves (powers of two and binary fractions): none depends on the result of an exp or a pow.

The restatements are written as the reference is -- np.where cascades, np.minimum / np.maximum, np.bincount -- and call
math.exp / math.pow element by element where the oracle calls libm: numpy's SIMD loops differ from libm by a few ulp
(tests/golden/make_golden.py:25).  Line numbers are the reference's, as the comments of oracle/lf_oracle.c cite them.
"""
import math
import types

import numpy as np


# ----------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """float64 arrays equal bit for bit: the same NaN pattern, and everywhere else the same 64 bits (so the sign of a zero
    counts).  NaN payloads and signs are not values of the model and are left out."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def first_difference(a, b):
    """'index: got != expected' of the first element that differs in the sense of same_bits (for assertion messages)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return "shapes %s != %s" % (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~(na | nb) & (a.view(np.uint64) != b.view(np.uint64)))
    if not bad.any():
        return "equal"
    i = tuple(int(x) for x in np.argwhere(bad)[0])
    return "%d differ, first at %s: %r != %r" % (int(bad.sum()), i, float(a[i]), float(b[i]))


def spots(k, n, stride=3):
    """the places of planted case k in a vector of n: one near the front and its mirror near the end"""
    p = (k * stride) % n
    return sorted({p, n - 1 - p})


def bmin(a, b):
    """Python's builtins.min(a, b) as the numba kernels use it: b if b < a else a"""
    return np.where(b < a, b, a)


def bmax(a, b):
    return np.where(b > a, b, a)


def _exp_each(x, where):
    out = np.zeros(x.shape)
    flat, o, w = x.reshape(-1), out.reshape(-1), where.reshape(-1)
    for i in np.nonzero(w)[0]:
        o[i] = math.exp(flat[i])
    return out


def counts_table(title, census):
    width = max(len(k) for k in census)
    return "\n".join(["%s" % title] + ["  %-*s %6d" % (width, k, v) for k, v in census.items()])


# ======================================================================================================================
# 1. canopy: soilloop.dynamic_canopy (soilloop.py:519-627), V = L = 3, vegetation row v reads land-use row v
# ======================================================================================================================
CANOPY_IO = "Interception TaInterception LeafDrainage CumInterception potential_transpiration RWS Ta W1a W1b W1".split()
CANOPY_PARAM = "LAI LAITerm CropCoef CropGroupNumber WFC1 WFC1a WFC1b WWP1 WWP1a WWP1b WPF3a WPF3b".split()
CANOPY_STATE = "CumInterception W1a W1b W1".split()
CANOPY_SCALARS = dict(LeafDrainageK=0.25, DtDay=0.5, InvDtDay=2.0)


def canopy_inputs(N, seed=5, steps=2):
    """-> dict: the [3,N] parameter maps and initial states of dynamic_canopy, `isFrozenSoil` [N], the forcing rows
    Rain / EWRef / ETRef [steps,N] and the scalars (DtDay = 0.5, so 0.1 * ETRef * InvDtDay reaches its cap of 1 at
    ETRef = 5, exactly)."""
    rng = np.random.default_rng(seed)
    V = 3
    d = dict(CANOPY_SCALARS)
    lai = rng.uniform(0.2, 8.0, (V, N))
    cum = rng.uniform(0.0, 3.0, (V, N)) * (rng.random((V, N)) < 0.7)
    cgn = rng.uniform(1.0, 5.0, (V, N))
    wwp1a, wwp1b = rng.uniform(5.0, 20.0, (V, N)), rng.uniform(10.0, 40.0, (V, N))
    wfc1a, wfc1b = wwp1a + rng.uniform(5.0, 30.0, (V, N)), wwp1b + rng.uniform(5.0, 30.0, (V, N))
    w1a, w1b = wwp1a + rng.uniform(-1.0, 40.0, (V, N)), wwp1b + rng.uniform(-1.0, 40.0, (V, N))
    frozen = rng.random(N) < 0.1
    rain = rng.uniform(0.0, 30.0, (steps, N)) * (rng.random((steps, N)) < 0.6)
    ewref, etref = rng.uniform(0.0, 5.0, (steps, N)), rng.uniform(0.0, 8.0, (steps, N))
    crop = rng.uniform(0.6, 1.2, (V, N))
    plain = dict(lai=0.5, cum=0.0, cgn=4.0)            # a column whose other branches are the ordinary ones

    def plant(k, **kw):
        for p in spots(k, N):
            v = k % V
            for name, x in dict(plain, **kw).items():
                if name == "lai": lai[v, p] = x
                elif name == "cum": cum[v, p] = x
                elif name == "cgn": cgn[v, p] = x
                elif name == "etref": etref[:, p] = x
                elif name == "ewref": ewref[:, p] = x
                elif name == "rain": rain[:, p] = x
                elif name == "frozen": frozen[p] = x
                elif name == "range":                     # WFC1 - WWP1 of the column (0: none, < 0: inverted)
                    wfc1a[v, p], wfc1b[v, p] = wwp1a[v, p] + 0.5 * x, wwp1b[v, p] + 0.5 * x
                elif name == "above":                     # (W1a - WWP1a, W1b - WWP1b)
                    w1a[v, p], w1b[v, p] = wwp1a[v, p] + x[0], wwp1b[v, p] + x[1]
                else:
                    raise KeyError(name)
    plant(0, lai=0.05, cum=1.5)                           # lai < 0.1: nothing is caught, the store still evaporates
    plant(1, lai=0.1, cum=0.0)                            # the tie lai == 0.1 (SMax = 0), and cum == 0 after the catch
    plant(2, lai=0.05, cum=-0.25)                         # cum < 0 after the catch
    plant(3, lai=43.3, cum=1.0, rain=20.0)                # the tie lai == 43.3 (the parabola)
    plant(4, lai=50.0, cum=1.0, rain=20.0)                # lai > 43.3 (SMax = 11.718)
    plant(5, lai=np.nextafter(0.1, 1.0), cum=0.5)
    plant(6, lai=np.nextafter(43.3, 100.0), cum=1.0, rain=20.0)
    plant(7, lai=3.0, cum=0.0, rain=0.0)                  # SMax > 0 and still cum == 0 after the catch
    plant(8, cgn=2.5)                                     # the tie cgn == 2.5 (the correction is added)
    plant(9, cgn=np.nextafter(2.5, 3.0))
    plant(10, cgn=1.0)
    plant(11, cgn=0.0, etref=1.0)                         # (e - 0.6) / 0 = -inf: the depletion fraction is clipped at 0
    plant(12, etref=6.0)                                  # 0.1 * ETRef * InvDtDay above its cap
    plant(13, etref=5.0)                                  # ... on it, exactly
    plant(14, etref=0.0, cgn=5.0)                         # depletion fraction clipped at 1: wcrit1 - wwp1 == 0
    plant(15, range=0.0, above=(10.0, 10.0), etref=4.0, ewref=0.0, frozen=False)   # WFC1 == WWP1: rws = 1
    plant(16, range=-1.0, above=(10.0, 10.0), etref=4.0, ewref=0.0, frozen=False)  # WFC1 < WWP1: rws = 1
    plant(17, above=(-1.0, -1.0))                         # W1 < WWP1: rws = 0, nothing to transpire
    plant(18, above=(0.0, 0.0))                           # W1 == WWP1
    plant(19, above=(0.0, 0.0), etref=4.0, ewref=0.0, frozen=False)  # (W1 is raised below: st <= 0 with ta > 0)
    plant(20, above=(30.0, 30.0), etref=4.0, ewref=0.0, frozen=True)  # frozen where there would be transpiration
    plant(21, above=(60.0, 1.0), etref=4.0, ewref=0.0, frozen=False)   # all of ta from layer 1a
    plant(22, above=(0.0, 60.0), etref=4.0, ewref=0.0, frozen=False)   # none of it from layer 1a
    plant(23, lai=3.0, rain=0.0, range=0.2, above=(0.3, 0.3), etref=7.0, ewref=0.0, frozen=False)  # ta = all above WWP1
    wwp1, wfc1, w1 = wwp1a + wwp1b, wfc1a + wfc1b, w1a + w1b
    for p in spots(19, N):                                # both layers at wilting point, W1 says there is water
        w1[19 % V, p] = wwp1[19 % V, p] + 5.0
    u = rng.uniform(0.0, 1.0, (2, V, N))
    d.update(LAI=lai, LAITerm=np.exp(-0.5 * lai), CropCoef=crop, CropGroupNumber=cgn, WFC1=wfc1, WFC1a=wfc1a, WFC1b=wfc1b,
             WWP1=wwp1, WWP1a=wwp1a, WWP1b=wwp1b, WPF3a=wwp1a + u[0] * (wfc1a - wwp1a), WPF3b=wwp1b + u[1] * (wfc1b - wwp1b),
             CumInterception=cum, W1a=w1a, W1b=w1b, W1=w1, isFrozenSoil=frozen, Rain=rain, EWRef=ewref, ETRef=etref)
    return d


def canopy_var(d, step=0, base=None):
    """a `var` namespace for oracle.canopy / soilloop(v).dynamic_canopy() with copies of the builder's arrays and the
    forcing of `step`; base: a namespace to fill (the module class wants the vegetation / land-use tables too)"""
    v = base if base is not None else types.SimpleNamespace()
    N = d["LAI"].shape[1]
    for k in CANOPY_PARAM + CANOPY_STATE:
        setattr(v, k, d[k].copy())
    for k in CANOPY_IO:
        if k not in CANOPY_STATE:
            setattr(v, k, np.zeros((3, N)))
    v.isFrozenSoil = d["isFrozenSoil"].copy()
    for k, x in CANOPY_SCALARS.items():
        setattr(v, k, x)
    canopy_forcing(v, d, step)
    return v


def canopy_forcing(v, d, step):
    for k in ("Rain", "EWRef", "ETRef"):
        setattr(v, k, d[k][step].copy())


def canopy_reference(d, state, step):
    """One dynamic_canopy() call restated: state = dict of CumInterception, W1a, W1b, W1 at the start of the call.
    -> (outputs by the names of CANOPY_IO plus WFilla / WFillb / SoilMoistureStressDays, intermediates for the census)"""
    K, inv_dt = d["LeafDrainageK"], d["InvDtDay"]
    rain, ewref, etref = d["Rain"][step][None, :], d["EWRef"][step][None, :], d["ETRef"][step][None, :]
    lai = d["LAI"]
    # interception_water_balance, soilloop.py:27-70 (builtins min / max), called from :531-544
    bare = 1. - d["LAITerm"]                                                             # :531
    ta_max = ewref * bare                                                                # :532
    smax = np.where(lai <= .1, 0., np.where(lai <= 43.3, 0.935 + 0.498 * lai - 0.00575 * (lai * lai), 11.718))
    cum0 = state["CumInterception"]
    pos = smax > 0
    with np.errstate(all="ignore"):
        arg = -0.046 * lai * rain / smax
        by_room, by_exp = smax - cum0, smax * (1. - _exp_each(arg, pos))
    by_rain = np.broadcast_to(rain, lai.shape)
    caught = np.where(pos, bmin(bmin(by_room, by_exp), by_rain), 0.)
    cum1 = np.where(pos, cum0 + caught, cum0)
    wet = cum1 > 0.
    ta_int = np.where(wet, bmax(bmin(cum1, ta_max), 0.), 0.)
    cum2 = bmax(cum1 - ta_int, 0.)
    drain = np.where(wet, K * cum2, 0.)
    cum = np.where(wet, bmax(cum2 - drain, 0.), cum1)
    # potentialTranspiration, :549-556
    pot = np.maximum(d["CropCoef"] * etref * bare - ta_int, 0.)
    # soil water depletion fraction, critical amounts, stress factor, :564-598
    cgn = d["CropGroupNumber"]
    e_raw = np.broadcast_to(0.1 * etref * inv_dt, lai.shape)
    e = np.minimum(e_raw, 1.0)
    with np.errstate(all="ignore"):
        swdf_raw = 1 / (0.76 + 1.5 * e) - 0.10 * (5 - cgn)
        swdf_raw = np.where(cgn <= 2.5, swdf_raw + (e - 0.6) / (cgn * (cgn + 3)), swdf_raw)
    swdf = np.maximum(np.minimum(swdf_raw, 1.0), 0.)
    wwp1, wwp1a, wwp1b = d["WWP1"], d["WWP1a"], d["WWP1b"]
    wcrit1 = ((1 - swdf) * (d["WFC1"] - wwp1)) + wwp1
    wcrit1a = ((1 - swdf) * (d["WFC1a"] - wwp1a)) + wwp1a
    wcrit1b = ((1 - swdf) * (d["WFC1b"] - wwp1b)) + wwp1b
    w1 = state["W1"]                                                                     # the land-use row, :592
    span = wcrit1 - wwp1
    with np.errstate(all="ignore"):
        rws_raw = np.where(span > 0, (w1 - wwp1) / span, 1.)
    rws = np.maximum(np.minimum(rws_raw, 1.), 0.)
    ta_open = np.minimum(rws * pot, np.maximum(w1 - wwp1, 0.))
    frozen = np.broadcast_to(d["isFrozenSoil"][None, :], lai.shape)
    ta = np.where(frozen, 0., ta_open)
    # abstraction from the layers 1a and 1b, :600-627
    w1a, w1b = state["W1a"], state["W1b"]
    from_a = np.minimum(ta, np.maximum(w1a - wcrit1a, 0.))
    rest_a = np.maximum(ta - from_a, 0.)
    from_b = np.minimum(rest_a, np.maximum(w1b - wcrit1b, 0.))
    rest = np.maximum(rest_a - from_b, 0.)
    left_a, left_b = np.maximum(w1a - from_a - wwp1a, 0.), np.maximum(w1b - from_b - wwp1b, 0.)
    left = left_a + left_b
    with np.errstate(all="ignore"):
        from_a = from_a + np.where(left > 0, left_a / left, 0.) * rest
        from_b = from_b + np.where(left > 0, left_b / left, 0.) * rest
    w1a, w1b = w1a - from_a, w1b - from_b
    out = dict(Interception=caught, TaInterception=ta_int, LeafDrainage=drain, CumInterception=cum,
               potential_transpiration=pot, RWS=rws, Ta=ta, W1a=w1a, W1b=w1b, W1=w1a + w1b,
               SoilMoistureStressDays=np.where(rws < 1, d["DtDay"], 0.),                 # :597-598
               WFilla=np.minimum(wcrit1a[2], d["WPF3a"][2]), WFillb=np.minimum(wcrit1b[2], d["WPF3b"][2]))  # :582-587
    mid = dict(lai=lai, smax=smax, by_room=by_room, by_exp=by_exp, by_rain=by_rain, cum1=cum1, ta_max=ta_max, cgn=cgn,
               e_raw=e_raw, swdf_raw=swdf_raw, span=span, rws_raw=rws_raw, rws=rws, above=w1 - wwp1, ta_open=ta_open,
               frozen=frozen, ta=ta, rest_a=rest_a, rest=rest, left=left, wcrit1a=wcrit1a, wpf3a=d["WPF3a"], pot=pot)
    return out, mid


def canopy_census(mid):
    """how many (vegetation, pixel) columns of one call take each side and each tie of dynamic_canopy's comparisons"""
    m = mid
    pos = m["smax"] > 0
    least = np.minimum(np.minimum(m["by_room"], m["by_exp"]), m["by_rain"])
    n = lambda x: int(np.count_nonzero(x))
    return {
        "lai < 0.1": n(m["lai"] < .1), "lai == 0.1": n(m["lai"] == .1), "0.1 < lai < 43.3": n((m["lai"] > .1) & (m["lai"] < 43.3)),
        "lai == 43.3": n(m["lai"] == 43.3), "lai > 43.3": n(m["lai"] > 43.3),
        "catch = room left": n(pos & (m["by_room"] == least) & (m["by_room"] < m["by_rain"])),
        "catch = exp term": n(pos & (m["by_exp"] == least) & (m["by_exp"] < m["by_room"]) & (m["by_exp"] < m["by_rain"])),
        "catch = rain": n(pos & (m["by_rain"] == least) & (m["by_rain"] < m["by_room"])),
        "cum == 0 after catch, SMax = 0": n(~pos & (m["cum1"] == 0)), "cum == 0 after catch, SMax > 0": n(pos & (m["cum1"] == 0)),
        "cum < 0 after catch": n(m["cum1"] < 0), "cum > 0 after catch": n(m["cum1"] > 0),
        "evaporation = store": n((m["cum1"] > 0) & (m["cum1"] <= m["ta_max"])),
        "evaporation = its maximum": n((m["cum1"] > 0) & (m["cum1"] > m["ta_max"])),
        "cgn < 2.5": n(m["cgn"] < 2.5), "cgn == 2.5": n(m["cgn"] == 2.5), "cgn > 2.5": n(m["cgn"] > 2.5),
        "e < 1": n(m["e_raw"] < 1), "e == 1": n(m["e_raw"] == 1), "e > 1": n(m["e_raw"] > 1),
        "depletion fraction > 1": n(m["swdf_raw"] > 1), "depletion fraction < 0": n(m["swdf_raw"] < 0),
        "depletion fraction inside": n((m["swdf_raw"] > 0) & (m["swdf_raw"] < 1)),
        "wcrit1 - wwp1 > 0": n(m["span"] > 0), "wcrit1 - wwp1 == 0": n(m["span"] == 0), "wcrit1 - wwp1 < 0": n(m["span"] < 0),
        "rws clipped to 0": n(m["rws_raw"] < 0), "rws == 0 unclipped": n(m["rws_raw"] == 0),
        "rws clipped to 1": n(m["rws_raw"] > 1), "0 < rws < 1": n((m["rws"] > 0) & (m["rws"] < 1)),
        "W1 < WWP1": n(m["above"] < 0), "W1 == WWP1": n(m["above"] == 0), "W1 > WWP1": n(m["above"] > 0),
        "ta = rws * pot": n((m["ta_open"] > 0) & (m["ta_open"] < m["above"])),
        "ta = water above wilting point": n((m["ta_open"] > 0) & (m["ta_open"] == m["above"])),
        "frozen with ta > 0 otherwise": n(m["frozen"] & (m["ta_open"] > 0)), "not frozen, ta > 0": n(~m["frozen"] & (m["ta"] > 0)),
        "all of ta from above wcrit1a": n((m["ta"] > 0) & (m["rest_a"] == 0)),
        "rest > 0 after both layers": n(m["rest"] > 0), "rest == 0 after both layers": n((m["ta"] > 0) & (m["rest"] == 0)),
        "rest > 0 and nothing left (st <= 0)": n((m["rest"] > 0) & (m["left"] <= 0)),
        "WFilla = wcrit1a": n(m["wcrit1a"][2] < m["wpf3a"][2]), "WFilla = WPF3a": n(m["wcrit1a"][2] >= m["wpf3a"][2]),
    }


# ======================================================================================================================
# 2. pixel aggregates: opensealed.dynamic (opensealed.py:40-71), soil.dynamic_perpixel (soil.py:471-514),
#    groundwater.dynamic (groundwater.py:134-180)
# ======================================================================================================================
PIX_V_STEP = ("TaInterception Ta ESAct PrefFlow Infiltration SeepTopToSubA SeepTopToSubB SeepSubToGW Theta1a Theta1b Theta2 "
              "W1a W1b W2 UZOutflow GwPercUZLZ").split()
PIX_N_STEP = "Rain SnowMelt EWRef".split()
PIX_STATIC = "SoilFraction SoilDepthTotal SMaxSealed DirectRunoffFraction WaterFraction LowerZoneK LZThreshold GwLossStep".split()
PIX_STATE = "CumInterSealed LZ LZInflowCUM TaInterceptionCUM TaCUM ESActCUM GwLossCUM".split()
PIX_OUT = ("RainSnowmelt EWaterAct InterSealed TASealed DirectRunoff TaInterceptionAll TaPixel ESActPixel PrefFlowPixel "
           "InfiltrationPixel ThetaAll SeepTopToSubPixelA SeepTopToSubPixelB SeepSubToGWPixel Theta1aPixel Theta1bPixel "
           "Theta2Pixel LZOutflow UZOutflowPixel GwPercUZLZPixel GwLossLZ LZAvInflow LZOutflowToChannelPixel Theta").split()


def pixel_inputs(N, seed=7, steps=2):
    """-> dict: static maps, initial states, and per step (lists of `steps` arrays) the [3,N] column results and the [N]
    forcing that pixel_aggregates reads; InvDtDay; TimeSinceStart of step s is s + 3."""
    rng = np.random.default_rng(seed)
    d = dict(InvDtDay=2.0)
    d["SoilFraction"] = rng.dirichlet([3, 2, 1], N).T * rng.uniform(0.5, 1.0, N)
    d["SoilDepthTotal"] = rng.uniform(300.0, 2000.0, (3, N))
    d["SMaxSealed"] = np.full(N, 1.0)
    d["DirectRunoffFraction"] = rng.uniform(0, 0.15, N) * (rng.random(N) < 0.5)
    d["WaterFraction"] = rng.uniform(0, 0.1, N) * (rng.random(N) < 0.3)
    d["LowerZoneK"] = rng.uniform(0.001, 0.05, N)
    d["LZThreshold"] = rng.uniform(0.0, 20.0, N) * (rng.random(N) < 0.5)
    d["GwLossStep"] = rng.uniform(0.0, 0.5, N) * (rng.random(N) < 0.5)
    d["CumInterSealed"] = rng.uniform(0.0, 0.9, N)
    d["LZ"] = rng.uniform(20.0, 100.0, N)
    d["LZInflowCUM"] = rng.uniform(0.0, 3.0, N)
    for k in ("TaInterceptionCUM", "TaCUM", "ESActCUM", "GwLossCUM"):
        d[k] = rng.uniform(0.0, 10.0, N)
    for k in PIX_V_STEP:
        hi = 300.0 if k in ("W1a", "W1b", "W2") else (1.0 if k.startswith("Theta") else 4.0)
        d[k] = [rng.uniform(0.0, hi, (3, N)) for _ in range(steps)]
    d["Rain"] = [rng.uniform(0, 20, N) * (rng.random(N) < 0.6) for _ in range(steps)]
    d["SnowMelt"] = [rng.uniform(0, 3, N) * (rng.random(N) < 0.3) for _ in range(steps)]
    d["EWRef"] = [rng.uniform(0, 5, N) for _ in range(steps)]

    def plant(k, **kw):
        for p in spots(k, N):
            for name, x in kw.items():
                if isinstance(d[name], list):
                    for s in range(steps):
                        d[name][s][..., p] = x
                else:
                    d[name][..., p] = x
    plant(0, Rain=1.0, SnowMelt=-3.0)                          # Rain + SnowMelt < 0
    plant(1, Rain=2.0, SnowMelt=-2.0)                          # ... == 0
    plant(2, SMaxSealed=1.0, CumInterSealed=2.5, Rain=4.0, EWRef=0.25)     # SMaxSealed < CumInterSealed
    plant(3, SMaxSealed=1.0, CumInterSealed=1.0, Rain=4.0, EWRef=0.0)      # ... == CumInterSealed (and stays so)
    plant(4, EWRef=-0.5, Rain=3.0)                             # EWRef < 0
    plant(5, EWRef=0.0, Rain=3.0)
    plant(6, SoilFraction=0.0, SoilDepthTotal=0.0, W1a=0.0, W1b=0.0, W2=0.0)   # no soil fraction at all: Theta is 0 * 0 / 0
    plant(7, LZ=5.0, LZThreshold=10.0, GwLossStep=0.0)         # LZ < LZThreshold
    plant(8, LZ=8.0, LZThreshold=8.0, GwLossStep=0.0, GwPercUZLZ=0.0)      # LZ == LZThreshold (and stays so)
    plant(9, LZ=50.0, LZThreshold=49.0)                        # outflow = LZ - threshold, not K * LZ
    plant(10, LZ=0.5, LZThreshold=1.0, GwLossStep=4.0, GwPercUZLZ=0.25)     # GwLossStep > LZ
    plant(11, LZInflowCUM=0.0, LZ=30.0, GwLossStep=1.0, GwPercUZLZ=0.0)     # LZInflowCUM + (perc - loss) < 0
    plant(12, LZInflowCUM=1.0, LZ=30.0, GwLossStep=1.0, GwPercUZLZ=0.0)     # ... == 0 on the first step
    return d


def pixel_var(d, step=0, v=None):
    """a `var` namespace for oracle.pixel_aggregates / pixel_aggregates.dynamic (states copied at step 0, kept after)"""
    if v is None:
        v = types.SimpleNamespace(InvDtDay=d["InvDtDay"])
        for k in PIX_STATIC:
            setattr(v, k, d[k].copy())
        for k in PIX_STATE:
            setattr(v, k, d[k].copy())
    for k in PIX_V_STEP + PIX_N_STEP:
        setattr(v, k, d[k][step].copy())
    v.TimeSinceStart = float(step + 3)
    return v


def _deffraction(f, x):
    """soil.py:460-468: (SoilFraction * X).sum("vegetation") over three rows = ((f0 x0 + f1 x1) + f2 x2)"""
    return (f[0] * x[0] + f[1] * x[1]) + f[2] * x[2]


def pixel_reference(d, state, step):
    """one opensealed.dynamic + soil.dynamic_perpixel + groundwater.dynamic restated; state: dict of PIX_STATE at the
    start of the step -> (outputs and new states by name, intermediates for the census)"""
    g = lambda k: d[k][step] if isinstance(d[k], list) else d[k]
    f, sealed, water, ewref = g("SoilFraction"), g("DirectRunoffFraction"), g("WaterFraction"), g("EWRef")
    o = {}
    # opensealed.py:45-70
    raw_supply = g("Rain") + g("SnowMelt")
    supply = np.maximum(raw_supply, 0.0)
    ewact = np.maximum(np.minimum(ewref, supply) * 1.0, 0.0)
    room = g("SMaxSealed") - state["CumInterSealed"]
    caught = np.minimum(np.maximum(room, 0.0), supply)
    store = state["CumInterSealed"] + caught
    evap = np.maximum(np.minimum(store, ewref), 0.0)
    o.update(RainSnowmelt=supply, EWaterAct=ewact, InterSealed=caught, TASealed=evap,
             CumInterSealed=np.maximum(store - evap, 0.0),
             DirectRunoff=sealed * (supply - caught) + water * (supply - ewact))
    # soil.py:475-513
    o["TaInterceptionAll"] = _deffraction(f, g("TaInterception")) + sealed * evap
    o["TaInterceptionCUM"] = state["TaInterceptionCUM"] + o["TaInterceptionAll"]
    o["TaPixel"] = _deffraction(f, g("Ta"))
    o["TaCUM"] = state["TaCUM"] + o["TaPixel"]
    o["ESActPixel"] = _deffraction(f, g("ESAct")) + water * ewact
    o["ESActCUM"] = state["ESActCUM"] + o["ESActPixel"]
    for name, src in (("PrefFlowPixel", "PrefFlow"), ("InfiltrationPixel", "Infiltration"), ("SeepTopToSubPixelA", "SeepTopToSubA"),
                      ("SeepTopToSubPixelB", "SeepTopToSubB"), ("SeepSubToGWPixel", "SeepSubToGW"), ("Theta1aPixel", "Theta1a"),
                      ("Theta1bPixel", "Theta1b"), ("Theta2Pixel", "Theta2"), ("UZOutflowPixel", "UZOutflow"),
                      ("GwPercUZLZPixel", "GwPercUZLZ")):
        o[name] = _deffraction(f, g(src))
    with np.errstate(all="ignore"):
        theta = f * (g("W1a") + g("W1b") + g("W2")) / g("SoilDepthTotal")
        fsum = (f[0] + f[1]) + f[2]
        o["Theta"] = theta
        o["ThetaAll"] = np.where(fsum > 0, ((theta[0] + theta[1]) + theta[2]) / fsum, 0.0)
    # groundwater.py:137-180
    lz0 = state["LZ"]
    by_k, by_thr = g("LowerZoneK") * lz0, lz0 - g("LZThreshold")
    out = np.maximum(np.minimum(by_k, by_thr), 0.0)
    perc = o["GwPercUZLZPixel"]
    lz = (lz0 - out) + perc
    loss = np.maximum(np.minimum(g("GwLossStep"), lz), 0.0)
    cum_raw = state["LZInflowCUM"] + (perc - loss)
    cum = np.maximum(cum_raw, 0.0)
    o.update(LZOutflow=out, LZOutflowToChannelPixel=out, GwLossLZ=loss, LZ=lz - loss, LZInflowCUM=cum,
             GwLossCUM=state["GwLossCUM"] + loss, LZAvInflow=(cum * d["InvDtDay"]) / float(step + 3))
    mid = dict(raw_supply=raw_supply, room=room, ewref=ewref, supply=supply, store=store, fsum=fsum, theta=theta, by_k=by_k,
               by_thr=by_thr, loss_step=g("GwLossStep"), lz=lz, cum_raw=cum_raw)
    return o, mid


def pixel_census(mid):
    m = mid
    n = lambda x: int(np.count_nonzero(x))
    return {
        "Rain + SnowMelt < 0": n(m["raw_supply"] < 0), "Rain + SnowMelt == 0": n(m["raw_supply"] == 0),
        "Rain + SnowMelt > 0": n(m["raw_supply"] > 0),
        "SMaxSealed < CumInterSealed": n(m["room"] < 0), "SMaxSealed == CumInterSealed": n(m["room"] == 0),
        "SMaxSealed > CumInterSealed": n(m["room"] > 0),
        "sealed catch = room": n((m["room"] > 0) & (m["room"] < m["supply"])),
        "sealed catch = supply": n((m["room"] > 0) & (m["room"] >= m["supply"])),
        "EWRef < 0": n(m["ewref"] < 0), "EWRef == 0": n(m["ewref"] == 0), "EWRef > 0": n(m["ewref"] > 0),
        "EWRef < supply": n(m["ewref"] < m["supply"]), "EWRef >= supply": n(m["ewref"] >= m["supply"]),
        "sealed store < EWRef": n(m["store"] < m["ewref"]), "sealed store >= EWRef": n(m["store"] >= m["ewref"]),
        "fraction sum == 0": n(m["fsum"] == 0), "fraction sum > 0": n(m["fsum"] > 0),
        "Theta NaN where fraction sum == 0": n((m["fsum"] == 0) & np.isnan(m["theta"]).all(axis=0)),
        "LZ < LZThreshold": n(m["by_thr"] < 0), "LZ == LZThreshold": n(m["by_thr"] == 0),
        "outflow = K LZ": n((m["by_thr"] > 0) & (m["by_k"] <= m["by_thr"])),
        "outflow = LZ - threshold": n((m["by_thr"] > 0) & (m["by_k"] > m["by_thr"])),
        "GwLossStep > LZ": n(m["loss_step"] > m["lz"]), "GwLossStep <= LZ": n(m["loss_step"] <= m["lz"]),
        "LZInflowCUM clipped at 0": n(m["cum_raw"] < 0), "LZInflowCUM == 0 unclipped": n(m["cum_raw"] == 0),
        "LZInflowCUM > 0": n(m["cum_raw"] > 0),
    }


# ======================================================================================================================
# 3. surface routing: the arithmetic before the three overland routers (surface_routing.py:122-149)
# ======================================================================================================================
SURFACE_SHAPE = (24, 31)


def surface_inputs(beta, seed=9, steps=2):
    """-> dict for surface_routing(v).dynamic() / oracle.SurfaceRouting on a 24 x 31 all-land raster with about 30 %
    channel pixels: AvailableWaterForInfiltration - Infiltration negative, zero and positive in every row, overland
    discharges of exactly 0.
    Runoff is either exactly 0 or at least a few hundredths of a mm (fractions >= 0.04, differences >= 0.5 mm, direct
    runoff >= 0.5 mm): the reference's Newton iteration stops at |q + a q^beta - c| <= 1e-12 (NEWTON_TOL,
    kinematic_wave_parallel_tools.py:26), which leaves a q^beta -- and with it the volume L alpha q^beta = a q^beta DtSec --
    undetermined by up to 1e-12 * DtSec = 8.64e-8 m3 whatever the libm.  A volume below SURFACE_MIN_VOLUME = that / 1e-9
    cannot be compared at rtol 1e-9; surface_volumes_are_comparable() shows on the oracle's run that there is none."""
    from lisflood_amd import synthetic as syn
    H, W = SURFACE_SHAPE
    N = H * W
    rng = np.random.default_rng(seed)
    mask = np.ones((H, W), bool)
    codes = syn.make_ldd("shallow", H, W, seed)[mask].astype(np.float64)
    is_chan = rng.random(N) < 0.3
    pixel_length, pixel_area, dt_sec, nsub = 5000.0, 2.5e7, 86400.0, 24
    grad = rng.uniform(0.001, 0.2, N)
    nman = np.stack([rng.uniform(0.05, 0.2, N), rng.uniform(0.2, 0.5, N), rng.uniform(0.01, 0.05, N)])
    d = dict(mask=mask, ldd_to_chan=np.where(is_chan, 5.0, codes), IsChannel=is_chan, Beta=beta, PixelLength=pixel_length,
             DtSec=dt_sec, MMtoM3=0.001 * pixel_area, M3toMM=1 / (0.001 * pixel_area), InvNoRoutSteps=1 / nsub,
             OFAlpha=((nman / np.sqrt(grad)) ** beta) * ((pixel_length + 2 * 0.001 * 5.0) ** (2.0 / 3.0 * beta)),
             SoilFraction=(rng.dirichlet([3, 2, 1], N).T + 0.1) / 1.3 * rng.uniform(0.5, 1.0, N))
    for k in ("OFQDirect", "OFQOther", "OFQForest"):
        d[k] = rng.uniform(0, 0.3, N) * (rng.random(N) < 0.8)          # a fifth of the discharges exactly 0
    d["AvailableWaterForInfiltration"], d["Infiltration"] = [], []
    for s in range(steps):
        avail = rng.uniform(5.0, 20.0, (3, N))
        side = rng.integers(0, 3, (3, N))                               # 0: less is infiltrated, 1: all of it, 2: "more"
        infil = np.where(side == 0, avail * rng.uniform(0.0, 0.9, (3, N)), np.where(side == 1, avail, avail + rng.uniform(0.0, 2.0, (3, N))))
        for k in range(9):                                              # and each of the three in every row, planted
            for p in spots(k, N):
                infil[k % 3, p] = avail[k % 3, p] + (k // 3 - 1) * 0.5
        d["AvailableWaterForInfiltration"].append(avail)
        d["Infiltration"].append(infil)
    d["DirectRunoff"] = [rng.uniform(0.5, 5.0, N) * (rng.random(N) < 0.5) for _ in range(steps)]
    d["UZOutflowPixel"] = [rng.uniform(0.0, 2.0, N) for _ in range(steps)]
    d["LZOutflowToChannelPixel"] = [rng.uniform(0.0, 1.0, N) for _ in range(steps)]
    return d


SURFACE_MIN_VOLUME = 1e-12 * 86400.0 / 1e-9          # m3: NEWTON_TOL * DtSec / rtol, see surface_inputs


def surface_volumes_are_comparable(v):
    """on the oracle's `var` after a step: no overland volume in the open interval (0, SURFACE_MIN_VOLUME)"""
    m3 = np.concatenate([v.OFM3Direct, v.OFM3Other, v.OFM3Forest])
    return bool(((m3 == 0) | (m3 >= SURFACE_MIN_VOLUME)).all()), float(m3[m3 > 0].min())


SURFACE_STEP = "AvailableWaterForInfiltration Infiltration DirectRunoff UZOutflowPixel LZOutflowToChannelPixel".split()


def surface_var(d, base=None):
    v = base if base is not None else types.SimpleNamespace()
    v.Beta, v.InvBeta = d["Beta"], 1 / d["Beta"]
    v.PixelLength, v.DtSec = d["PixelLength"], d["DtSec"]
    v.InvPixelLength, v.InvDtSec = 1 / v.PixelLength, 1 / v.DtSec
    v.MMtoM3, v.M3toMM, v.InvNoRoutSteps = d["MMtoM3"], d["M3toMM"], d["InvNoRoutSteps"]
    v.IsChannel, v.OFAlpha, v.SoilFraction = d["IsChannel"].copy(), d["OFAlpha"].copy(), d["SoilFraction"].copy()
    for k in ("OFQDirect", "OFQOther", "OFQForest"):
        setattr(v, k, d[k].copy())
    return v


def surface_forcing(v, d, step):
    for k in SURFACE_STEP:
        setattr(v, k, d[k][step].copy())


def surface_pre_reference(d, step):
    """surface_routing.py:122-149 -> SurfaceRunSoil [3,N], SurfaceRunoff, TotalRunoff, the sideflows (Direct, Other, Forest)"""
    f, direct = d["SoilFraction"], d["DirectRunoff"][step]
    part = f * np.maximum(d["AvailableWaterForInfiltration"][step] - d["Infiltration"][step], 0.)
    surf = direct + ((part[0] + part[1]) + part[2])
    total = surf + d["UZOutflowPixel"][step] + d["LZOutflowToChannelPixel"][step]
    scale = lambda x: x * d["MMtoM3"] * (1 / d["PixelLength"]) * (1 / d["DtSec"])
    return dict(SurfaceRunSoil=part, SurfaceRunoff=surf, TotalRunoff=total,
                side=np.stack([scale(direct), scale(part[0] + part[2]), scale(part[1])]))


def surface_census(d, step):
    diff = d["AvailableWaterForInfiltration"][step] - d["Infiltration"][step]
    c = {}
    for row, name in enumerate(("Rainfed", "Forest", "Irrigated")):
        c["%s: available < infiltration" % name] = int((diff[row] < 0).sum())
        c["%s: available == infiltration" % name] = int((diff[row] == 0).sum())
        c["%s: available > infiltration" % name] = int((diff[row] > 0).sum())
    for k in ("OFQDirect", "OFQOther", "OFQForest"):
        c["%s == 0" % k] = int((d[k] == 0).sum())
    c["DirectRunoff == 0"] = int((d["DirectRunoff"][step] == 0).sum())
    c["channel pixels"], c["other pixels"] = int(d["IsChannel"].sum()), int((~d["IsChannel"]).sum())
    return c


# ======================================================================================================================
# 4. lakes and reservoirs of the routing loop: lakes.dynamic_inloop (lakes.py:199-297), reservoir.dynamic_inloop
#    (reservoir.py:173-322), inflow.dynamic_inloop (inflow.py:129-147), transmission.dynamic_inloop
#    (transmission.py:67-89), the SideflowChanM3 assembly (routing.py:462-478)
# ======================================================================================================================
LAKE_PARAM = "LakeFactor LakeFactorSqr LakeAreaCC".split()
LAKE_STATE = "LakeStorageM3CC LakeInflowOldCC LakeOutflowCC LakeStorageM3BalanceCC LakeLevelCC LakeInflowCC".split()
RES_PARAM = ("TotalReservoirStorageM3CC MinReservoirOutflowCC NormalReservoirOutflowCC NonDamagingReservoirOutflowCC "
             "ConservativeStorageLimitCC NormalStorageLimitCC FloodStorageLimitCC Normal_FloodStorageLimitCC DeltaO "
             "DeltaLN DeltaNFL").split()
RES_STATE = "ReservoirStorageM3CC ReservoirFillCC ReservoirInflowCC".split()
DENSE_OUT = "QLakeOutM3Dt QResOutM3Dt QInDt QinADDEDM3 TransLossM3Dt TransCum SideflowChanM3".split()
SITE_N = 4099                        # cells of the value-by-value case: more than one workgroup, no multiple of 64
ALL_OPTIONS = dict(simulateLakes=True, simulateReservoirs=True, inflow=True, TransLoss=True)
# the planted reservoirs: limits that are binary fractions of a power-of-two capacity, so storage = limit * capacity
# and storage / capacity == limit hold exactly
TIE_CAP, TIE_LC, TIE_LN, TIE_LNF, TIE_LF = float(2 ** 26), 0.125, 0.5, 0.75, 0.875


def _random_reservoirs(rng, n, q0):
    d = {}
    d["TotalReservoirStorageM3CC"] = np.exp(rng.uniform(np.log(1e6), np.log(5e8), n))
    d["ConservativeStorageLimitCC"] = rng.uniform(0.05, 0.15, n)
    d["NormalStorageLimitCC"] = rng.uniform(0.4, 0.7, n)
    d["FloodStorageLimitCC"] = rng.uniform(0.8, 0.97, n)
    d["Normal_FloodStorageLimitCC"] = d["NormalStorageLimitCC"] + 0.5 * (d["FloodStorageLimitCC"] - d["NormalStorageLimitCC"])
    d["MinReservoirOutflowCC"], d["NormalReservoirOutflowCC"] = 0.1 * q0 + 0.01, 0.9 * q0 + 0.05
    d["NonDamagingReservoirOutflowCC"] = 4.0 * q0 + 1.0
    d["DeltaO"] = d["NormalReservoirOutflowCC"] - d["MinReservoirOutflowCC"]
    d["DeltaLN"] = d["NormalStorageLimitCC"] - 2 * d["ConservativeStorageLimitCC"]
    d["DeltaNFL"] = d["FloodStorageLimitCC"] - d["Normal_FloodStorageLimitCC"]
    return d


def _random_lakes(rng, n, dt, inflow):
    d = {}
    d["LakeAreaCC"] = rng.uniform(2e6, 5e7, n)
    lake_a = rng.uniform(5.0, 80.0, n)
    d["LakeFactor"] = d["LakeAreaCC"] / (dt * np.sqrt(lake_a))
    d["LakeFactorSqr"] = np.square(d["LakeFactor"])
    d["LakeInflowOldCC"] = np.array(inflow, dtype=np.float64)
    d["LakeLevelCC"] = rng.uniform(0.5, 3.0, n)
    storage = d["LakeAreaCC"] * d["LakeLevelCC"]
    d["LakeOutflowCC"] = np.square(d["LakeLevelCC"]) * lake_a
    d["LakeStorageM3BalanceCC"] = storage.copy()
    return d, storage


def _plant_tie_reservoir(d, r, qmin=300.0, qnorm=400.0, qnd=900.0, delta_o=77.0):
    for k, x in (("TotalReservoirStorageM3CC", TIE_CAP), ("ConservativeStorageLimitCC", TIE_LC), ("NormalStorageLimitCC", TIE_LN),
                 ("Normal_FloodStorageLimitCC", TIE_LNF), ("FloodStorageLimitCC", TIE_LF), ("MinReservoirOutflowCC", qmin),
                 ("NormalReservoirOutflowCC", qnorm), ("NonDamagingReservoirOutflowCC", qnd), ("DeltaO", delta_o),
                 ("DeltaLN", TIE_LN - 2 * TIE_LC), ("DeltaNFL", TIE_LF - TIE_LNF)):
        d[k][r] = x


def site_inputs(n_lakes, n_res, seed=13, N=SITE_N):
    """-> dict with the `var` attributes of oracle.InloopStructures for N cells in pixel order: sites at random cells,
    each fed by none, one, two or eight other cells (downstruct), ChanQ of two sub-steps, the planted lakes and
    reservoirs.  DeltaO of a planted reservoir is NOT NormalReservoirOutflow - MinReservoirOutflow, so the rule below
    NormalStorageLimit does not end where the rule above it begins and a tie on the limit shows which one was taken."""
    rng = np.random.default_rng(seed)
    dt, nsub = 3600.0, 24
    n = n_lakes + n_res
    cells = rng.permutation(N)
    site_cells, free = cells[:n], list(cells[n:])
    lake, res = np.sort(site_cells[:n_lakes]), np.sort(site_cells[n_lakes:])
    nsrc_l, nsrc_r = rng.choice([0, 1, 2, 8], n_lakes), rng.choice([0, 1, 2, 8], n_res)
    chan_q = [rng.uniform(0.0, 40.0, N), rng.uniform(0.0, 40.0, N)]
    d = dict(DtRouting=dt, NoRoutSteps=nsub, InvNoRoutSteps=1 / nsub, LakeIndex=lake, ReservoirIndex=res)
    d.update(_random_reservoirs(rng, n_res, rng.uniform(1.0, 100.0, n_res)))
    res_storage = rng.uniform(0.02, 1.3, n_res) * d["TotalReservoirStorageM3CC"]
    big = dict(lake=[], res=[])

    # ---- planted reservoirs (case k at r = 3k and at its mirror) ----
    def plant_r(k, fill=None, nsrc=0, **kw):
        for r in (spots(k, n_res) if n_res else []):
            _plant_tie_reservoir(d, r, **kw)
            nsrc_r[r] = nsrc
            if fill is not None:
                res_storage[r] = fill * TIE_CAP
            yield r
    for k, fill in enumerate((2 * TIE_LC, TIE_LN, TIE_LNF, TIE_LF)):       # the four exact ties, no inflow
        list(plant_r(k, fill=fill))
    for k, fill in ((4, 0.125), (5, 0.375), (6, 0.625), (7, 0.8125), (8, 0.9375)):   # one of each regime, inflow of one cell
        list(plant_r(k, fill=fill, nsrc=1))
    list(plant_r(9, fill=0.8125, nsrc=0))                     # above Normal_Flood, below Flood, no inflow: damped to qnorm
    list(plant_r(10, fill=1.5, nsrc=0))                       # fill > 1: out >= storage - total
    for r in plant_r(11, nsrc=0, qmin=3.0, qnorm=30.0, qnd=90.0):           # a small reservoir with a large rule outflow:
        d["TotalReservoirStorageM3CC"][r], res_storage[r] = 1e3, 600.0      # out <= storage (30 m3/s * 3600 s = 1.08e5 m3)
    for r in plant_r(12, nsrc=0):                             # a site missing from the table: total = 0, fill = inf
        d["TotalReservoirStorageM3CC"][r], res_storage[r] = 0.0, 1e6
    for r in (spots(13, n_res)[:1] if n_res else []):         # total = 0 and empty: fill = 0 / 0
        _plant_tie_reservoir(d, r)
        d["TotalReservoirStorageM3CC"][r], res_storage[r], nsrc_r[r] = 0.0, 0.0, 0
    for r in plant_r(14, fill=0.625, nsrc=3):                 # inflow 1e16 + 1 + 1 in ascending cell order
        big["res"].append(r)
    # ---- lakes ----
    lakes, lake_storage = _random_lakes(rng, n_lakes, dt, rng.uniform(0.0, 100.0, n_lakes))
    d.update(lakes)

    def plant_l(k, nsrc, factor=None, storage=None, outflow=None, inflow_old=None):
        for i in (spots(k, n_lakes) if n_lakes else []):
            nsrc_l[i] = nsrc
            if factor is not None:
                d["LakeFactor"][i], d["LakeFactorSqr"][i] = factor, factor * factor
            if storage is not None:
                lake_storage[i] = storage
            if outflow is not None:
                d["LakeOutflowCC"][i] = outflow
            if inflow_old is not None:
                d["LakeInflowOldCC"][i] = inflow_old
            yield i
    list(plant_l(0, 0, factor=100.0, storage=0.0, outflow=10.0, inflow_old=0.0))   # si = -5: storage < 0, reset to 0
    list(plant_l(1, 0, factor=1.0, storage=0.0, outflow=10.0, inflow_old=0.0))     # LakeFactorSqr + 2 si = -9: NaN, then 0
    big["lake"] = list(plant_l(2, 3))
    list(plant_l(3, 0)); list(plant_l(4, 1)); list(plant_l(5, 8))
    # ---- upstream lists: downstruct[source] = site cell, everything else drains nowhere (N) ----
    ds = np.full(N, N, np.int32)
    for cell_of, nsrc, which in ((lake, nsrc_l, "lake"), (res, nsrc_r, "res")):
        for i, c in enumerate(cell_of):
            src = sorted(free.pop() for _ in range(int(nsrc[i])))
            ds[src] = c
            if i in big[which] and len(src) == 3:     # (in a short list a later planted case may have taken the place)
                for q in chan_q:
                    q[src] = (1e16, 1.0, 1.0)
    d.update(downstruct=ds, ChanQ=chan_q, nsrc_lake=nsrc_l, nsrc_res=nsrc_r)
    d["LakeStorageM3"] = np.zeros(N); d["LakeStorageM3"][lake] = lake_storage
    d["ReservoirStorageM3"] = np.zeros(N); d["ReservoirStorageM3"][res] = res_storage
    # ---- the dense part ----
    d["ToChanM3RunoffDt"] = rng.uniform(0.0, 500.0, N)
    d["QInM3Old"], d["QDelta"] = np.zeros(N), np.zeros(N)
    pts = rng.choice(N, 64, replace=False)
    d["QInM3Old"][pts], d["QDelta"][pts] = rng.uniform(1e4, 2e5, 64), rng.uniform(-2e3, 2e3, 64)
    d["UpTrans"] = (rng.random(N) < 0.3) & (chan_q[0] > 1.0) & (chan_q[1] > 1.0) & (chan_q[0] < 1e3)
    d["TransPower1"], d["TransPower2"], d["TransSub"] = 1 / 0.95, 0.95, 1e-9
    d["TransCum"] = rng.uniform(0.0, 50.0, N)
    d["QinADDEDM3"] = rng.uniform(1.0, 9.0, N)               # what the previous model step left: sub-step 0 starts from 0
    for k in ("EvaAddM3Dt", "withdrawal_CH_actual_M3_routStep", "returnflow_GwAbs2Channel_M3_routStep", "ChannelToPolderM3Dt"):
        d[k] = rng.uniform(0.0, 30.0, N) * (rng.random(N) < 0.5)
    return d


_SITE_COPIED = (LAKE_PARAM + RES_PARAM + "LakeInflowOldCC LakeOutflowCC LakeStorageM3BalanceCC LakeLevelCC LakeStorageM3 "
                "ReservoirStorageM3 downstruct LakeIndex ReservoirIndex ToChanM3RunoffDt QInM3Old QDelta UpTrans TransCum "
                "EvaAddM3Dt withdrawal_CH_actual_M3_routStep returnflow_GwAbs2Channel_M3_routStep ChannelToPolderM3Dt".split())


def site_var(d):
    """a `var` namespace for oracle.InloopStructures(v, options) from site_inputs (ChanQ of sub-step 0)"""
    v = types.SimpleNamespace()
    for k in _SITE_COPIED:
        setattr(v, k, np.array(d[k], copy=True))
    for k in ("DtRouting", "NoRoutSteps", "InvNoRoutSteps", "TransPower1", "TransPower2", "TransSub"):
        setattr(v, k, d[k])
    v.ChanQ = d["ChanQ"][0].copy()
    return v


def site_inflow(downstruct, chan_q, cells):
    """np.bincount(downstruct, weights=ChanQ)[site] (lakes.py:215, reservoir.py:190): the sources in ascending cell order"""
    return np.bincount(downstruct, weights=chan_q, minlength=chan_q.size + 1)[cells]


def lake_reference(p, state, inflow, dt):
    """lakes.py:215-258.  p: LAKE_PARAM by name, state: LAKE_STATE by name -> (new state + QLakeOut [site], intermediates)"""
    mean_in = (inflow + state["LakeInflowOldCC"]) * 0.5                                   # :218
    si = state["LakeStorageM3CC"] / dt - 0.5 * state["LakeOutflowCC"] + mean_in           # :224
    with np.errstate(all="ignore"):
        qout = np.square(-p["LakeFactor"] + np.sqrt(p["LakeFactorSqr"] + 2 * si))         # :228
        vol_out = qout * dt
        raw = (si - qout * 0.5) * dt                                                      # :245
        st = np.where(np.isnan(raw) | (raw < 0), 0.0, raw)                                # :250-255
        out = dict(LakeInflowCC=inflow, LakeInflowOldCC=inflow, LakeOutflowCC=qout, LakeStorageM3CC=st,
                   LakeStorageM3BalanceCC=state["LakeStorageM3BalanceCC"] + (mean_in * dt - vol_out),
                   LakeLevelCC=st / p["LakeAreaCC"], QLakeOut=vol_out)
    return out, dict(raw=raw, under_root=p["LakeFactorSqr"] + 2 * si)


def reservoir_reference(p, storage, inflow, dt):
    """reservoir.py:190-296: the four candidate rules (:212-229), the cascade of np.where in the reference's order
    (:235-245), the damping rule (:247-251), the two clamps (:253-258) -> (new state + QResOut [site], intermediates)"""
    cap = p["TotalReservoirStorageM3CC"]
    qmin, qnorm, qnd = p["MinReservoirOutflowCC"], p["NormalReservoirOutflowCC"], p["NonDamagingReservoirOutflowCC"]
    two_lc, ln = 2 * p["ConservativeStorageLimitCC"], p["NormalStorageLimitCC"]
    lf, lnf = p["FloodStorageLimitCC"], p["Normal_FloodStorageLimitCC"]
    per_day = 1 / 86400.0
    with np.errstate(all="ignore"):
        st = storage + inflow * dt                                                        # :206
        fill = st / cap
        rule1 = np.minimum(qmin, st * per_day)
        rule2 = qmin + p["DeltaO"] * (fill - two_lc) / p["DeltaLN"]
        rule3 = qnorm + ((fill - lnf) / p["DeltaNFL"]) * (qnd - qnorm)
        rule4 = np.maximum((fill - lf - 0.01) * cap * per_day, np.minimum(qnd, np.maximum(inflow * 1.2, qnorm)))
        q = np.where(fill > two_lc, rule2, rule1)
        q = np.where(fill > ln, qnorm, q)
        q = np.where(fill > lnf, rule3, q)
        q = np.where(fill > lf, rule4, q)
        damp = (q > 1.2 * inflow) & (q > qnorm) & (fill < lf)
        damped = np.minimum(q, np.maximum(inflow, qnorm))
        q2 = np.where(damp, damped, q)
        rule_vol = q2 * dt
        vol = np.minimum(rule_vol, st)
        vol_out = np.maximum(vol, st - cap)
        left = st - vol_out
        f2 = left / cap
        f2 = np.where(np.isnan(f2) | (f2 < 0), 0.0, f2)
    out = dict(ReservoirInflowCC=inflow, ReservoirStorageM3CC=left, ReservoirFillCC=f2, QResOut=vol_out)
    mid = dict(fill=fill, two_lc=two_lc, ln=ln, lnf=lnf, lf=lf, q=q, damp=damp, damped=damped, rule_vol=rule_vol, st=st,
               vol=vol, cap=cap, qnorm=qnorm, inflow=inflow)
    return out, mid


def reservoir_census(mid):
    """which rule, tie, clamp each reservoir of one sub-step takes"""
    m = mid
    n = lambda x: int(np.count_nonzero(x))
    f = m["fill"]
    with np.errstate(all="ignore"):
        return {
            "fill < 2 Conservative": n(f < m["two_lc"]), "fill == 2 Conservative": n(f == m["two_lc"]),
            "2 Conservative < fill < Normal": n((f > m["two_lc"]) & (f < m["ln"])), "fill == Normal": n(f == m["ln"]),
            "Normal < fill < Normal_Flood": n((f > m["ln"]) & (f < m["lnf"])), "fill == Normal_Flood": n(f == m["lnf"]),
            "Normal_Flood < fill < Flood": n((f > m["lnf"]) & (f < m["lf"])), "fill == Flood": n(f == m["lf"]),
            "fill > Flood": n((f > m["lf"]) & np.isfinite(f)),
            "damped": n(m["damp"] & (m["damped"] != m["q"])),
            "not damped: fill >= Flood": n((m["q"] > 1.2 * m["inflow"]) & (m["q"] > m["qnorm"]) & (f >= m["lf"])),
            "not damped: out <= 1.2 inflow": n((m["q"] <= 1.2 * m["inflow"]) & (m["q"] > m["qnorm"]) & (f < m["lf"])),
            "out > storage": n(m["rule_vol"] > m["st"]), "out < storage - total": n(m["vol"] < m["st"] - m["cap"]),
            "fill > 1": n((f > 1) & np.isfinite(f)),
            "total == 0: fill inf": n(np.isinf(f)), "total == 0: fill NaN": n(np.isnan(f)),
        }


def lake_census(mid):
    m = mid
    n = lambda x: int(np.count_nonzero(x))
    with np.errstate(all="ignore"):
        return {"lake storage < 0, reset": n(m["raw"] < 0), "lake storage NaN, reset": n(np.isnan(m["raw"])),
                "lake storage >= 0": n(m["raw"] >= 0), "LakeFactorSqr + 2 si < 0": n(m["under_root"] < 0)}


def layout_census(d):
    """the site count and layout from the index vectors alone: one lane per site, lakes first, 256 lanes per workgroup,
    64 per wavefront"""
    nl, nr = len(d["LakeIndex"]), len(d["ReservoirIndex"])
    c = {"sites": nl + nr, "workgroups of the site kernels": -(-(nl + nr) // 256),
         "lake / reservoir boundary inside a wavefront": int(nl % 64 != 0 and nr > 0 and nl > 0),
         "reservoirs in a second workgroup": max(nl + nr - max(nl, 256), 0)}
    for name, nsrc in (("lakes", d["nsrc_lake"]), ("reservoirs", d["nsrc_res"])):
        for k in (0, 1, 3, 8):
            c["%s with %d sources" % (name, k)] = int((np.asarray(nsrc) == k).sum())
    return c


def dense_reference(d, v, step, options, lake_out=None, res_out=None):
    """inflow.py:142-144, transmission.py:76-87 and routing.py:462-478 for one sub-step.  v: the state before
    (QinADDEDM3, TransCum) and ChanQ; lake_out / res_out: dense outflow vectors or None -> dict of DENSE_OUT"""
    N = v.ChanQ.size
    o = {}
    side = np.array(v.ToChanM3RunoffDt, dtype=np.float64, copy=True)
    if options.get("openwaterevapo"):
        side = side - d["EvaAddM3Dt"]
    if options.get("wateruse"):                                                           # routing.py:466-468
        side = side - (d["withdrawal_CH_actual_M3_routStep"] - d["returnflow_GwAbs2Channel_M3_routStep"])
    if options.get("inflow"):                                                             # inflow.py:142-144
        qin = (v.QInM3Old + (step + 1) * v.QDelta) * v.InvNoRoutSteps
        o["QInDt"] = qin
        o["QinADDEDM3"] = (0.0 if step < 1 else v.QinADDEDM3) + qin
        side = side + qin
    if options.get("TransLoss"):                                                          # transmission.py:76-87
        q = v.ChanQ
        below = q.copy()
        for p in np.nonzero(v.UpTrans)[0]:
            below[p] = math.pow(math.pow(q[p], v.TransPower2) - v.TransSub, v.TransPower1)
        loss = (q - below) * v.DtRouting
        o["TransLossM3Dt"], o["TransCum"] = loss, v.TransCum + loss
        side = side - loss
    if lake_out is not None:
        side = side + lake_out
    if res_out is not None:
        side = side + res_out
    if options.get("simulatePolders"):
        side = side - d["ChannelToPolderM3Dt"]
    o["SideflowChanM3"] = side
    assert side.shape == (N,)
    return o


def inloop_reference(d, v, step, options):
    """One lfo_inloop_structures call restated on the namespace `v` (as oracle.InloopStructures keeps it): returns the
    expected values of every vector it writes, and the census intermediates.  v is left unchanged."""
    dt, N = v.DtRouting, v.ChanQ.size
    exp, mid = {}, {}
    lake_out = res_out = None
    if options.get("simulateLakes") and len(v.LakeIndex):
        cells = np.asarray(v.LakeIndex)
        state = {k: getattr(v, k, None) for k in LAKE_STATE}
        if step == 0:
            state["LakeStorageM3CC"] = np.asarray(v.LakeStorageM3)[cells]                 # lakes.py:212-213
        o, mid["lake"] = lake_reference({k: np.asarray(getattr(v, k), np.float64) for k in LAKE_PARAM}, state,
                                        site_inflow(v.downstruct, v.ChanQ, cells), dt)
        lake_out = np.array(getattr(v, "QLakeOutM3Dt", np.zeros(N)), copy=True)
        lake_out[cells] = o.pop("QLakeOut")
        exp.update(o, QLakeOutM3Dt=lake_out)
    if options.get("simulateReservoirs") and len(v.ReservoirIndex):
        cells = np.asarray(v.ReservoirIndex)
        storage = np.asarray(v.ReservoirStorageM3)[cells] if step == 0 else v.ReservoirStorageM3CC   # reservoir.py:195-196
        o, mid["res"] = reservoir_reference({k: np.asarray(getattr(v, k), np.float64) for k in RES_PARAM}, storage,
                                            site_inflow(v.downstruct, v.ChanQ, cells), dt)
        res_out = np.array(getattr(v, "QResOutM3Dt", np.zeros(N)), copy=True)
        res_out[cells] = o.pop("QResOut")
        exp.update(o, QResOutM3Dt=res_out)
    exp.update(dense_reference(d, v, step, options, lake_out, res_out))
    return exp, mid


# ----------------------------------------------------------------------------------------------------------------------
# the sites inside the routing loop of a 120 x 160 raster
# ----------------------------------------------------------------------------------------------------------------------
LOOP_SHAPE = (120, 160)
LOOP_SITES = (130, 190)
LOOP_OPTION_SETS = {
    "everything": dict(ALL_OPTIONS, openwaterevapo=True, wateruse=True, simulatePolders=True),
    "lakes": dict(simulateLakes=True),
    "reservoirs": dict(simulateReservoirs=True),
    "inflow_transloss": dict(inflow=True, TransLoss=True),
}


def loop_inputs(family, seed=17):
    """-> (attributes of a routing `var` with split routing on a 120 x 160 all-land raster, the structures' attributes,
    the cut LDD, the land mask).  130 lakes + 190 reservoirs, none of them the downstream neighbour of another site
    (a site's inflow is then routed discharge only, never another site's cell).  The reservoirs start spread over all
    five regimes; a few are small against their rule outflow (out > storage), a few start above capacity, two are missing
    from the table (total = 0) and two lakes start with an outflow their storage cannot give (storage < 0 / NaN)."""
    import oracle as orc
    from lisflood_amd import synthetic as syn
    H, W = LOOP_SHAPE
    N = H * W
    n_lakes, n_res = LOOP_SITES
    mask = np.ones((H, W), bool)
    codes = syn.make_ldd(family, H, W, 8).reshape(-1).astype(np.float64)
    p = syn.router_params(N, seed=4)
    rng = np.random.default_rng(seed)
    beta, dt, nsteps = p["beta"], 3600.0, 24
    alpha, length = p["alpha"], p["dx"]
    alpha2 = alpha * rng.uniform(1.2, 2.0, N)
    qlimit = 2.0 * p["Q0"] * rng.uniform(0.3, 1.2, N)
    r = dict(ChanLength=length, InvChanLength=1 / length, ChannelAlpha=alpha, InvChannelAlpha=1 / alpha, ChannelAlpha2=alpha2,
             InvChannelAlpha2=1 / alpha2, QLimit=qlimit, M3Limit=alpha * length * qlimit ** beta,
             Chan2M3Start=alpha2 * length * qlimit ** beta, Chan2QStart=qlimit * 0.1, PixelArea=np.full(N, 2.5e7),
             IsChannelKinematic=np.ones(N, bool), Beta=beta, InvBeta=1 / beta, DtRouting=dt, InvDtRouting=1 / dt,
             NoRoutSteps=nsteps, InvNoRoutSteps=1 / nsteps, DtSec=dt * nsteps,
             ToChanM3RunoffDt=syn.lateral_inflow(N, 0) * length * dt)
    r["Chan2M3Kin"] = r["Chan2M3Start"].copy()
    r["ChanM3Kin"] = alpha * length * p["Q0"] ** beta
    r["ChanQKin"] = p["Q0"].copy()
    r["Chan2QKin"] = (r["Chan2M3Kin"] / length / alpha2) ** (1 / beta)
    r["ChanQ"] = r["ChanQKin"].copy()
    for k in ("CrossSection2Area", "Sideflow1Chan", "sumDisDay"):
        r[k] = np.zeros(N)
    # ---- sites: something upstream, something downstream, and no other site just downstream ----
    down = orc.lookups(codes, mask)[0].astype(np.int64)          # -1: a pit
    nups = np.bincount(down[down >= 0], minlength=N)
    cand = rng.permutation(np.nonzero((nups > 0) & (down >= 0))[0])
    is_site = np.zeros(N, bool)
    below_site = np.zeros(N, bool)                    # cells a chosen site drains straight into
    sites = []
    for c in cand:
        if len(sites) == n_lakes + n_res:
            break
        if is_site[down[c]] or below_site[c]:         # the cell downstream of c is a site / a site drains into c
            continue
        sites.append(c); is_site[c] = True
        below_site[down[c]] = True
    sites = np.array(sites)
    assert sites.size == n_lakes + n_res and not is_site[down[sites]].any()
    lake, res = np.sort(sites[:n_lakes]), np.sort(sites[n_lakes:])

    def last_on_its_river(cells):
        """the first two of `cells` with no site anywhere downstream: what they let out reaches no other site"""
        found = []
        for i, c in enumerate(cells):
            c = down[c]
            while c >= 0 and not is_site[c]:
                c = down[c]
            if c < 0:
                found.append(i)
        return found[:2]
    (nan_lake, _), (nan_res, empty) = last_on_its_river(lake), last_on_its_river(res)      # the sites that turn NaN
    ups = (down >= 0) & is_site[np.maximum(down, 0)]
    cut = codes.copy(); cut[ups] = 5.0
    ds = np.where(down >= 0, down, N).astype(np.int32); ds[codes == 5] = N
    qin = np.bincount(ds, weights=r["ChanQ"], minlength=N + 1)
    s = dict(downstruct=ds, LakeIndex=lake, ReservoirIndex=res)
    lakes, lake_storage = _random_lakes(rng, n_lakes, dt, qin[lake])
    s.update(lakes)
    # si = -5 at the first sub-step: storage < 0 and reset, or LakeFactorSqr + 2 si < 0 and NaN from then on
    for i, factor in (((1 if nan_lake == 0 else 0), 100.0), (nan_lake, 1.0)):
        s["LakeFactor"][i], s["LakeFactorSqr"][i], s["LakeOutflowCC"][i] = factor, factor * factor, 2 * qin[lake[i]] + 10.0
        s["LakeInflowOldCC"][i], lake_storage[i] = qin[lake[i]], 0.0
    s["LakeStorageM3"] = np.zeros(N); s["LakeStorageM3"][lake] = lake_storage
    s.update(_random_reservoirs(rng, n_res, qin[res]))
    fill = rng.uniform(0.0, 1.05, n_res)
    fill[:4] = (1.5, 1.3, 0.6, 0.6)
    s["TotalReservoirStorageM3CC"][2:4] = 1e3         # small against qnorm * DtRouting: out > storage
    s["TotalReservoirStorageM3CC"][[nan_res, empty]] = 0.0      # missing from the table: fill = inf, NaN from then on
    storage = fill * s["TotalReservoirStorageM3CC"]
    storage[nan_res] = 1e6                            # (`empty` holds nothing at first, its inflow then makes fill inf too)
    s["ReservoirStorageM3"] = np.zeros(N); s["ReservoirStorageM3"][res] = storage
    s["QInM3Old"], s["QDelta"] = np.zeros(N), np.zeros(N)
    pts = rng.choice(N, 32, replace=False)
    s["QInM3Old"][pts] = rng.uniform(1e4, 2e5, 32); s["QDelta"][pts] = rng.uniform(0.0, 2e3, 32)
    s["UpTrans"] = (rng.random(N) < 0.3) & (r["ChanQ"] > 1.0)
    s["TransPower1"], s["TransPower2"], s["TransSub"] = 1 / 0.95, 0.95, 1e-9
    s["TransCum"] = np.zeros(N)
    runoff = r["ToChanM3RunoffDt"]
    s["EvaAddM3Dt"] = 0.05 * runoff * rng.uniform(0.0, 1.0, N)
    s["withdrawal_CH_actual_M3_routStep"] = 0.10 * runoff * rng.uniform(0.0, 1.0, N)
    s["returnflow_GwAbs2Channel_M3_routStep"] = 0.04 * runoff * rng.uniform(0.0, 1.0, N)
    s["ChannelToPolderM3Dt"] = 0.05 * runoff * (rng.random(N) < 0.1)
    return r, s, cut, mask


def loop_var(r, s):
    v = types.SimpleNamespace()
    for d in (r, s):
        for k, x in d.items():
            setattr(v, k, np.array(x, copy=True) if isinstance(x, np.ndarray) else x)
    return v


_loop_runs = {}


def loop_oracle_run(orc, family, name):
    """The 24 sub-steps of a model step by the oracle alone (structures, then the split-routing sub-step), computed once
    per (family, option set) -> (the `var` namespace at the end, the reservoir census summed over the sub-steps)"""
    key = (family, name)
    if key not in _loop_runs:
        r, s, cut, mask = loop_inputs(family)
        options = LOOP_OPTION_SETS[name]
        v = loop_var(r, s)
        kw = orc.kinematicWave(cut, mask, r["ChannelAlpha"], r["Beta"], r["ChanLength"], r["DtRouting"],
                               alpha_floodplains=r["ChannelAlpha2"])
        st, sub = orc.InloopStructures(v, options), orc.RoutingSubstep(kw, v)
        params = {k: np.asarray(s[k], np.float64) for k in RES_PARAM}
        census = {}
        for step in range(int(v.NoRoutSteps)):
            if options.get("simulateReservoirs"):
                before = (np.asarray(v.ReservoirStorageM3)[s["ReservoirIndex"]] if step == 0 else v.ReservoirStorageM3CC).copy()
            st.dynamic_inloop(step)
            if options.get("simulateReservoirs"):
                _, mid = reservoir_reference(params, before, v.ReservoirInflowCC, v.DtRouting)
                for k, n in reservoir_census(mid).items():
                    census[k] = census.get(k, 0) + n
            sub.dynamic(split=True, sideflow_m3=v.SideflowChanM3)
        _loop_runs[key] = (v, census)
    return _loop_runs[key]
