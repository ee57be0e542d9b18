"""Snow and frost (lf_snow_frost_members_device, lisflood_amd.snow_frost): the numpy restatement of the arithmetic that
include/lisflood_amd.h states -- the contract the kernel is held to --, the same arithmetic element by element with the
operations handed in (plain Python floats, or mpmath at 240 bits rounded to a double after every operation), seeded input
families that put elements on both sides and on the ties of every comparison, and a census that shows it from the values.
A plain helper module: tests/test_snow_frost_cpu.py pins the restatement, tests/test_snow_frost_gpu.py and
tests/test_hotpath_meteo_gpu.py run the same inputs through the kernel.

Signed zeros: np.maximum(-0.0, 0.0) may give either zero (its SIMD loops and its scalar loop differ).  It does not show:
the second operand of every maximum here is the literal +0.0, a melt term is +0.0, positive or NaN before the ice term
(-0.0 for a cold pixel outside the ice season) is ADDED to it, and a frost index is never -0.0.  same_bits counts the sign of
a zero, so the tests would say if that were wrong.
"""
import math

import numpy as np

from module_edges import same_bits, first_difference, spots, counts_table  # noqa: F401 (read from here by the tests)

SENTINEL = -12345.678
SCALARS = dict(TempSnow=1.0, TempMelt=0.0, IceMeltCoef=7.0, DtDay=0.5, Afrost=0.97, SnowWaterEquivalent=0.45,
               FrostIndexThreshold=56.0)
STATICS = ("DeltaTSnow", "SnowMeltCoef", "SnowFactor")
# (SnowSeasonTerm, SummerSeason) of the four steps: the ice season off, on, on, off; the first pair is exact in binary, which
# the planted melt tie needs
SEASONS = ((0.5, 0.0), (0.25, 0.5), (-0.5, 0.75), (0.7071, 0.0))
OUTPUTS = ("Rain", "SnowMelt", "Snow", "SnowCover")


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
def exp_rounded(x):
    """exp of every element, correctly rounded: mpmath at 240 bits, rounded to the nearest double"""
    import mpmath
    x = np.asarray(x, np.float64)
    out = np.empty(x.shape)
    with mpmath.workprec(240):
        flat, o = x.reshape(-1), out.reshape(-1)
        for i in range(flat.size):
            o[i] = float(mpmath.exp(mpmath.mpf(float(flat[i])))) if flat[i] == flat[i] else flat[i]
    return out


def snow_step(par, zones, precipitation, tavg, season, trace=None):
    """snow.dynamic: zones [..., 3, N] and the meteo rows [..., N] -> dict(SnowCoverS, Rain, SnowMelt, Snow, SnowCover).
    trace: a dict that receives what the census counts."""
    delta, factor = par["DeltaTSnow"], par["SnowFactor"]
    seas = season[0] + par["SnowMeltCoef"]
    P, T = np.asarray(precipitation, np.float64), np.asarray(tavg, np.float64)
    new = np.empty(np.broadcast_shapes(zones.shape, P.shape[:-1] + (3,) + P.shape[-1:]))
    snow = rain = melt = cover = 0.0
    with np.errstate(all="ignore"):
        for i in range(3):
            tavg_s = T + delta * float(i - 1)
            snow_s = np.where(tavg_s < par["TempSnow"], factor * P, 0.0)
            rain_s = np.where(tavg_s >= par["TempSnow"], P, 0.0)
            melt_s = np.maximum((tavg_s - par["TempMelt"]) * seas * (1 + 0.01 * rain_s) * par["DtDay"], 0.0)
            ice_s = np.maximum((T if i < 2 else tavg_s) * par["IceMeltCoef"] * par["DtDay"] * season[1], 0.0)
            wanted = melt_s + ice_s
            melt_s = np.maximum(np.minimum(wanted, zones[..., i, :]), 0.0)
            new[..., i, :] = zones[..., i, :] + snow_s - melt_s
            snow = snow + snow_s
            rain = rain + rain_s
            melt = melt + melt_s
            cover = cover + new[..., i, :]
            if trace is not None:
                trace.setdefault("zones", []).append(dict(tavg_s=tavg_s, warm=tavg_s - par["TempMelt"], wanted=wanted,
                                                          pack=np.broadcast_to(zones[..., i, :], wanted.shape)))
        return dict(SnowCoverS=new, Rain=rain / 3, SnowMelt=melt / 3, Snow=snow / 3, SnowCover=cover / 3)


def frost_step(par, frost, cover, tavg, exp=np.exp, trace=None):
    """frost.dynamic -> dict(FrostIndex, isFrozenSoil); exp: the exponential of an array"""
    T = np.asarray(tavg, np.float64)
    with np.errstate(all="ignore"):
        kfrost = np.where(T < 0, 0.08, 0.5)
        e = exp(-0.04 * kfrost * cover / par["SnowWaterEquivalent"])
        rate = -(1 - par["Afrost"]) * frost - T * e
        raw = frost + rate * par["DtDay"]
        new = np.maximum(raw, 0.0)
    if trace is not None:
        trace.update(raw=raw, e=e, cover=np.broadcast_to(cover, raw.shape), tavg=np.broadcast_to(T, raw.shape))
    return dict(FrostIndex=new, isFrozenSoil=new > par["FrostIndexThreshold"])


def step(par, zones, frost, precipitation, tavg, season, exp=np.exp, trace=None):
    """snow.dynamic followed by frost.dynamic -> dict of the two states, the four outputs and isFrozenSoil"""
    out = snow_step(par, zones, precipitation, tavg, season, trace)
    out.update(frost_step(par, frost, out["SnowCover"], tavg, exp, trace))
    return out


def run(x, exp=np.exp, steps=None, traces=None):
    """the steps of an input family from its initial state -> list of step() results"""
    zones, frost, out = x["SnowCoverS"], x["FrostIndex"], []
    for s in range(len(x["seasons"]) if steps is None else steps):
        trace = None if traces is None else {}
        out.append(step(x, zones, frost, x["Precipitation"][s], x["Tavg"][s], x["seasons"][s], exp, trace))
        zones, frost = out[-1]["SnowCoverS"], out[-1]["FrostIndex"]
        if traces is not None:
            traces.append(trace)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the same arithmetic for one element, the operations handed in
# ----------------------------------------------------------------------------------------------------------------------
class FloatOps:
    """Python floats: every operation one IEEE operation"""
    add = staticmethod(lambda a, b: a + b)
    sub = staticmethod(lambda a, b: a - b)
    mul = staticmethod(lambda a, b: a * b)

    @staticmethod
    def div(a, b):
        return a / b if b != 0 else float(np.float64(a) / np.float64(b))

    @staticmethod
    def exp(a):
        return float(exp_rounded(np.array([a]))[0])


class MpOps:
    """mpmath at 240 bits, rounded to the nearest double after every operation.  A product of two doubles is exact in 106
    bits; a sum and a quotient are rounded twice, at 240 and at 53 bits, which differs from one rounding only for a value
    within 2^-187 of a tie."""

    @staticmethod
    def _op(f, a, b):
        import mpmath
        if a != a or b != b or math.isinf(a) or math.isinf(b):
            return float(f(np.float64(a), np.float64(b)))
        with mpmath.workprec(240):
            r = f(mpmath.mpf(a), mpmath.mpf(b))
            if r == 0:                   # (mpmath has one zero: the sign is IEEE's)
                return float(f(np.float64(a), np.float64(b)))
            return float(r)
    add = classmethod(lambda c, a, b: c._op(lambda p, q: p + q, a, b))
    sub = classmethod(lambda c, a, b: c._op(lambda p, q: p - q, a, b))
    mul = classmethod(lambda c, a, b: c._op(lambda p, q: p * q, a, b))
    div = classmethod(lambda c, a, b: c._op(lambda p, q: p / q, a, b) if b != 0 else float(np.float64(a) / np.float64(b)))
    exp = staticmethod(FloatOps.exp)


def npmax(a, b):
    return a if a != a else (b if b != b else (b if b > a else a))


def npmin(a, b):
    return a if a != a else (b if b != b else (b if b < a else a))


def element_step(o, par, p, zones, frost, P, T, season):
    """step() for pixel p of one member: zones [3] floats, frost, P, T floats -> (zones, frost, Rain, SnowMelt, Snow,
    SnowCover, isFrozenSoil)"""
    delta, factor = float(par["DeltaTSnow"][p]), float(par["SnowFactor"][p])
    seas = o.add(season[0], float(par["SnowMeltCoef"][p]))
    snow = rain = melt = cover = 0.0
    new = [0.0, 0.0, 0.0]
    for i in range(3):
        tavg_s = o.add(T, o.mul(delta, float(i - 1)))
        snow_s = o.mul(factor, P) if tavg_s < par["TempSnow"] else 0.0
        rain_s = P if tavg_s >= par["TempSnow"] else 0.0
        m = o.mul(o.mul(o.mul(o.sub(tavg_s, par["TempMelt"]), seas), o.add(1.0, o.mul(0.01, rain_s))), par["DtDay"])
        melt_s = npmax(m, 0.0)
        ice_s = npmax(o.mul(o.mul(o.mul(T if i < 2 else tavg_s, par["IceMeltCoef"]), par["DtDay"]), season[1]), 0.0)
        melt_s = npmax(npmin(o.add(melt_s, ice_s), zones[i]), 0.0)
        new[i] = o.sub(o.add(zones[i], snow_s), melt_s)
        snow, rain, melt, cover = o.add(snow, snow_s), o.add(rain, rain_s), o.add(melt, melt_s), o.add(cover, new[i])
    snow, rain, melt, cover = o.div(snow, 3.0), o.div(rain, 3.0), o.div(melt, 3.0), o.div(cover, 3.0)
    kfrost = 0.08 if T < 0 else 0.5
    e = o.exp(o.div(o.mul(o.mul(-0.04, kfrost), cover), par["SnowWaterEquivalent"]))
    rate = o.sub(o.mul(-o.sub(1.0, par["Afrost"]), frost), o.mul(T, e))
    frost = npmax(o.add(frost, o.mul(rate, par["DtDay"])), 0.0)
    return new, frost, rain, melt, snow, cover, frost > par["FrostIndexThreshold"]


def elements_step(o, x, zones, frost, s, member=0):
    """step s of one member from the state (zones [members, 3, N], frost [members, N]), element by element through the
    operations `o` -> dict like step()'s"""
    N = x["DeltaTSnow"].size
    r = dict(SnowCoverS=np.empty((3, N)), FrostIndex=np.empty(N), Rain=np.empty(N), SnowMelt=np.empty(N), Snow=np.empty(N),
             SnowCover=np.empty(N), isFrozenSoil=np.empty(N, bool))
    for p in range(N):
        z, f, rain, melt, snow, cover, frozen = element_step(
            o, x, p, [float(v) for v in zones[member, :, p]], float(frost[member, p]), float(x["Precipitation"][s][member, p]),
            float(x["Tavg"][s][member, p]), x["seasons"][s])
        r["SnowCoverS"][:, p], r["FrostIndex"][p], r["Rain"][p], r["SnowMelt"][p] = z, f, rain, melt
        r["Snow"][p], r["SnowCover"][p], r["isFrozenSoil"][p] = snow, cover, frozen
    return r


# ----------------------------------------------------------------------------------------------------------------------
# how far a device FrostIndex may lie from the reference one
# ----------------------------------------------------------------------------------------------------------------------
def frost_bound(par, frost, trace, E):
    """Per element: the largest |FrostIndex - reference| of an implementation whose exp value lies within E ulps of the
    reference's exp value e (the reference: frost_step with exp_rounded, its intermediates in `trace`) and whose other
    operations are IEEE.  The difference E ulp(e) goes through t = Tavg * e, rate = a - t, rate * DtDay and FrostIndex + that;
    every one of these four results is rounded on both sides, half an ulp each -- the ulp of the reference's value on one
    side and of the largest value the other side can have on the other (a power of two may lie between them).  The maximum
    with 0 widens nothing."""
    T, e, dt = np.abs(trace["tavg"]), trace["e"], par["DtDay"]

    def rounded(ref, err):
        ref = np.abs(ref)
        return err + 0.5 * np.spacing(ref) + 0.5 * np.spacing(ref + err)
    with np.errstate(all="ignore"):
        t = trace["tavg"] * e
        rate = -(1 - par["Afrost"]) * frost - t
        err = rounded(t, T * E * np.spacing(e))
        err = rounded(rate, err)
        err = rounded(rate * dt, err * dt)
        err = rounded(trace["raw"], err)
    # no snow cover: the argument of exp is a zero, exp is exactly 1 on both sides and so is every operation behind it
    return np.where(trace["cover"] == 0, 0.0, err)


# ----------------------------------------------------------------------------------------------------------------------
# input families
# ----------------------------------------------------------------------------------------------------------------------
def _base(N, members, seed, steps):
    rng = np.random.default_rng(seed)
    x = dict(SCALARS)
    x["seasons"] = list(SEASONS[:steps])
    x["DeltaTSnow"] = rng.uniform(0.0, 4.0, N)
    x["SnowMeltCoef"] = rng.uniform(2.0, 6.0, N)
    x["SnowFactor"] = rng.uniform(0.8, 1.2, N)
    return rng, x


def inputs(N, members=1, seed=11, steps=4, nan=True):
    """The general family: seeded uniform values -- Tavg in [-15, 15], precipitation on six pixels of ten, packs in six zones
    of ten, FrostIndex in [0, 100] around the threshold of 56 -- and the planted cases of plant() where N has room for them
    (N >= 64; smaller N get as many as fit, the census is taken at N >= 257; nan=False: without the four NaN).  -> dict: the statics [N], the scalars,
    SnowCoverS [members, 3, N], FrostIndex [members, N], Precipitation / Tavg [steps][members, N], seasons."""
    rng, x = _base(N, members, seed, steps)
    x["SnowCoverS"] = rng.uniform(0.0, 50.0, (members, 3, N)) * (rng.random((members, 3, N)) < 0.6)
    x["FrostIndex"] = rng.uniform(0.0, 100.0, (members, N))
    x["Precipitation"] = [rng.uniform(0.0, 20.0, (members, N)) * (rng.random((members, N)) < 0.6) for _ in range(steps)]
    x["Tavg"] = [rng.uniform(-15.0, 15.0, (members, N)) for _ in range(steps)]
    plant(x, N, nan)
    return x


def exact_inputs(N, members=1, seed=12, steps=4):
    """The exact family: every pack empty and no snow falls -- a pixel is warm in all three zones (Tavg >= 6, DeltaTSnow <= 4)
    or has no precipitation -- so SnowCover stays 0, the argument of exp is a zero, exp is exactly 1 and the frost line is
    exact.  It holds the planted threshold ties."""
    rng, x = _base(N, members, seed, steps)
    x["SnowCoverS"] = np.zeros((members, 3, N))
    x["FrostIndex"] = rng.uniform(0.0, 100.0, (members, N)) * (rng.random((members, N)) < 0.8)
    dry = rng.random((members, N)) < 0.4
    x["Precipitation"] = [np.where(dry, 0.0, rng.uniform(0.0, 20.0, (members, N))) for _ in range(steps)]
    x["Tavg"] = [np.where(dry, rng.uniform(-20.0, 10.0, (members, N)), rng.uniform(6.0, 25.0, (members, N))) for _ in range(steps)]
    plant_threshold(x, N, 0)
    return x


def plant_threshold(x, N, k0):
    """FrostIndex exactly the threshold (not frozen) and one ulp above it (frozen) after step 0, on pixels without snow
    cover and without precipitation: FrostIndex 0, so rate = -0.0 - Tavg * 1 and FrostIndex = 0 + (-Tavg) * 0.5 -- Tavg =
    -112 and the double below it."""
    thr, dt = x["FrostIndexThreshold"], x["DtDay"]
    for k, tavg in ((k0, -thr / dt), (k0 + 1, -np.nextafter(thr, np.inf) / dt)):
        for p in spots(k, N):
            x["SnowCoverS"][:, :, p], x["FrostIndex"][:, p] = 0.0, 0.0
            x["Precipitation"][0][:, p], x["Tavg"][0][:, p] = 0.0, tavg


def plant(x, N, nan=True):
    """the cases of the census that random values do not give, at fixed places (spots): each on every member, at step 0"""
    P, T = x["Precipitation"][0], x["Tavg"][0]
    cases = [
        dict(delta=2.0, tavg=3.0),                         # zone 0: TavgS = 3 - 2 = TempSnow, the tie: it rains
        dict(delta=2.0, tavg=1.0),                         # zone 1 tie
        dict(delta=2.0, tavg=-1.0),                        # zone 2 tie
        dict(delta=2.0, tavg=2.0),                         # zone 0: TavgS - TempMelt = 0
        dict(delta=2.0, tavg=2.0, coef=3.5, prec=0.0, zone1=4.0),   # zone 1: melt 2 * (0.5 + 3.5) * 1 * 0.5 = 4 = the pack
        dict(tavg=-0.0), dict(tavg=0.0),
        dict(tavg=12.0, frost=1.0, zones=0.0),             # FrostIndex clamped at 0, no cover
    ]
    if nan:
        cases += [dict(prec=np.nan), dict(tavg=np.nan), dict(zone1=np.nan), dict(frost=np.nan)]
    if N < 3 * (len(cases) + 2):
        cases = cases[:max(0, N // 3 - 2)]
    for k, c in enumerate(cases):
        for p in spots(k + 2, N):
            if "delta" in c: x["DeltaTSnow"][p] = c["delta"]
            if "coef" in c: x["SnowMeltCoef"][p] = c["coef"]
            if "tavg" in c: T[:, p] = c["tavg"]
            if "prec" in c: P[:, p] = c["prec"]
            if "zone1" in c: x["SnowCoverS"][:, 1, p] = c["zone1"]
            if "zones" in c: x["SnowCoverS"][:, :, p] = c["zones"]
            if "frost" in c: x["FrostIndex"][:, p] = c["frost"]
    if N >= 12:
        plant_threshold(x, N, 0)


def census(x, traces):
    """how many (step, member, pixel) elements take each side of each comparison: from the inputs and the restatement's
    intermediates (run(x, traces=...)) alone"""
    n = lambda m: int(np.count_nonzero(m))
    out = {}
    cat = lambda f: np.stack([f(s, tr) for s, tr in enumerate(traces)])
    for i in range(3):
        ts = cat(lambda s, tr: tr["zones"][i]["tavg_s"])
        out["zone %d: TavgS < TempSnow" % i] = n(ts < x["TempSnow"])
        out["zone %d: TavgS == TempSnow (rain)" % i] = n(ts == x["TempSnow"])
        out["zone %d: TavgS > TempSnow" % i] = n(ts > x["TempSnow"])
    warm = cat(lambda s, tr: np.stack([z["warm"] for z in tr["zones"]]))
    wanted = cat(lambda s, tr: np.stack([z["wanted"] for z in tr["zones"]]))
    pack = cat(lambda s, tr: np.stack([z["pack"] for z in tr["zones"]]))
    out["TavgS - TempMelt < 0"], out["TavgS - TempMelt == 0"], out["TavgS - TempMelt > 0"] = n(warm < 0), n(warm == 0), n(warm > 0)
    out["melt limited by the pack"] = n((wanted > pack) & (pack > 0))
    out["melt not limited"] = n((wanted < pack) & (wanted > 0))
    out["melt exactly the pack"] = n((wanted == pack) & (pack > 0))
    out["empty zone"] = n(pack == 0)
    P, T = np.stack(x["Precipitation"][:len(traces)]), np.stack(x["Tavg"][:len(traces)])
    out["zero precipitation"] = n(P == 0)
    summer = np.array([s[1] for s in x["seasons"][:len(traces)]])[:, None, None]
    out["SummerSeason == 0"] = n((summer == 0) & (T == T))
    out["SummerSeason > 0, Tavg > 0 (ice melts)"] = n((summer > 0) & (T > 0))
    out["SummerSeason > 0, Tavg < 0 (clamped)"] = n((summer > 0) & (T < 0))
    out["Tavg < 0"], out["Tavg > 0"] = n(T < 0), n(T > 0)
    out["Tavg == -0.0"], out["Tavg == +0.0"] = n((T == 0) & np.signbit(T)), n((T == 0) & ~np.signbit(T))
    raw, cover = cat(lambda s, tr: tr["raw"]), cat(lambda s, tr: tr["cover"])
    thr = x["FrostIndexThreshold"]
    out["FrostIndex clamped at 0"] = n(raw < 0)
    out["FrostIndex == threshold, no cover (not frozen)"] = n((raw == thr) & (cover == 0))
    out["FrostIndex one ulp above threshold, no cover (frozen)"] = n((raw == np.nextafter(thr, np.inf)) & (cover == 0))
    out["frozen"], out["not frozen"] = n(raw > thr), n(raw <= thr)
    out["without snow cover"] = n(cover == 0)
    out["NaN Precipitation"], out["NaN Tavg"] = n(np.isnan(P)), n(np.isnan(T))
    out["NaN zone"] = n(np.isnan(x["SnowCoverS"]))
    out["NaN FrostIndex"] = n(np.isnan(x["FrostIndex"]))
    return out


def inside_threshold(x, exp=exp_rounded, E=1.0):
    """per step: (reference results, bound, elements whose reference FrostIndex lies within the bound of the threshold), the
    restatement following its own trajectory"""
    out, zones, frost = [], x["SnowCoverS"], x["FrostIndex"]
    for s in range(len(x["seasons"])):
        trace = {}
        r = step(x, zones, frost, x["Precipitation"][s], x["Tavg"][s], x["seasons"][s], exp, trace)
        bound = frost_bound(x, frost, trace, E)
        with np.errstate(invalid="ignore"):
            inside = (bound > 0) & (np.abs(r["FrostIndex"] - x["FrostIndexThreshold"]) <= bound)
        out.append((r, bound, inside))
        zones, frost = r["SnowCoverS"], r["FrostIndex"]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the member rows of one call of lf_snow_frost_members_device as the device holds them, with sentinels in every gap
# ----------------------------------------------------------------------------------------------------------------------
GAP_BYTE = 0xA5
HALVES = ("both", "snow", "frost")


class Layout:
    """Host images of every vector of a call: SnowCoverS rows 3 N + pad apart, the [N] rows and the byte row N + pad apart,
    Precipitation / Tavg rows N + pad apart (per_member) or one row; SENTINEL (GAP_BYTE in the byte row) in every gap and in
    every output.  halves: "both", "snow" (no FrostIndex, no isFrozenSoil), "frost" (no SnowCoverS; SnowCover is an input).
    device(par, season): upload, one call, download -- the images then hold what the device holds."""

    def __init__(self, N, members, pad, per_member, snow_row, halves):
        self.N, self.M, self.pad, self.per_member, self.halves = N, members, pad, per_member, halves
        self.zstride, self.rstride = 3 * N + pad, N + pad
        self.fstride = self.rstride if per_member else 0
        f = lambda rows, stride: np.full((rows, stride), SENTINEL)
        self.h = {"Tavg": f(members if per_member else 1, self.rstride), "SnowCover": f(members, self.rstride)}
        if halves != "frost":
            self.h.update(Precipitation=f(members if per_member else 1, self.rstride), SnowCoverS=f(members, self.zstride),
                          Rain=f(members, self.rstride), SnowMelt=f(members, self.rstride))
            if snow_row:
                self.h["Snow"] = f(members, self.rstride)
        if halves != "snow":
            self.h["FrostIndex"] = f(members, self.rstride)
            self.h["isFrozenSoil"] = np.full((members, self.rstride), GAP_BYTE, np.uint8)

    def width(self, k):
        return 3 * self.N if k == "SnowCoverS" else self.N

    def put(self, k, rows):
        if k in self.h:
            rows = np.asarray(rows, np.float64)
            self.h[k][:, :self.width(k)] = rows.reshape(-1, self.width(k))[:self.h[k].shape[0]]

    def get(self, k):
        a = self.h[k][:, :self.width(k)]
        return a.reshape(self.M, 3, self.N) if k == "SnowCoverS" else a

    def gaps_untouched(self):
        for k, a in self.h.items():
            g = a[:, self.width(k):]
            if not (g == (GAP_BYTE if a.dtype == np.uint8 else SENTINEL)).all():
                return k
        return None

    def forcing(self, x, s):
        """Precipitation / Tavg of step s: member rows, or member 0's row for all"""
        P, T = x["Precipitation"][s], x["Tavg"][s]
        return (P, T) if self.per_member else (P[:1], T[:1])

    def device(self, par, season, lib_module, snow_frost_module):
        import ctypes as C
        D = {k: lib_module.DeviceArray.from_host(np.ascontiguousarray(a.reshape(-1)), 0) for k, a in self.h.items()}
        for k in STATICS:
            if self.halves != "frost":
                D[k] = lib_module.DeviceArray.from_host(np.ascontiguousarray(par[k]), 0)
        a = snow_frost_module.fill_scalars(snow_frost_module._SnowFrostArgs(), par, self.N)
        a.SnowSeasonTerm, a.SummerSeason = season
        for k, d in D.items():
            setattr(a, k, d.ptr.value)
        try:
            lib_module.check(lib_module.lib().lf_snow_frost_members_device(0, C.byref(a), self.M, self.zstride, self.rstride,
                                                                           self.fstride))
            for k in self.h:
                self.h[k] = D[k].download().reshape(self.h[k].shape)
        finally:
            for d in D.values():
                d.free()

    def fake(self, par, season, exp=np.exp):
        """what device() does, from the restatement (a rehearsal of the harness without a device)"""
        T = self.get("Tavg")
        cover = self.get("SnowCover")
        if self.halves != "frost":
            r = snow_step(par, self.get("SnowCoverS"), self.get("Precipitation"), T, season)
            for k in ("SnowCoverS", "Rain", "SnowMelt", "Snow", "SnowCover"):
                self.put(k, r[k])
            cover = r["SnowCover"]
        if self.halves != "snow":
            r = frost_step(par, self.get("FrostIndex"), cover, T, exp)
            self.put("FrostIndex", r["FrostIndex"])
            self.h["isFrozenSoil"][:, :self.N] = r["isFrozenSoil"]


def check_steps(x, lay, advance, steps=4):
    """`steps` consecutive updates of layout `lay` (advance(par, season): one call) against the restatement, each step fed
    the layout's own previous state: everything but FrostIndex and isFrozenSoil bit for bit; FrostIndex bit for bit where
    there is no snow cover (exp is exactly 1) and within frost_bound(E = 1) elsewhere; isFrozenSoil wherever the reference
    FrostIndex is further than that bound from the threshold -- and no element may lie inside; the gaps untouched.
    -> the largest |FrostIndex - reference| seen"""
    worst = 0.0
    lay.put("SnowCoverS", x["SnowCoverS"])
    lay.put("FrostIndex", x["FrostIndex"])
    for s in range(steps):
        P, T = lay.forcing(x, s)
        lay.put("Precipitation", P)
        lay.put("Tavg", T)
        zones = lay.get("SnowCoverS").copy() if lay.halves != "frost" else None
        frost = lay.get("FrostIndex").copy() if lay.halves != "snow" else None
        if lay.halves == "frost":               # SnowCover is an input: what snow.dynamic of the family's own run leaves
            cover = run(x, steps=s + 1)[s]["SnowCover"]
            lay.put("SnowCover", cover)
        advance(x, x["seasons"][s])
        assert lay.gaps_untouched() is None, (s, lay.gaps_untouched())
        if lay.halves != "frost":
            want = snow_step(x, zones, P, T, x["seasons"][s])
            for k in ("SnowCoverS",) + OUTPUTS:
                if k in lay.h:
                    got = lay.get(k)
                    assert same_bits(got, np.broadcast_to(want[k], got.shape)), (s, k, first_difference(got, np.broadcast_to(want[k], got.shape)))
            cover = want["SnowCover"]
        if lay.halves != "snow":
            trace = {}
            want = frost_step(x, frost, cover, T, exp_rounded, trace)
            bound = frost_bound(x, frost, trace, 1.0)
            got, ref = lay.get("FrostIndex"), np.broadcast_to(want["FrostIndex"], frost.shape)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (s, "FrostIndex NaN pattern")
            exact = np.broadcast_to(trace["cover"] == 0, ref.shape)
            assert same_bits(got[exact], ref[exact]), (s, "FrostIndex without snow cover", first_difference(got[exact], ref[exact]))
            with np.errstate(invalid="ignore"):
                diff = np.abs(got - ref)
                ok = np.isnan(ref) | (diff <= bound)
                inside = (bound > 0) & (np.abs(ref - x["FrostIndexThreshold"]) <= bound)
            worst = max(worst, float(np.nanmax(np.where(np.isnan(diff), 0.0, diff), initial=0.0)))
            assert ok.all(), (s, "FrostIndex beyond the bound: largest excess %.3g, largest difference %.3g"
                              % (float(np.nanmax(diff - bound)), float(np.nanmax(diff))))
            assert not inside.any(), (s, "a reference FrostIndex within its bound of the threshold", int(inside.sum()))
            frozen = lay.h["isFrozenSoil"][:, :lay.N]
            assert np.array_equal(frozen, np.broadcast_to(want["isFrozenSoil"], frozen.shape).astype(np.uint8)), (s, "isFrozenSoil")
    return worst
