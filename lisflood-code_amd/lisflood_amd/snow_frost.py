"""snow.dynamic and frost.dynamic (three elevation zones) as one device pass: from precipitation and average temperature
to the Rain, SnowMelt and isFrozenSoil the land surface starts from, with the snow pack of the zones (SnowCoverS) and the
frost index carried from step to step (lf_snow_frost_members_device; the arithmetic is stated in include/lisflood_amd.h).

    season_terms(calendar_day, snow_season)     the two per-step scalars the kernel takes as given
    snow, frost                                 module classes on a `var` namespace (reference attribute names), staged
                                                through the host per call like soilloop / surface_routing
    SnowFrostDevice, SnowFrostEnsemble          the resident form: vectors stay in HBM, an ensemble's rows laid out by
                                                soilloop._EnsembleVectors

Not covered: the southern-hemisphere phase shift of the season term, glacier variants, TotalPrecipitation bookkeeping, the
evaporation calibration factors and reading the meteo files."""
import ctypes as C
import math

import numpy as np

from ._lib import BufferCache, check, f64, lib
from .hydro_module import HydroModule
from .soilloop import _EnsembleVectors

STATICS = ("DeltaTSnow", "SnowMeltCoef", "SnowFactor")
SCALARS = ("TempSnow", "TempMelt", "IceMeltCoef", "DtDay", "Afrost", "SnowWaterEquivalent", "FrostIndexThreshold")
STATE = ("SnowCoverS", "FrostIndex")
METEO = ("Precipitation", "Tavg")
_POINTERS = ("Precipitation Tavg SnowCoverS FrostIndex Rain SnowMelt Snow SnowCover isFrozenSoil "
             "DeltaTSnow SnowMeltCoef SnowFactor").split()
_SNOW_OUT = ("Rain", "SnowMelt", "Snow", "SnowCover")


class _SnowFrostArgs(C.Structure):  # lf_snow_frost_args, include/lisflood_amd.h
    _fields_ = ([(k, C.c_void_p) for k in _POINTERS] +
                [(k, C.c_double) for k in SCALARS + ("SnowSeasonTerm", "SummerSeason")] + [("N", C.c_int64)])


def season_terms(calendar_day, snow_season):
    """-> (SnowSeasonTerm, SummerSeason) of a calendar day (1 .. 366): the seasonal variation of the snow melt rate,
    snow_season * sin(radians((day - 81) * 360 / 365.25)), and the ice melt season of the highest zones,
    sin(radians((day - 165) * 180 / (259 - 165))) for 165 < day < 260 and 0 outside (northern hemisphere)."""
    day = calendar_day
    term = snow_season * math.sin(math.radians((day - 81) * 360 / 365.25))
    summer = math.sin(math.radians((day - 165) * 180 / (259 - 165))) if 165 < day < 260 else 0.0
    return term, summer


def check_meteo(meteo, N, members=None):
    """the `meteo` dict of HotPathDevice / HotPathEnsemble / SnowFrostDevice / SnowFrostEnsemble checked -> a copy with
    float64 arrays and float scalars: the three statics [N], the seven scalars, SnowCoverS [3, N] (with members:
    or [members, 3, N]) and FrostIndex [N] (or [members, N]); "Snow": True asks for the Snow row as well"""
    if not isinstance(meteo, dict):
        raise ValueError("meteo must be a dict of %s" % ", ".join(STATICS + SCALARS + STATE))
    known = set(STATICS + SCALARS + STATE + ("Snow",))
    missing, extra = [k for k in STATICS + SCALARS + STATE if k not in meteo], sorted(set(meteo) - known)
    if missing:
        raise ValueError("meteo lacks %s" % ", ".join(missing))
    if extra:
        raise ValueError("meteo holds unknown entries: %s" % ", ".join(extra))
    out = {"Snow": bool(meteo.get("Snow", False))}
    for k in STATICS:
        a = np.asarray(meteo[k], np.float64)
        if a.shape != (N,):
            raise ValueError("meteo[%s] must be [%d]" % (k, N))
        out[k] = a
    for k in SCALARS:
        if np.ndim(meteo[k]) != 0:
            raise ValueError("meteo[%s] must be a scalar" % k)
        out[k] = float(meteo[k])
    for k, shape in (("SnowCoverS", (3, N)), ("FrostIndex", (N,))):
        a = np.asarray(meteo[k], np.float64)
        shapes = [shape] + ([(members,) + shape] if members is not None else [])
        if a.shape not in shapes:
            raise ValueError("meteo[%s] must be %s" % (k, " or ".join(str(list(s)) for s in shapes)))
        out[k] = a
    return out


def fill_scalars(a, meteo, N):
    """the scalar half of an argument block"""
    for k in SCALARS:
        setattr(a, k, float(meteo[k]))
    a.N = N
    return a


def _values(x):
    return np.asarray(getattr(x, "values", x))


class _module(HydroModule):
    """what the two module classes share: `var`, the device, and a BufferCache that lives as long as the module"""

    def __init__(self, var, device=0):
        self.var, self.device = var, device
        self._cache = BufferCache(device)

    def _block(self):
        v = self.var
        N = _values(v.Tavg).shape[-1]
        a = _SnowFrostArgs()
        for k in SCALARS:
            setattr(a, k, float(getattr(v, k, 0.0)))
        a.N = N
        return a, N

    def _row(self, name, N):
        return self._cache.put(name, f64(np.broadcast_to(_values(getattr(self.var, name)), (N,))))


class snow(_module):
    """snow.dynamic on `var`: Precipitation, Tavg, SnowCoverS [3, N], the statics DeltaTSnow / SnowMeltCoef / SnowFactor,
    the scalars TempSnow / TempMelt / IceMeltCoef / DtDay and the step's SnowSeasonTerm / SummerSeason (season_terms)
    -> Snow, Rain, SnowMelt, SnowCover, and SnowCoverS advanced; staged through the host per call"""
    module_name = "Snow"

    def initial(self):
        v = self.var
        if not hasattr(v, "SnowCover"):
            v.SnowCover = _values(v.SnowCoverS).sum(axis=0) / 3.0

    def dynamic(self):
        v = self.var
        a, N = self._block()
        a.SnowSeasonTerm, a.SummerSeason = float(v.SnowSeasonTerm), float(v.SummerSeason)
        dev = {k: self._row(k, N) for k in METEO}
        for k in STATICS:
            dev[k] = self._cache.put_static(k, f64(np.broadcast_to(_values(getattr(v, k)), (N,))))
        zones = f64(_values(v.SnowCoverS))
        if zones.shape != (3, N):
            raise ValueError("SnowCoverS must be [3, %d]" % N)
        dev["SnowCoverS"] = self._cache.put("SnowCoverS", zones)
        for k in _SNOW_OUT:
            dev[k] = self._cache.get(k, N)
        for k, d in dev.items():
            setattr(a, k, d.ptr.value)
        check(lib().lf_snow_frost_members_device(self.device, C.byref(a), 1, 3 * N, N, 0))
        for k in _SNOW_OUT + ("SnowCoverS",):
            setattr(v, k, dev[k].download())


class frost(_module):
    """frost.dynamic on `var`: Tavg, SnowCover (what snow.dynamic left), FrostIndex and the scalars Afrost,
    SnowWaterEquivalent, FrostIndexThreshold, DtDay -> FrostIndex advanced and isFrozenSoil (bool)"""
    module_name = "Frost"

    def dynamic(self):
        v = self.var
        a, N = self._block()
        dev = {k: self._row(k, N) for k in ("Tavg", "SnowCover", "FrostIndex")}
        dev["isFrozenSoil"] = self._cache.get("isFrozenSoil", N, np.uint8)
        for k, d in dev.items():
            setattr(a, k, d.ptr.value)
        check(lib().lf_snow_frost_members_device(self.device, C.byref(a), 1, 0, N, 0))
        v.FrostIndex = dev["FrostIndex"].download()
        v.isFrozenSoil = dev["isFrozenSoil"].download().astype(bool)


class SnowFrostEnsemble(_EnsembleVectors):
    """Snow and frost of an ensemble, device-resident: step(forcing, season) is ONE launch for every member.  meteo: the
    dict check_meteo() describes.  SnowCoverS rows lie 3 N + pad elements apart, every [N] row and the byte row of
    isFrozenSoil N + pad apart (bytes, for the byte row); Precipitation and Tavg as [N] (every member) or [members, N].
    get(name) / set(name, value) / gaps(name) / set_gaps(value): soilloop._EnsembleVectors."""

    def __init__(self, meteo, members, device=0, pad=0):
        N = np.asarray(meteo["DeltaTSnow"]).shape[-1]
        self._setup(members, 3, N, device, pad)
        m = self.meteo = check_meteo(meteo, N, self.members)
        self._member, self._forcing = ["SnowCoverS"], list(METEO) + ["isFrozenSoil"]
        self._pixel = ["FrostIndex", "Rain", "SnowMelt", "SnowCover"] + (["Snow"] if m["Snow"] else [])
        for k in STATICS:
            self._put_static(k, m[k])
        self._put("SnowCoverS", m["SnowCoverS"])
        self._put("FrostIndex", m["FrostIndex"])
        for k in self._pixel[1:] + list(METEO):
            self._put(k, np.zeros(N))
        self._put("isFrozenSoil", np.zeros(N, bool))
        a = self.args = fill_scalars(_SnowFrostArgs(), m, N)
        for k in _POINTERS:
            if k in self.dev:
                setattr(a, k, self.dev[k].ptr.value)

    def forcing_member_stride(self):
        return 0 if all(self._shared_forcing[k] for k in METEO) else self.fstride

    def step(self, forcing=None, season=(0.0, 0.0)):
        """forcing: None (the rows of the step before) or dict of Precipitation / Tavg, [N] or [members, N];
        season: (SnowSeasonTerm, SummerSeason) of the step (season_terms)"""
        for k, x in (forcing or {}).items():
            if k not in METEO:
                raise ValueError("%s is no forcing of this call (%s)" % (k, ", ".join(METEO)))
            self._put(k, x)
        self.args.SnowSeasonTerm, self.args.SummerSeason = float(season[0]), float(season[1])
        check(lib().lf_snow_frost_members_device(self.device, C.byref(self.args), self.members, self.stride, self.fstride,
                                                 self.forcing_member_stride()))


class SnowFrostDevice(SnowFrostEnsemble):
    """Snow and frost of one run, device-resident: SnowFrostEnsemble with one member, whose vectors get() returns without
    the member axis"""

    def __init__(self, meteo, device=0):
        super().__init__(meteo, 1, device, 0)

    def get(self, name):
        out = super().get(name)
        return out if name in self._static else out[0]
