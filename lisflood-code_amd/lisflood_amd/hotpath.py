"""Device-resident hot path of one LISFLOOD model step (Lisflood_dynamic.py:114-229, the stages SURVEY.md section 8
covers), with every vector kept in HBM between steps:

    soilloop.dynamic_canopy -> soilloop.dynamic_soil -> opensealed / soil.dynamic_perpixel / groundwater
    -> surface_routing.dynamic (3 routers on LddToChan) -> NoRoutSteps x routing.dynamic (1-2 routers, fused
    wavefront) -> ChanQAvg

Per step only the meteorological forcing (Rain, SnowMelt, EWRef, ETRef, ESRef -- five [N] vectors) crosses PCIe.
With meteo= the step begins one module earlier: snow.dynamic and frost.dynamic (snow_frost.py, lf_snow_frost_members_device)
make Rain, SnowMelt and isFrozenSoil on the device from Precipitation and Tavg, which take the two vectors' place in the
forcing, and the snow pack of three elevation zones and the frost index are state like the soil's.
The stages are exactly the kernels the module classes (`soilloop`, `pixel_aggregates`, `surface_routing`,
`routing`) call -- those stage their `var` arrays through the host on every call, this class wires the same
device buffers from one stage to the next.  Channel vectors live in the channel router's engine order; the one
vector that crosses from the surface graph to the channel graph (ToChanM3RunoffDt) is permuted on the device.
"""
import ctypes as C
import os
import types

import numpy as np

from . import output
from . import pixel_aggregates as PA
from . import routing as RT
from . import snow_frost as SF
from . import soilloop as SL
from . import surface_routing as SR
from . import zonal as ZN
from ._lib import DeviceArray, PinnedArray, check, f64, lib, ptr, timer_start, timer_stop, u8
from .channel_domain import _structures_on_subdomain, channel_domain, inert_pixels  # noqa: F401 (inert_pixels: read from here)
from .kinematic_wave_parallel import Graph, kinematicWave

FORCING = ("Rain", "SnowMelt", "EWRef", "ETRef", "ESRef")
# with meteo=: the snow and frost kernel makes Rain, SnowMelt and isFrozenSoil on the device from these
METEO_FORCING = SF.METEO + ("EWRef", "ETRef", "ESRef")
_CHANNEL_NAMES = set(RT._STATIC + RT._STATE + RT._OUT)
# HotPathEnsemble.track_begin: the derived names of a tracked name's accumulators, and what lies between the int32 rows
_TRACK_F64, _TRACK_I32 = ("peak", "sum", "period_mean"), ("peak_step", "first_above", "steps_above")
TRACK_GAP_I32 = -7


# Maps of the land-surface stages that nothing else on the hot path reads (HotPathDevice(report=...)): the soil kernel's
# diagnostics (soilloop.py:330-336), the per-pixel diagnostics of opensealed / soil.dynamic_perpixel / groundwater and the
# cumulative sums of the mass-balance report.  Everything else -- states, `dis`, what a later stage reads -- always exists.
OPTIONAL_MAPS = ("Theta1a Theta1b Theta2 Sat1a Sat1b Sat1 Sat2 "
                 "RainSnowmelt EWaterAct InterSealed TASealed TaInterceptionAll TaPixel ESActPixel PrefFlowPixel InfiltrationPixel "
                 "Theta ThetaAll SeepTopToSubPixelA SeepTopToSubPixelB SeepSubToGWPixel Theta1aPixel Theta1bPixel Theta2Pixel "
                 "LZOutflow GwPercUZLZPixel GwLossLZ LZAvInflow LZInflowCUM TaInterceptionCUM TaCUM ESActCUM GwLossCUM").split()
# [3,N] inputs of the per-pixel aggregates -> the optional outputs that read them (none reported: the input is not streamed)
PA_READERS = dict(TaInterception=("TaInterceptionAll", "TaInterceptionCUM"), Ta=("TaPixel", "TaCUM"), ESAct=("ESActPixel", "ESActCUM"),
                  PrefFlow=("PrefFlowPixel",), Infiltration=("InfiltrationPixel",), SeepTopToSubA=("SeepTopToSubPixelA",),
                  SeepTopToSubB=("SeepTopToSubPixelB",), SeepSubToGW=("SeepSubToGWPixel",), Theta1a=("Theta1aPixel",),
                  Theta1b=("Theta1bPixel",), Theta2=("Theta2Pixel",), W1a=("Theta", "ThetaAll"), W1b=("Theta", "ThetaAll"),
                  W2=("Theta", "ThetaAll"), SoilDepthTotal=("Theta", "ThetaAll"))


class PendingRasters:
    """Report maps on their way to the host (summary_rasters() / rasters()): the pack kernel and the asynchronous copy into
    page-locked memory are enqueued, nothing has been waited for.  wait() blocks until the copy has landed (an event, not
    the device) and returns name -> array: views of the page-locked buffers of the request's buffer set, valid until that set
    is used again -- the request after the next one.  From then on wait() raises instead of handing out overwritten memory."""

    def __init__(self, owner, buffer_set, serial, views):
        self._owner, self.buffer_set, self.serial, self._views = owner, buffer_set, serial, views

    def wait(self):
        o = self._owner
        if o._report_serial[self.buffer_set] != self.serial:
            raise RuntimeError("stale PendingRasters handle: request %d used buffer set %d, which a later request has taken "
                               "over (or free() has released); copy what wait() returns before the request after the next"
                               % (self.serial, self.buffer_set))
        check(lib().lf_download_wait(o.device, self.buffer_set))
        return dict(self._views)


class _HotPath:
    """What HotPathDevice and HotPathEnsemble are both made of: the `report` set, the three overland routers and the order
    of the non-channel vectors, the channel domain (channel_domain.channel_domain) with the channel router on it -- or,
    with structures=, the resident routing module (_routing_module) --, the engine-order index vectors, the scalar half of
    the argument blocks, and the host side of set_lai / set_inflow / state files / free().  The constructors call the
    pieces in their own order, which is the order of their device allocations."""

    # everything a stage reads back from the previous step (the reference writes its state maps as end / state files,
    # default_options.py:131-160): the in/out vectors of the canopy and soil kernels, the accumulators of the per-pixel
    # aggregates, the overland and channel router states
    STATE = tuple(dict.fromkeys(SL._CANOPY_IO + list(SL._V_IO) + PA._STATE + SR._STATE +
                                ["OFM3Direct", "OFM3Other", "OFM3Forest"] + RT._STATE + list(SF.STATE)))

    def _begin(self, scalars, land_mask, split, device, overlap_channel, report, meteo=None, members=None):
        self.device, self.split = device, bool(split)
        # overlap_channel: the channel wavefront of a step on a second HIP stream, beside the canopy / soil / overland kernels
        # of the step after it (same kernels, same results; False: one stream, as rounds 1-3).  Read at every call.
        self.overlap_channel = bool(overlap_channel)
        # report: which of the OPTIONAL maps (OPTIONAL_MAPS: diagnostics and cumulative sums nothing else on the hot
        # path reads) are wanted.  None: all of them, as the reference computes them every step; an iterable of names: only
        # those -- the others get no device vector, are not computed, and the [3,N] vectors only they read are not streamed
        # (the reference writes the maps its rep* options name; what is not reported need not exist).  `dis`, the state
        # maps and everything another stage reads are always there.
        self.report = None if report is None else set(report)
        if self.report is not None and not self.report <= set(OPTIONAL_MAPS):
            raise ValueError("report: not optional maps: %s" % sorted(self.report - set(OPTIONAL_MAPS)))
        self.sc = dict(scalars)
        land_mask = np.asarray(land_mask, bool)
        self.N = int(land_mask.sum())
        self.rmod, self._qin_old, self._pinned, self.steps_done = None, None, [], 0
        # rasters() / summary_rasters(): the mask the rasters are laid out on, the index tables of the pack kernel (made on
        # first use), two buffer sets (device staging, page-locked host image) and which request holds each of them
        self.land_mask = land_mask
        self._report_tables, self._report_sets, self._report_serial, self._report_count = {}, [None, None], [0, 0], 0
        # meteo: None -- the forcing is Rain, SnowMelt, EWRef, ETRef, ESRef and isFrozenSoil stays what `values` says -- or the
        # dict snow_frost.check_meteo describes: the forcing is Precipitation, Tavg, EWRef, ETRef, ESRef, and the snow and
        # frost kernel (lf_snow_frost_members_device) is the first launch of every step
        self.meteo = None if meteo is None else SF.check_meteo(meteo, self.N, members)
        self.forcing_names = FORCING if meteo is None else METEO_FORCING
        return land_mask

    def _meteo_values(self):
        """what `meteo` adds to the per-pixel arrays of the constructor (pixel order): the statics and the two states"""
        return {k: self.meteo[k] for k in SF.STATICS + SF.STATE}

    def _meteo_block(self, pointer_of):
        """the argument block of the snow and frost kernel: pointer_of(name) -> address of (member 0's row of) a vector"""
        a = SF.fill_scalars(SF._SnowFrostArgs(), self.meteo, self.N)
        for k in SF._POINTERS:
            if k != "Snow" or self.meteo["Snow"]:
                setattr(a, k, pointer_of(k))
        return a

    def _season(self, season):
        """season= of step() checked: required with meteo=, refused without; sets the two scalars of the block"""
        if self.meteo is None:
            if season is not None:
                raise ValueError("season= without meteo=: this object takes Rain and SnowMelt as forcing")
            return
        if season is None or np.shape(season) != (2,):
            raise ValueError("step(..., season=(SnowSeasonTerm, SummerSeason)) is required with meteo= "
                             "(snow_frost.season_terms)")
        self.snow_frost.SnowSeasonTerm, self.snow_frost.SummerSeason = float(season[0]), float(season[1])

    def _check_forcing(self, forcing):
        """the names of a forcing dict against what an object with meteo= takes"""
        if self.meteo is None:
            return
        made = [k for k in ("Rain", "SnowMelt") if k in forcing]
        if made:
            raise ValueError("%s in the forcing of an object with meteo=: the snow and frost kernel makes them from "
                             "Precipitation and Tavg" % " and ".join(made))
        missing = [k for k in self.forcing_names if k not in forcing]
        if missing:
            raise ValueError("forcing lacks %s" % ", ".join(missing))

    def _check_state_file(self, files):
        missing = [k for k in SF.STATE if self.meteo is not None and k not in files]
        if missing:
            raise ValueError("state file without %s: it was written by an object without meteo=" % " and ".join(missing))

    def _kept(self):
        """the optional maps that exist in this object: the reported ones plus what they are made of (the per-pixel Theta
        averages read the soil kernel's Theta1a / Theta1b / Theta2)"""
        if self.report is None:
            return set(OPTIONAL_MAPS)
        keep = set(self.report)
        for pix, col in (("Theta1aPixel", "Theta1a"), ("Theta1bPixel", "Theta1b"), ("Theta2Pixel", "Theta2"),
                         ("LZAvInflow", "LZInflowCUM")):
            if pix in keep:
                keep.add(col)
        return keep

    def _wanted(self, names):
        kept = self._kept()
        return [k for k in names if k not in OPTIONAL_MAPS or k in kept]

    def _overland(self, values, ldd_to_chan, land_mask, surface_order=True):
        """the three overland routers on one graph, and position -> pixel of that graph's sweep order (None: the non-channel
        vectors stay in pixel order)"""
        sc = self.sc
        g_surf = Graph(ldd_to_chan, land_mask)
        alpha_of = np.asarray(values["OFAlpha"], float)
        mk = lambda row: kinematicWave(None, None, alpha_of[row], sc["Beta"], sc["PixelLength"], sc["DtSec"],
                                       device=self.device, graph=g_surf)
        self.r_other, self.r_forest, self.r_direct = mk(0), mk(1), mk(2)
        self.pixel_of_position = g_surf.layout()[0].astype(np.int64) if surface_order else None

    def _channel(self, values, ldd_kinematic, land_mask, structures, compact):
        """The channel domain -- all land pixels, or only the ones whose routing sub-step is not the identity -- and the
        channel router on it: `river` alone, or with structures the routing module `rmod` that owns it.
        -> (v, structures): the namespace of the channel values and scalars, and the structures, both on the domain."""
        N, sc = self.N, self.sc
        ldd_kinematic = np.asarray(ldd_kinematic, np.float64)
        self.ids, chan_mask = channel_domain(values, ldd_kinematic, land_mask, self.split, structures, compact)
        Nk = self.Nk = self.ids.size                          # ids: channel-domain pixel -> land pixel
        self._outside = np.setdiff1d(np.arange(N), self.ids)
        if Nk < N and structures is not None:
            structures = _structures_on_subdomain(structures, self.ids, N)
        v = types.SimpleNamespace(IsChannelKinematic=np.zeros(Nk, bool))     # (not given: no pixel is a channel pixel)
        for k in set(RT._STATIC + RT._STATE) & set(values):
            setattr(v, k, np.array(np.broadcast_to(np.asarray(values[k]), (N,))[self.ids], copy=True))
        v.Beta, v.InvBeta, v.DtRouting, v.InvDtRouting = sc["Beta"], 1 / sc["Beta"], sc["DtRouting"], 1 / sc["DtRouting"]
        v.DtSec, v.NoRoutSteps, v.InvNoRoutSteps = sc["DtSec"], int(sc["NoRoutSteps"]), 1 / sc["NoRoutSteps"]
        if structures is None:
            self.river = kinematicWave(ldd_kinematic[self.ids], chan_mask, v.ChannelAlpha, sc["Beta"], v.ChanLength,
                                       sc["DtRouting"], alpha_floodplains=v.ChannelAlpha2 if self.split else None,
                                       device=self.device)
        else:
            self.rmod = self._routing_module(v, structures, ldd_kinematic[self.ids], chan_mask)
            self.river = self.rmod.river_router
        return v, structures

    def _routing_module(self, v, structures, ldd_kinematic, chan_mask):
        """the channel part as a resident, engine-order routing module with its structures attached"""
        v.ToChanM3RunoffDt = np.zeros(self.Nk)
        for k, a in structures.items():
            setattr(v, k, a)
        opts = dict(SplitRouting=self.split, InitLisflood=False, simulateLakes="LakeIndex" in structures,
                    simulateReservoirs="ReservoirIndex" in structures, inflow="QInM3Old" in structures,
                    TransLoss="UpTrans" in structures)
        m = RT.routing(v, options=opts, device=self.device, engine_order=True)
        m.attach_router(ldd_kinematic, chan_mask)
        m.attach_structures()
        m.begin_step()                              # uploads the channel state once; it stays resident
        m._structures_substep(0, launch=False)      # site state from the dense maps, once
        m._args.split = 1 if self.split else 0
        return m

    def _engine_order(self):
        self.perm = self.river.graph.layout()[0].astype(np.int64)        # engine position -> channel-domain pixel
        self.gpix = src = self.ids[self.perm]                             # engine position -> land pixel
        if self.pixel_of_position is not None:
            inv = np.empty(self.N, np.int64)
            inv[self.pixel_of_position] = np.arange(self.N)
            src = inv[self.gpix]                                          # where a channel cell's land pixel sits in those vectors
        self._gidx = DeviceArray.from_host(src.astype(np.int32), self.device)

    def _finish_args(self, p, f):
        """what the blocks of the per-pixel aggregates and of the overland step hold beside pointers to vectors"""
        sc, N, kept = self.sc, self.N, self._kept()
        if self.report is not None:        # a [3,N] input that only unreported maps read is not handed to the kernel
            for src, outs in PA_READERS.items():
                if not any(o in kept for o in outs):
                    setattr(p, src, None)
        p.InvDtDay, p.N = sc["InvDtDay"], N
        f.Beta, f.MMtoM3, f.M3toMM = sc["Beta"], sc["MMtoM3"], sc["M3toMM"]
        f.PixelLength, f.InvPixelLength = sc["PixelLength"], 1 / sc["PixelLength"]
        f.DtSec, f.InvDtSec, f.InvNoRoutSteps, f.N = sc["DtSec"], 1 / sc["DtSec"], 1 / sc["NoRoutSteps"], N

    def _ordered(self, a):
        """a per-pixel array ([N] or [..., N], pixel order) in the order the non-channel device vectors are kept in"""
        a = np.asarray(a)
        if self.pixel_of_position is None or a.ndim == 0 or a.shape[-1] != self.N:
            return a
        return np.ascontiguousarray(a[..., self.pixel_of_position])

    def _pixel_order(self, a):
        """inverse of _ordered"""
        if self.pixel_of_position is None or a.ndim == 0 or a.shape[-1] != self.N:
            return a
        out = np.empty_like(a)
        out[..., self.pixel_of_position] = a
        return out

    def _check_inside(self, a, message):
        """ValueError(message) if `a` ([..., N], pixel order) is not zero on the pixels left out of the channel domain"""
        if self._outside.size and np.any(a[..., self._outside] != 0):
            raise ValueError(message)

    def _side_begin(self, side=True):
        """From here to _side_end(what this returns), in a try / finally, the calls go to the channel loop's stream (the side
        stream, behind the loop of the step before) -- if overlap_channel says so now, else they stay where they are."""
        side = side and self.overlap_channel
        if side:
            check(lib().lf_side_stream_begin(self.device))
        return side

    def _side_end(self, side):
        if side:
            check(lib().lf_side_stream_end(self.device))

    def set_lai(self, LAI, LAITerm):
        """The prescribed leaf area index of the coming steps: what leafarea.dynamic sets once per ten-day interval
        (leafarea.py:80-91: LAI of the interval, LAITerm = exp(-kgb * LAI)), [3, N] each, pixel order (an ensemble's
        members share the two vectors).  Waits for the step in flight (its canopy kernel reads the vectors)."""
        check(lib().lf_device_synchronize(self.device))
        for k, a in (("LAI", LAI), ("LAITerm", LAITerm)):
            a = np.asarray(a, np.float64)
            if a.shape != (3, self.N):
                raise ValueError("%s must be [3, %d]" % (k, self.N))
            self._lai_vectors()[k].upload(f64(self._ordered(a)))

    def _inflow(self, QInM3):
        """The host half of set_inflow: QInM3 in pixel order, [N] -- for an ensemble every member's, or [members, N] --
        -> (q, delta) on the channel domain, shaped like _qin_old: the volumes, and QDelta = (QInM3 - QInM3Old) *
        InvNoRoutSteps (inflow.py:108-125)."""
        if self._qin_old is None:
            raise RuntimeError("inflow hydrographs need structures= with QInM3Old / QDelta (the `inflow` option)")
        q, lead = np.asarray(QInM3, np.float64), self._qin_old.shape[:-1]
        if lead and q.shape not in ((self.N,), lead + (self.N,)):
            raise ValueError("QInM3 must be [%d] or [%d, %d]" % (self.N, lead[0], self.N))
        q = np.broadcast_to(q, lead + (self.N,))
        self._check_inside(q, "inflow at a pixel this object left out of the channel domain; flag the inflow pixels in "
                              "structures['InflowPoints'] or build it with compact=False")
        q = np.ascontiguousarray(q[..., self.ids])
        return q, (q - self._qin_old) * self.rmod.var.InvNoRoutSteps

    def _pinned_set(self, shape, dtype):
        """a forcing dict of page-locked host arrays that belong to this object (freed by free())"""
        bufs = {k: PinnedArray(shape, dtype, self.device) for k in self.forcing_names}
        self._pinned.append(bufs)
        return {k: b.a for k, b in bufs.items()}

    def upload_wait(self, buffer_set=None):
        """Block until the forcing uploads started by prefetch() / step() have left the host arrays (lf_upload_wait):
        after it the arrays of pinned_forcing() may be refilled in place.  buffer_set: 0 / 1, default both."""
        for b in ((0, 1) if buffer_set is None else (int(buffer_set),)):
            check(lib().lf_upload_wait(self.device, b))

    def chan_q_avg(self):
        """ChanQAvg = sumDisDay / NoRoutSteps (Lisflood_dynamic.py:209): the `dis` output of the reference ([members, N]
        of an ensemble)."""
        return self.download("sumDisDay") / self.sc["NoRoutSteps"]

    # ---- report maps as [H, W] rasters, packed on the device and downloaded beside the next step --------------------------
    _PACK_KIND = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.int32): 2}      # LF_PACK_F64 / _F32 / _I32
    _PACK_MAX = 16                                                                              # sources of one launch

    def _raster_table(self, which):
        """device int32 [H * W] (output.raster_index), made once: where a raster cell's value sits in "land" rows (the order
        of pixel_of_position), in "channel" rows (engine order of the channel router; a land pixel outside the channel
        domain: -2, zero) or in a map in "pixel" order (the product maps)"""
        d = self._report_tables.get(which)
        if d is None:
            row = None
            if which == "channel":
                row = np.full(self.N, -1, np.int64)
                row[self.gpix] = np.arange(self.Nk)
            elif which == "land" and self.pixel_of_position is not None:
                row = np.empty(self.N, np.int64)
                row[self.pixel_of_position] = np.arange(self.N)
            d = self._report_tables[which] = DeviceArray.from_host(output.raster_index(self.land_mask, row), self.device)
        return d

    def _report_buffers(self, b, nbytes):
        """(device staging, page-locked image) of set b, at least nbytes long: grow-only, replaced only once the set's last
        copy has landed (the caller has waited)"""
        st = self._report_sets[b]
        if st is None or st[0].nbytes < nbytes:
            if st is not None:
                st[0].free(); st[1].free()
            st = self._report_sets[b] = (DeviceArray(nbytes, np.uint8, self.device), PinnedArray(nbytes, np.uint8, self.device))
        return st

    def _report_rasters(self, groups, dtype, fill, side, produce=None):
        """groups: [(table name, [(key, device vector, rows, stride, divisor, stack)])] -- every source of a group is packed
        in one launch through the group's table, fp64 sources as `dtype`, int32 sources as int32; a key comes out as [H, W],
        or as [rows, H, W] if `stack` (rows is 1 without it; a tuple: the leading shape the rows are split into).  side: the
        work may go to the channel loop's stream (nothing but that stream writes the sources).  produce(): enqueues what makes the sources, on the stream the pack follows.  -> PendingRasters"""
        L, dev = lib(), self.device
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("dtype must be float32 or float64 (got %s)" % dtype)
        shape, cells = self.land_mask.shape, self.land_mask.size
        keys = [s[0] for _, sources in groups for s in sources]
        if len(set(keys)) != len(keys):
            raise ValueError("a name is given twice: %s" % keys)
        if not 1 <= len(keys) <= self._PACK_MAX:
            raise ValueError("1 to %d maps per call (got %d)" % (self._PACK_MAX, len(keys)))
        plan, total = [], 0
        for table, sources in groups:
            calls = []
            for key, src, rows, stride, divisor, stack in sources:
                dt = np.dtype(np.int32) if src.dtype == np.int32 else dtype
                calls.append(types.SimpleNamespace(key=key, src=src, rows=rows, stride=stride, divisor=divisor, stack=stack,
                                                   dtype=dt, at=total, nbytes=rows * cells * dt.itemsize))
                total += -(-calls[-1].nbytes // 256) * 256                     # (every map starts on a 256-byte boundary)
            if calls:
                plan.append((self._raster_table(table), calls))
        b = self._report_count % 2
        self._report_count += 1
        # the set is used again: whoever holds its buffers is stale from here on, and its last copy has landed before the
        # buffers are written (or replaced)
        check(L.lf_download_wait(dev, b))
        self._report_serial[b] = self._report_count
        stage, pin = self._report_buffers(b, max(total, 256))
        views = {}
        side = self._side_begin(side)
        try:
            if not side:
                check(L.lf_side_stream_join(dev))
            if produce is not None:
                produce()
            check(L.lf_report_acquire(dev, b))
            for table, calls in plan:
                n = len(calls)
                check(L.lf_pack_rasters_device(
                    dev, n, (C.c_void_p * n)(*[c.src.ptr.value for c in calls]),
                    (C.c_void_p * n)(*[stage.ptr.value + c.at for c in calls]), (C.c_int32 * n)(*[c.rows for c in calls]),
                    (C.c_int64 * n)(*[c.stride for c in calls]), (C.c_int32 * n)(*[self._PACK_KIND[c.src.dtype] for c in calls]),
                    (C.c_int32 * n)(*[self._PACK_KIND[c.dtype] for c in calls]), (C.c_double * n)(*[c.divisor for c in calls]),
                    table.ptr, cells, float(fill)))
                for c in calls:
                    lead = c.stack if isinstance(c.stack, tuple) else ((c.rows,) if c.stack else ())
                    views[c.key] = pin.a[c.at:c.at + c.nbytes].view(c.dtype).reshape(lead + shape)
            check(L.lf_download_begin(dev, b))
            try:
                check(L.lf_download_copy(dev, pin.ptr, stage.ptr, total))
            finally:
                check(L.lf_download_end(dev, b))
        finally:
            self._side_end(side)
        return PendingRasters(self, b, self._report_count, views)

    def _report_free(self):
        for b in (0, 1):
            check(lib().lf_download_wait(self.device, b))
            if self._report_sets[b] is not None:
                self._report_sets[b][0].free(); self._report_sets[b][1].free()
        for d in self._report_tables.values():
            d.free()
        self._report_tables, self._report_sets, self._report_serial = {}, [None, None], [-1, -1]

    def _free_shared(self, arrays):
        """`arrays`: the device arrays of the class, which may include the routing module's (each is freed once); then the
        four routers, and -- once no upload can still be reading them -- the page-locked buffers"""
        self._report_free()
        arrays = {id(a): a for a in arrays}
        if self.rmod is not None:
            arrays.update({id(a): a for a in list(self.rmod._st["dev"].values()) + list(self.rmod._dev.values())})
        for a in arrays.values():
            a.free()
        for r in (self.r_other, self.r_forest, self.r_direct, self.river):
            r.close()
        check(lib().lf_device_synchronize(self.device))
        for bufs in self._pinned:
            for b in bufs.values():
                b.free()
        self._pinned = []


class HotPathDevice(_HotPath):
    def __init__(self, values, scalars, land_mask, ldd_to_chan, ldd_kinematic, split=True, device=0, structures=None,
                 compact=True, overlap_channel=True, surface_order=True, land_fused=None, report=None, meteo=None):
        """values: name -> host array in pixel order ([N], [3,N]) for every vector of the stages (reference
        attribute names); scalars: Beta, DtSec, DtRouting, NoRoutSteps, DtDay, PixelLength, MMtoM3, M3toMM,
        LeafDrainageK, AvWaterThreshold, CourantCrit, DrainedFraction, InvDtDay.  ldd_to_chan / ldd_kinematic:
        compressed LDD codes of the overland and the channel graph.
        structures: optional dict of the reference's lake / reservoir / inflow / transmission attributes (the names
        routing.attach_structures reads, incl. `downstruct` of the uncut LDD); ldd_kinematic is then the CUT LDD
        (structures.py:44-61) and the sub-step loop runs with the structures inside the wavefront.
        compact: leave inert pixels out of the channel router's domain (see inert_pixels): on real domains most land
        pixels are not channel pixels, and the channel wavefront then touches only the ones that are."""
        # overlap_channel, report, meteo: see _HotPath._begin
        land_mask = self._begin(scalars, land_mask, split, device, overlap_channel, report, meteo)
        N, sc = self.N, self.sc
        if self.meteo is not None:
            values = dict(values, **self._meteo_values())
            values.setdefault("isFrozenSoil", np.zeros(N, bool))
        # surface_order: every per-pixel vector that is not a channel vector lives in the sweep order of the OVERLAND
        # routers' graph (the canopy / soil / aggregate kernels are element-wise and do not care; the three overland routers
        # then stream their vectors instead of going through the position -> pixel table: lf_surface_step_ordered).
        # Vectors come in and go out in pixel order all the same (constructor, step(), download(), state files); a caller
        # whose forcing is already in that order (`pixel_of_position`) says step(..., ordered=True) and saves the gather.
        # the ten derived soil parameter arrays recomputed instead of read where they are what soil.py:180-228 makes them
        self.soil_derived = SL.derived_parameters_hold(values)
        # land_fused: canopy + ESMax + soil columns as ONE pass over the columns (lf_land_columns_device; the three prescribed
        # fractions map to their own land-use rows, which is what it needs).  None: on, unless LF_LAND_FUSED=0 (A/B switch);
        # False: the three separate launches of rounds 1-5 -- same bits either way
        self.land_fused = (os.environ.get("LF_LAND_FUSED", "1") != "0") if land_fused is None else bool(land_fused)
        # ---- routers, channel domain ------------------------------------------------------------------
        self._overland(values, ldd_to_chan, land_mask, surface_order)
        v, structures = self._channel(values, ldd_kinematic, land_mask, structures, compact)
        Nk = self.Nk
        if structures is not None and "QInM3Old" in structures:      # inflow hydrographs: QInM3 of the previous model step
            self._qin_old = f64(np.broadcast_to(structures["QInM3Old"], (Nk,))).copy()
        self._engine_order()
        chan_names = set(RT._STATIC + RT._STATE)
        self.d = {}
        # ---- device vectors ------------------------------------------------------------------------
        if self.rmod is None:       # the channel vectors, in the engine order of the river router, and their argument block
            vec = RT.SubstepVectors(RT.substep_host_vectors(v, Nk, self.perm), Nk, sc["Beta"], 1 / sc["DtRouting"],
                                    sc["DtSec"], self.split, True, device, order=RT._STATIC + RT._STATE)
        else:       # self.d and self.rout alias the routing module's own vectors and block (free() frees each array once)
            vec = self.rmod._vectors
        self.d.update(vec.dev)
        bool_names = SL._BOOL | {"IsChannel", "IsChannelKinematic"}
        for k, a in values.items():
            a = np.asarray(a)
            if self.report is not None and k in OPTIONAL_MAPS and k not in self._kept():
                continue                              # an optional map nobody asked for: no device vector at all
            if k in chan_names:                       # channel vectors: made above
                continue
            if self.pixel_of_position is not None and a.ndim >= 1 and a.shape[-1] == N and k not in bool_names:
                self.d[k] = self._upload_ordered(f64(a))      # permuted on the device (a host gather of ~100 fields is slow)
                continue
            a = self._ordered(a)
            self.d[k] = DeviceArray.from_host(u8(a) if k in bool_names else f64(a), device)
        if getattr(self, "_perm_tmp", None) is not None:
            self._perm_tmp.free(); self._perm_idx.free()
            self._perm_tmp = self._perm_idx = None

        def zeros(name, shape):
            if name not in self.d:
                self.d[name] = DeviceArray(shape, np.float64, device).zero()
            return self.d[name]
        # forcing: two buffer sets, so that the upload of the next step's vectors (second HIP stream) overlaps the
        # kernels of the current step -- see prefetch()
        self.force = [{k: DeviceArray(N, np.float64, device).zero() for k in self.forcing_names} for _ in range(2)]
        self._prefetched, self._keep = [None, None], [None, None]
        for k in self.forcing_names:
            self.d[k] = self.force[0][k]
        # ---- argument blocks (pointers into self.d) -----------------------------------------------------
        def fill(args, names, shape_of):
            for k in names:
                setattr(args, k, zeros(k, shape_of(k)).ptr.value)
        vn = lambda k: (3, N)
        n1 = lambda k: N
        a = self.canopy = SL._CanopyArgs()
        fill(a, SL._CANOPY_IO + SL._CANOPY_V_IN + SL._CANOPY_L_IN, vn)
        fill(a, SL._CANOPY_N_IN, n1)
        self._idx = np.arange(3, dtype=np.int64)
        a.index_landuse = self._idx.ctypes.data
        a.LeafDrainageK, a.DtDay, a.InvDtDay = sc["LeafDrainageK"], sc["DtDay"], sc["InvDtDay"]
        a.V, a.L, a.N = 3, 3, N
        zeros("LAITerm", (3, N)); zeros("ESMax", (3, N))
        s = self.soil = SL._SoilArgs()
        wanted = self._wanted
        fill(s, wanted(SL._L_FIELDS + SL._V_IN + SL._V_IO), vn)
        fill(s, SL._N_FIELDS, n1)
        self._irr = np.array([0, 0, 1], np.uint8)
        self._pad = np.zeros(3, np.uint8)
        s.index_landuse_all, s.is_irrigated, s.is_paddy_irrig = (self._idx.ctypes.data, self._irr.ctypes.data,
                                                                 self._pad.ctypes.data)
        s.DtDay, s.AvWaterThreshold, s.CourantCrit, s.DrainedFraction = (sc["DtDay"], sc["AvWaterThreshold"],
                                                                         sc["CourantCrit"], sc["DrainedFraction"])
        s.V, s.L, s.N = 3, 3, N
        p = self.pixel = PA._PixelArgs()
        fill(p, wanted(PA._V_IN + ["Theta"]), vn)
        fill(p, wanted(PA._N_IN + PA._STATE + PA._OUT), n1)
        f = self.surface = SR._SurfaceArgs()
        fill(f, SR._V_IN + ["SurfaceRunSoil", "scratch"], vn)
        fill(f, SR._N_IN + SR._STATE + SR._OUT, n1)
        self._finish_args(p, f)
        if self.rmod is None:       # outputs, scratch and sideflow come last, where they always were allocated
            vec.allocate(["SideflowChanM3"] + RT._OUT + ["scratch0", "scratch1"])
            self.d.update(vec.dev)
        self.rout = vec.args
        if self.meteo is not None:  # Rain and SnowMelt exist once (made above, by the blocks that read them), written by the kernel
            for k in ["SnowCover"] + (["Snow"] if self.meteo["Snow"] else []):
                zeros(k, N)
            self.snow_frost = self._meteo_block(lambda k: self.d[k].ptr.value)

    def _lai_vectors(self):
        return self.d

    def _upload_ordered(self, a):
        """fp64 [N] or [R, N] host array in pixel order -> device array in the order of pixel_of_position: every row is
        uploaded as it is and gathered on the device (lf_gather_device)"""
        L, dev, N = lib(), self.device, self.N
        if getattr(self, "_perm_tmp", None) is None:
            self._perm_tmp = DeviceArray(N, np.float64, dev)
            self._perm_idx = DeviceArray.from_host(self.pixel_of_position.astype(np.int32), dev)
        dst = DeviceArray(a.shape, np.float64, dev)
        rows = a.reshape(-1, N)
        for r in range(rows.shape[0]):
            self._perm_tmp.upload(np.ascontiguousarray(rows[r]))
            check(L.lf_gather_device(dev, N, self._perm_idx.ptr, self._perm_tmp.ptr, dst.ptr.value + r * N * 8))
        return dst

    def _upload(self, b, forcing, ordered=False):
        """float32 vectors (meteo as the netCDF files store it) go up as float32 and are widened on the device -- exactly
        what widening them on the host first would give, at half the PCIe traffic"""
        L, dev = lib(), self.device
        as_is = lambda a: np.ascontiguousarray(a) if np.asarray(a).dtype == np.float32 else f64(a)
        self._check_forcing(forcing)
        host = [as_is(forcing[k]) if ordered else as_is(self._ordered(forcing[k])) for k in self.forcing_names]
        check(L.lf_upload_begin(dev, b))
        for k, a in zip(self.forcing_names, host):
            if a.size != self.N:
                raise ValueError("forcing vector %s must have %d entries" % (k, self.N))
            if a.dtype == np.float32:
                check(L.lf_upload_copy_f32(dev, self.force[b][k].ptr, a.ctypes.data_as(C.c_void_p), a.size))
                continue
            check(L.lf_upload_copy(dev, self.force[b][k].ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))
        check(L.lf_upload_end(dev, b))
        self._keep[b] = host                 # the host vectors stay alive until the set is uploaded again

    def pinned_forcing(self, dtype=np.float64):
        """A forcing dict (Rain, SnowMelt, EWRef, ETRef, ESRef) of [N] arrays in page-locked host memory, to be filled in
        place (e.g. by the netCDF reader) and passed to prefetch() / step(): their upload is an asynchronous DMA at the
        PCIe rate instead of a staged, blocking copy.  The arrays belong to this object (freed by free()).
        The DMA reads the arrays AFTER prefetch() / step() has returned: call upload_wait() before writing the next
        time step into a set that was handed over (or alternate between two pinned sets and wait before reuse)."""
        return self._pinned_set(self.N, dtype)

    def prefetch(self, forcing, ordered=False):
        """Start uploading the forcing of the NEXT step() call now: the copies run on a second stream while the kernels
        of the step just enqueued are still executing.  Pass the same dict object to the next step().
        ordered: the vectors are already in the order of `pixel_of_position` (e.g. compressed from the netCDF raster
        with the composed index) -- otherwise they are in pixel order and are permuted on the host first."""
        b = self.steps_done % 2
        self._upload(b, forcing, ordered)
        self._prefetched[b] = forcing

    def _use_set(self, b):
        for k in self.forcing_names:
            self.d[k] = self.force[b][k]
            for st in (self.canopy, self.soil, self.pixel, self.surface) + (() if self.meteo is None else (self.snow_frost,)):
                if hasattr(type(st), k):
                    setattr(st, k, self.force[b][k].ptr.value)

    def set_inflow(self, QInM3):
        """inflow.dynamic + dynamic_init (inflow.py:108-125) for the coming step: QInM3 [N] is the hydrograph volume of
        the model step [m3]; QDelta = (QInM3 - QInM3Old) * InvNoRoutSteps goes to the device next to QInM3Old, and
        QInM3 becomes QInM3Old once the step is enqueued (Lisflood_dynamic.py:185)."""
        q, delta = self._inflow(QInM3)
        m, dev = self.rmod, self.rmod._st["dev"]
        # Only the channel wavefront reads the two vectors: they go up on ITS stream (the side stream when the wavefront
        # runs there), behind the wavefront of the step before and ahead of the next one, without a host wait and without
        # making the main stream wait for the side stream (lf_memcpy_h2d would do both)
        side = self._side_begin()
        try:
            dev["QInM3Old"].upload(f64(m._up(self._qin_old)), staged=True)
            dev["QDelta"].upload(f64(m._up(delta)), staged=True)
        finally:
            self._side_end(side)
        self._qin_old = q

    def step(self, forcing, time_since_start=None, QInM3=None, ordered=False, season=None):
        """With meteo=: forcing holds Precipitation, Tavg, EWRef, ETRef, ESRef, and season=(SnowSeasonTerm, SummerSeason)
        of the step is required (snow_frost.season_terms); step(None, season=...) takes the meteo its buffer set holds, as
        without meteo=, and still advances the snow pack and the frost index."""
        self._season(season)
        if QInM3 is not None:
            self.set_inflow(QInM3)
        self._step(forcing, time_since_start, ordered)

    def _step(self, forcing, time_since_start, ordered, stage_ms=None):
        L, dev = lib(), self.device
        b = self.steps_done % 2
        if forcing is None:          # the vectors this buffer set already holds (uploaded for an earlier step): no PCIe traffic
            if self._keep[b] is None:
                raise ValueError("step(None): buffer set %d has never been uploaded" % b)
        elif self._prefetched[b] is not forcing:
            self._upload(b, forcing, ordered)
        self._prefetched[b] = None
        check(L.lf_compute_acquire(dev, b))
        self._use_set(b)
        try:
            self._enqueue(time_since_start, stage_ms)
        finally:
            check(L.lf_compute_release(dev, b))

    def _enqueue(self, time_since_start, stage_ms=None):
        """stage_ms: a dict -> every stage is bracketed by the device stopwatch (which synchronises) and its
        milliseconds are added under its name; the channel wavefront then runs on the main stream (step_profile)."""
        d, dev = self.d, self.device
        L = lib()

        class stage:                       # `with stage("soil"):` -- a no-op unless stage_ms was passed
            def __init__(self, name):
                self.name = name

            def __enter__(self):
                if stage_ms is not None:
                    timer_start(dev)

            def __exit__(self, *exc):
                if stage_ms is not None and exc[0] is None:
                    stage_ms[self.name] = stage_ms.get(self.name, 0.0) + timer_stop(dev)
                return False
        if self.meteo is not None:         # snow.dynamic, frost.dynamic: Rain, SnowMelt, isFrozenSoil of this step
            with stage("snow_frost"):
                check(L.lf_snow_frost_members_device(dev, C.byref(self.snow_frost), 1, 3 * self.N, self.N, 0))
        if self.land_fused:
            # canopy, ESMax and the soil columns in ONE pass (k_soil_fused<.., CANOPY>): the lane that runs a column's canopy
            # carries LeafDrainage / Interception / W1a / W1b / W1 / ESMax into its soil water balance in registers
            with stage("land_surface"):
                check(L.lf_land_columns_device(dev, C.byref(self.canopy), C.byref(self.soil), d["ESRef"].ptr,
                                               1 if self.soil_derived else 0))                         # dyn.py:114-123
        else:
            with stage("canopy"):
                check(L.lf_canopy_device(dev, C.byref(self.canopy)))                                    # dyn.py:114
                check(L.lf_scale_rows_device(dev, d["ESRef"].ptr, d["LAITerm"].ptr, d["ESMax"].ptr, 3, self.N))  # soilloop.py:638
            with stage("soil_columns"):
                soil_fn = L.lf_soil_columns_device_derived if self.soil_derived else L.lf_soil_columns_device
                check(soil_fn(dev, C.byref(self.soil)))                                                 # dyn.py:123
        self.steps_done += 1
        self.pixel.TimeSinceStart = float(time_since_start if time_since_start else self.steps_done)
        with stage("pixel_aggregates"):
            check(L.lf_pixel_aggregates_device(dev, C.byref(self.pixel)))                               # dyn.py:129-149
        with stage("overland"):
            step_fn = L.lf_surface_step_ordered if self.pixel_of_position is not None else L.lf_surface_step
            check(step_fn(self.r_direct._h, self.r_other._h, self.r_forest._h, C.byref(self.surface)))   # dyn.py:165
        # The channel wavefront reads nothing but its own vectors and the sideflow gathered below, and nothing of the NEXT
        # step's canopy / soil / aggregate / overland kernels reads a channel vector: it runs on the side stream, beside
        # them (a latency-bound chain of small launches beside bandwidth-bound streaming kernels).  Before the gather
        # overwrites the sideflow the main stream waits for the wavefront of the step before; downloads join by themselves.
        check(L.lf_side_stream_join(dev))
        with stage("sideflow_gather"):
            if self.rmod is not None:       # lakes / reservoirs / inflow / transmission loss inside the wavefront
                m = self.rmod
                check(L.lf_gather_device(dev, self.Nk, self._gidx.ptr, d["ToChanM3RunoffDt"].ptr,
                                         m._st["dev"]["ToChanM3RunoffDt"].ptr))
            else:
                check(L.lf_gather_device(dev, self.Nk, self._gidx.ptr, d["ToChanM3RunoffDt"].ptr,
                                         d["SideflowChanM3"].ptr))
        side = self._side_begin(stage_ms is None)
        try:
            with stage("channel_wavefront"):
                d["sumDisDay"].zero()                                                                   # dyn.py:177
                if self.rmod is not None:
                    m = self.rmod
                    check(L.lf_routing_substeps_fused_structures(self.river._h, C.byref(m._args), C.byref(m._inloop),
                                                                 int(self.sc["NoRoutSteps"])))           # dyn.py:179-180
                else:
                    check(L.lf_routing_substeps_fused(self.river._h, C.byref(self.rout), int(self.sc["NoRoutSteps"]), 0))
        finally:
            self._side_end(side)

    def step_profile(self, forcing, time_since_start=None, ordered=False, season=None):
        """step() with every stage timed on its own (synchronising; no overlap between the stages) -> {stage: ms}"""
        self._season(season)
        ms = {}
        self._step(forcing, time_since_start, ordered, ms)
        return ms

    def stage_bytes(self):
        """algorithmic HBM bytes of one model step, stage by stage: every vector a stage reads or writes counted once
        (8 B per fp64, 1 B per flag; in/out vectors twice), the routers at 48 B per cell and call"""
        N, Nk, n_sub = self.N, self.Nk, int(self.sc["NoRoutSteps"])
        v8 = lambda names: 3 * 8 * len(names)
        canopy = N * (2 * v8(SL._CANOPY_IO) + v8(SL._CANOPY_V_IN) + v8(SL._CANOPY_L_IN) + 8 * len(SL._CANOPY_N_IN) + 3 * 24)
        soil = 3 * N * 504
        kept = self._kept()
        have = lambda names: [k for k in names if k not in OPTIONAL_MAPS or k in kept]
        v_in = [k for k in PA._V_IN if k not in PA_READERS or any(o in kept for o in PA_READERS[k])]
        io = set(have(PA._STATE))
        pixel = N * (v8(v_in) + (24 if "Theta" in kept else 0) + 8 * len(PA._N_IN) + 16 * len(io) +
                     8 * len([k for k in have(PA._OUT) if k not in io]))
        soil -= 3 * N * 8 * len([k for k in ("Theta1a", "Theta1b", "Theta2", "Sat1a", "Sat1b", "Sat1", "Sat2") if k not in kept])
        sio = set(SR._STATE)
        overland = N * (v8(SR._V_IN) + 2 * 24 + 8 * len(SR._N_IN) + 16 * len(sio) + 8 * len([k for k in SR._OUT if k not in sio])
                        + 3 * 48)
        channel = Nk * n_sub * (96 if self.split else 48)
        # the fused land surface: the soil's 504 B per column without the three streams that now stay in registers
        # (LeafDrainage, Interception, ESMax), the canopy's own streams -- 5 read (LAI, LAITerm, CumInterception, CropCoef,
        # CropGroupNumber; its WWP / WFC / W1 reads are the soil's), 7 written -- and the three [N] vectors EWRef, ETRef, ESRef
        land = soil + 3 * N * (-24 + 8 * (5 + 7)) + 24 * N
        out = dict(canopy=canopy, soil_columns=soil, land_surface=land, pixel_aggregates=pixel, overland=overland,
                   sideflow_gather=Nk * 20, channel_wavefront=channel)
        if self.land_fused:
            out.pop("canopy"); out.pop("soil_columns")
        else:
            out.pop("land_surface")
        if self.meteo is not None:         # 48 B read and 57 B (65 with Snow) written per pixel, 24 B of statics
            out["snow_frost"] = N * (48 + 24 + (65 if self.meteo["Snow"] else 57))
        return out

    def download(self, name):
        a = self.d[name].download()
        if name in set(RT._STATIC + RT._STATE + RT._OUT + ["SideflowChanM3"]):
            out = np.zeros(self.N, a.dtype)          # pixels outside the channel domain: their state is identically 0
            out[self.gpix] = a[:self.Nk]
            return out
        return self._pixel_order(a)

    def download_site(self, name):
        """lake / reservoir site vectors (LakeStorageM3CC, ReservoirStorageM3CC, ...) and the dense in-loop outputs"""
        a = self.rmod._st["dev"][name].download()
        if a.size == self.Nk and name not in RT._LAKE_STATE + RT._RES_STATE:
            out = np.zeros(self.N)
            out[self.ids] = self.rmod._down(a)
            return out
        return a

    _CHANNEL_ROWS = set(RT._STATIC + RT._STATE + RT._OUT + ["SideflowChanM3"])        # what download() scatters through gpix

    def rasters(self, names, dtype=np.float32, fill=output.FILL):
        """Report maps of the step just enqueued as [H, W] rasters -- output.decompress(download(name)).astype(dtype) with
        `fill` outside the land mask, bit for bit -- without waiting for them: up to 16 names, each a channel vector,
        "ChanQAvg" (the bits of chan_q_avg()) or an [N] fp64 vector of the land part (not the forcing).  A kernel packs the
        rows as the device holds them into rasters (lf_pack_rasters_device), an asynchronous copy on a stream of its own
        brings them to page-locked memory; the next step() may be issued at once and runs beside the copy.
        -> PendingRasters, whose wait() gives name -> array; the arrays live in one of two buffer sets that alternate call by
        call."""
        groups = {"channel": [], "land": []}
        for name in names:
            if name == "ChanQAvg":                     # Lisflood_dynamic.py:209, as chan_q_avg() divides
                d, divisor, channel = self.d["sumDisDay"], float(self.sc["NoRoutSteps"]), True
            else:
                d, divisor, channel = self.d.get(name), 1.0, name in self._CHANNEL_ROWS
                if d is None or name in self.forcing_names or d.dtype != np.float64 or not (channel or d.shape == (self.N,)):
                    raise ValueError("%s is neither a channel vector, ChanQAvg nor an [N] fp64 vector of the land part" % name)
            groups["channel" if channel else "land"].append((name, d, 1, 0, divisor, False))
        return self._report_rasters(list(groups.items()), dtype, fill, side=not groups["land"])

    # ---- warm start (_HotPath.STATE) -----------------------------------------------------------------------------
    def state_names(self):
        return [k for k in self.STATE if k in self.d]

    def save_state(self, path):
        """every state vector of the chain, pixel order, as one .npz (+ the site vectors of the structures)"""
        out = {k: self.download(k) for k in self.state_names()}
        if self.rmod is not None:
            for k in RT._LAKE_STATE + RT._RES_STATE + ["TransCum"]:
                if k in self.rmod._st["dev"]:
                    out["site_" + k] = self.download_site(k)
        out["steps_done"] = np.int64(self.steps_done)
        np.savez(path, **out)

    def load_state(self, path):
        z = np.load(path)
        self._check_state_file(z.files)
        for k in self.state_names():
            if k not in z.files and k in OPTIONAL_MAPS:
                continue                              # a state file written by an object that did not report this map
            a = z[k]
            if k in _CHANNEL_NAMES:
                self._check_inside(a, "state file holds water in %s on pixels this object left out of the channel "
                                      "domain; build it with compact=False" % k)
                a = a[self.gpix]
            else:
                a = self._ordered(a)
            self.d[k].upload(f64(a))
        if self.rmod is not None:
            for k in RT._LAKE_STATE + RT._RES_STATE + ["TransCum"]:
                if "site_" + k in z.files:
                    a = z["site_" + k]
                    self.rmod._st["dev"][k].upload(f64(self.rmod._up(a[self.ids]) if k == "TransCum" else a))
        self.steps_done = int(z["steps_done"])

    # ---- state maps under the reference's names (default_options.py: the 'repStateMaps' / 'repEndMaps' entries) --------
    # name of the state map -> (attribute, row of a [3,N] array or None).  What the reference writes at a state step and
    # reads back through the *InitValue bindings of a warm run (settings/warm.xml); -9999 in a map read back means "cold
    # start value" (routing.py:203-218, surface_routing.py:49-63, soil.py:239-251, 393-406, groundwater.py:93-107).
    STATE_MAPS = dict(
        ChanQState=("ChanQ", None), ChanCrossSectionState=("TotalCrossSectionArea", None),
        CrossSection2State=("CrossSection2Area", None), ChSideState=("Sideflow1Chan", None),
        OFDirectState=("OFM3Direct", None), OFOtherState=("OFM3Other", None), OFForestState=("OFM3Forest", None),
        CumIntSealedState=("CumInterSealed", None), LZState=("LZ", None),
        CumInterceptionState=("CumInterception", 0), CumInterceptionForestState=("CumInterception", 1),
        CumInterceptionIrrigationState=("CumInterception", 2),
        DSLRState=("DSLR", 0), DSLRForestState=("DSLR", 1), DSLRIrrigationState=("DSLR", 2),
        UZState=("UZ", 0), UZForestState=("UZ", 1), UZIrrigationState=("UZ", 2),
        Theta1State=("Theta1a", 0), Theta1ForestState=("Theta1a", 1), Theta1IrrigationState=("Theta1a", 2),
        Theta2State=("Theta1b", 0), Theta2ForestState=("Theta1b", 1), Theta2IrrigationState=("Theta1b", 2),
        Theta3State=("Theta2", 0), Theta3ForestState=("Theta2", 1), Theta3IrrigationState=("Theta2", 2),
        LakeLevelState=("LakeLevel", None), LakePrevInflowState=("LakeInflowOld", None),
        LakePrevOutflowState=("LakeOutflow", None), ReservoirFillState=("ReservoirFill", None))

    def state_maps(self):
        """dict: reference state-map name -> [N] vector in pixel order -- what `repStateMaps` writes at a state step"""
        out = {}
        chan = {k: self.download(k) for k in ("ChanQ", "ChanM3Kin", "Chan2M3Kin", "Chan2M3Start", "InvChanLength",
                                              "CrossSection2Area", "Sideflow1Chan")}
        m3 = chan["ChanM3Kin"] + chan["Chan2M3Kin"] - chan["Chan2M3Start"] if self.split else chan["ChanM3Kin"]
        chan["TotalCrossSectionArea"] = m3 * chan["InvChanLength"]                  # Lisflood_dynamic.py:194-205
        depth = {k: self.download(k) for k in ("SoilDepth1a", "SoilDepth1b", "SoilDepth2")}
        pore = {k: self.download(k) for k in ("PoreSpaceNotZero1a", "PoreSpaceNotZero1b", "PoreSpaceNotZero2")}
        for name, (attr, row) in self.STATE_MAPS.items():
            if attr in chan:
                out[name] = chan[attr]
            elif attr.startswith("Theta"):          # thetaFun: W / SoilDepth, 0 without pore space (soilloop.py:386-387)
                lay = attr[5:]
                w, d, p = self.download("W" + lay)[row], depth["SoilDepth" + lay][row], pore["PoreSpaceNotZero" + lay][row]
                with np.errstate(divide="ignore", invalid="ignore"):
                    out[name] = np.where(p != 0, w / d, 0.0)
            elif attr in ("LakeLevel", "LakeInflowOld", "LakeOutflow", "ReservoirFill"):
                if self.rmod is None:
                    continue
                cc = {"LakeLevel": "LakeLevelCC", "LakeInflowOld": "LakeInflowOldCC", "LakeOutflow": "LakeOutflowCC",
                      "ReservoirFill": "ReservoirFillCC"}[attr]
                if cc not in self.rmod._st["dev"]:
                    continue
                idx = np.asarray(self.rmod.var.LakeIndex if attr.startswith("Lake") else self.rmod.var.ReservoirIndex)
                dense = np.zeros(self.N)
                dense[self.ids[idx]] = self.rmod._st["dev"][cc].download()          # lakes.py:283-292, reservoir.py:311-315
                out[name] = dense
            elif attr in self.d:
                a = self.download(attr)
                out[name] = a if row is None else a[row]
        return out

    def load_state_maps(self, maps):
        """Warm start from state maps under the reference's names (what a warm run reads through its *InitValue
        bindings); a map that is missing, or -9999, keeps the value this object was constructed with -- the reference's
        cold-start rule.  The channel state is rebuilt from TotalCrossSectionArea / CrossSection2Area exactly as
        routing.initial + initialSecond do (routing.py:203-218, 391-397); like the reference's, such a warm start
        continues to rounding, not to the bit (use save_state / load_state for that)."""
        g = lambda name: (None if name not in maps else np.asarray(maps[name], np.float64))
        up = lambda attr, a: self.d[attr].upload(f64(a[self.gpix] if attr in _CHANNEL_NAMES else self._ordered(a)))
        cur = lambda attr: self.download(attr)
        beta = self.sc["Beta"]
        # channel (routing.py:203-218, 243-248, 391-397)
        area = g("ChanCrossSectionState")
        if area is not None:
            length, alpha = cur("ChanLength"), cur("ChannelAlpha")
            with np.errstate(divide="ignore", invalid="ignore"):
                m3_cur = cur("ChanM3Kin") + (cur("Chan2M3Kin") - cur("Chan2M3Start") if self.split else 0.0)
                chan_m3 = np.where(area == -9999, m3_cur, area * length)
                if self.split:
                    c2 = g("CrossSection2State")
                    c2 = cur("CrossSection2Area") if c2 is None else np.where(c2 == -9999, 0.0, c2)
                    start, alpha2 = cur("Chan2M3Start"), cur("ChannelAlpha2")
                    m3_2 = c2 * length + start
                    m3_1 = chan_m3 - m3_2 + start
                    m3_1 = np.where((m3_1 < 0.0) & (m3_1 > -0.0000001), 0.0, m3_1)
                    up("CrossSection2Area", c2); up("Chan2M3Kin", m3_2); up("ChanM3Kin", m3_1)
                    up("Chan2QKin", (m3_2 * (1 / length) * (1 / alpha2)) ** (1 / beta))
                    up("ChanQKin", (m3_1 * (1 / length) * (1 / alpha)) ** (1 / beta))
                else:
                    up("ChanM3Kin", chan_m3)
                    up("ChanQKin", np.where(alpha > 0, (chan_m3 / length / alpha) ** (1 / beta), 0.0))
        q = g("ChanQState")
        if q is not None:
            up("ChanQ", np.where(q == -9999, cur("ChanQKin"), q))                   # routing.py:332-334
        side = g("ChSideState")
        if side is not None and self.split:
            up("Sideflow1Chan", np.where(side == -9999, 0.0, side))
        # overland flow (surface_routing.py:49-63, 93-95)
        ofa = self.download("OFAlpha")
        for name, row in (("Other", 0), ("Forest", 1), ("Direct", 2)):
            m3 = g("OF%sState" % name)
            if m3 is None:
                continue
            m3 = np.where(m3 == -9999, 0.0, m3)
            up("OFM3" + name, m3)
            up("OFQ" + name, (m3 * (1 / self.sc["PixelLength"]) * (1 / ofa[row])) ** (1 / beta))
        # soil, groundwater, interception
        for attr in ("CumInterception", "DSLR", "UZ"):
            a = cur(attr)
            hit = False
            for name, (at, row) in self.STATE_MAPS.items():
                if at == attr and g(name) is not None:
                    x = g(name)
                    a[row] = np.where(x == -9999, a[row], x)
                    hit = True
            if hit:
                up(attr, np.maximum(a, 1) if attr == "DSLR" else a)                  # soil.py:396-398
        for lay, thetas in (("1a", "Theta1"), ("1b", "Theta2"), ("2", "Theta3")):
            w, depth, pore = cur("W" + lay), cur("SoilDepth" + lay), cur("PoreSpaceNotZero" + lay)
            hit = False
            for row, suffix in enumerate(("State", "ForestState", "IrrigationState")):
                x = g(thetas + suffix)
                if x is not None:
                    w[row] = np.where(pore[row] != 0, np.where(x == -9999, w[row], x * depth[row]), 0.0)   # soil.py:261-267
                    hit = True
            if hit:
                up("W" + lay, w)
        if any(g(n) is not None for n in ("Theta1State", "Theta2State", "Theta1ForestState", "Theta2ForestState",
                                          "Theta1IrrigationState", "Theta2IrrigationState")):
            up("W1", cur("W1a") + cur("W1b"))                                       # soil.py:268
        for name, attr in (("LZState", "LZ"), ("CumIntSealedState", "CumInterSealed")):
            x = g(name)
            if x is not None:
                up(attr, np.where(x == -9999, cur(attr), x))
        if self.rmod is not None:
            dev = self.rmod._st["dev"]
            for name, cc, idx_name in (("LakeLevelState", "LakeLevelCC", "LakeIndex"),
                                       ("LakePrevInflowState", "LakeInflowOldCC", "LakeIndex"),
                                       ("LakePrevOutflowState", "LakeOutflowCC", "LakeIndex"),
                                       ("ReservoirFillState", "ReservoirFillCC", "ReservoirIndex")):
                x = g(name)
                if x is None or cc not in dev:
                    continue
                sites = self.ids[np.asarray(getattr(self.rmod.var, idx_name))]
                val = np.where(x[sites] == -9999, dev[cc].download(), x[sites])
                dev[cc].upload(f64(val))
                if cc == "LakeLevelCC":          # lakes.py:119-121: storage from level x area
                    area = dev["LakeAreaCC"].download()
                    dev["LakeStorageM3CC"].upload(f64(val * area))
                    dev["LakeStorageM3BalanceCC"].upload(f64(val * area))
                if cc == "ReservoirFillCC":      # reservoir.py:152-157
                    dev["ReservoirStorageM3CC"].upload(f64(val * dev["TotalReservoirStorageM3CC"].download()))

    def mass_balance(self):
        """Option repMBTs after a step() with structures: downloads the channel state into the routing module's `var`
        and runs its bookkeeping (routing.mbts_after_fused) -> (MBErrorSplitRoutingM3, OutletDischargeErrorSplitRouting)
        over the channel domain's pixels.  A diagnostic: it synchronises."""
        m = self.rmod
        if m is None:
            raise RuntimeError("mass_balance() needs structures=")
        m.options["repMBTs"] = True
        m._download_state()
        m._structures_download(int(self.sc["NoRoutSteps"]) - 1)
        m.var.ToChanM3RunoffDt = m._down(m._st["dev"]["ToChanM3RunoffDt"].download())
        m.mbts_after_fused()
        return m.var.MBErrorSplitRoutingM3, m.var.OutletDischargeErrorSplitRouting

    def free(self):
        self._free_shared(list(self.d.values()) + [self._gidx] + [a for fs in self.force for a in fs.values()])


class HotPathEnsemble(_HotPath):
    """HotPathDevice for an ENSEMBLE -- members that share the LDDs, the geometry and the parameters and differ in state and
    forcing (a forecast ensemble, a calibration batch over the forcing, an EnKF): one model step of every member costs
    roughly the launches of one member.  Per step:

        lf_land_columns_members_device -> lf_pixel_aggregates_members_device -> lf_surface_step_members
        -> lf_gather_rows_device -> lf_routing_substeps_fused_members (with structures=: ..._structures_members)

    It takes HotPathDevice's inputs; every member starts from `values`.  The non-channel vectors always live in the sweep
    order of the overland graph and the land surface is always the fused one.  The [N] / [3,N] statics, LAI and LAITerm exist
    once; a member's own vectors are rows of one device vector per name: [3,N] rows 3 N + pad elements apart, [N] rows and
    forcing rows N + pad apart (soilloop._EnsembleVectors, whose layout code this class uses), channel rows Nk + pad apart
    (routing.routingEnsemble).  Nothing reads or writes the elements between the rows (gaps / set_gaps).  Every member ends
    up, bit for bit, as a HotPathDevice of its own fed the same forcing.
    Both classes are a _HotPath: the overland routers, the channel domain and the channel router or routing module on it
    come from the same code.  With structures= the channel part is that routing module (_HotPath._routing_module), on the
    compact channel domain with the subset already applied, and its routing.ensemble(members).
    Forcing: there are two sets of member rows of Rain, SnowMelt, EWRef, ETRef and ESRef.  step(forcing) and
    prefetch(forcing) hand the vectors over as the caller holds them -- pixel order, [N] or [members, N], float32 or float64,
    any mix -- with one lf_upload_rows per vector into the set that is NOT in use: one asynchronous copy of the raw image on
    the copy stream and, behind it, a kernel that gathers into sweep order, widens and writes every member's row.  Nothing
    is permuted, widened or laid out on the host, and nothing waits for the main or the side stream: with overlap_channel the
    channel loop of a step runs beside the upload and the land surface of the step after it.  The step then switches to
    that set (lf_compute_acquire .. lf_compute_release around the kernels that read forcing); step(None) stays on the set
    in use, i.e. repeats the forcing of the step before.  pinned_forcing() gives page-locked arrays to fill in place,
    upload_wait() says when they may be refilled -- HotPathDevice's protocol.
    Results: download(name) brings every member's full vector to the host.  What an ensemble is run for is smaller and is
    made on the device, behind the channel loop of the last step: summary(name, ...) -- per pixel the mean, minimum and
    maximum over the members, the members above up to four threshold maps and order statistics (lf_members_summary_device,
    lf_members_order_statistics_device: one pass over the member rows as they lie, only the product maps cross PCIe) -- and
    sample(name, pixels), every member at a few gauges (lf_gather_rows_device), whose rows output.TssWriter.append takes.
    zonal(name, zones, weights=, mean=) is the areal counterpart of sample() -- a satellite footprint, a basin average above
    a gauge, a member's total storage for a water balance: [members, zones] sums or means of a member row over label-map or
    index-list zones (lf_members_zonal_device, one call per pass of a zonal.ZonePlan), in a fixed order so that the fp64
    bits are those of the numpy restatement; assimilation.zone_geometry gives the centroids serial_increments() takes.
    Maps that are written every step do not wait for the device at all: summary_rasters() and rasters() enqueue the pack
    kernel (lf_pack_rasters_device: [H, W] rasters of the writer's type, the fill outside the mask) and an asynchronous
    copy into page-locked memory on a download stream of its own, and return a PendingRasters to wait() on after the next
    step() has been issued.
    Products over the steps of a run -- every member's peak and when it came, whether, when and for how long it was above
    threshold maps, the period mean -- are folded on the device step by step: track_begin(name, thresholds) and from then
    on one lf_members_track_device per step(); the accumulators lie like their source and go through summary() / rasters() /
    sample() / download() as "<name>.peak" and so on.  They are not part of save_state() / load_state().
    The analysis step of an assimilation cycle -- step, sample() the gauges, update every member's state, step -- rewrites
    the state where it lies: transform(weights, taper=, bounds=) applies one [members, members] matrix to every state vector
    element by element (the update of every ensemble Kalman variant; lf_members_transform_device), resample(parents) makes
    member m a copy of member parents[m] (a particle filter's resampling; lf_members_resample_device).  Only the matrix or
    the parents cross PCIe (assimilation.enkf_weights / systematic_parents make them from sample()).  Both rewrite the
    particle -- state_names() and, with structures=, the site state and TransCum -- and leave what belongs to the member's
    slot: forcing sets, inflow-hydrograph rows, trackers, optional diagnostic maps.
    The forecast half of that cycle -- what makes the members differ -- is made on the device as well, from a few static
    spatial patterns and a [members, rank] table of coefficients per step (e.g. an AR(1) in time:
    assimilation.fourier_patterns / ar1_coefficients); only the table crosses PCIe.  forcing_perturbation(name, patterns)
    registers the patterns of a forcing vector, step(forcing, coefficients=) / prefetch(forcing, coefficients=) then write
    every member's row as f * (1 + sum_r c[m, r] P[r]) or f + sum, bounded, on the copy stream behind the upload
    (lf_upload_perturb_rows; an [N] vector goes up as ONE row); perturb(coefficients, patterns, names) does the same to state
    vectors in place (lf_members_perturb_device), which keeps the copies resample() made from staying copies.  Measured at
    2000^2, rank 8, Rain and ETRef perturbed, 4 / 16 / 51 members (tools/bench_members_perturb.py): the prefetched step on
    [N] forcing 12.59 / 46.87 / 139.23 ms, with coefficients 12.72 / 46.66 / 139.66 ms (the two kernels take 0.15 / 0.32 /
    0.65 ms, 0.80 - 0.94 of the copy ceiling at 8 (rank + 1 + members) bytes per element), from host-made [members, N]
    rows 12.67 / 47.17 / 141.54 ms plus 222 / 854 / 2523 ms of numpy per step to make them.
    With meteo= (the dict snow_frost.check_meteo describes: three statics, seven scalars, initial SnowCoverS [3, N] or
    [members, 3, N] and FrostIndex [N] or [members, N]; "Snow": True for the Snow row as well) the forcing is Precipitation,
    Tavg, EWRef, ETRef, ESRef -- what a forecast ensemble differs in, so forcing_perturbation("Tavg", ..., multiplicative=False,
    lower=-inf) and ("Precipitation", ...) act where the spread is -- and step(..., season=(SnowSeasonTerm, SummerSeason)) is
    required.  lf_snow_frost_members_device is then the first launch of the step, ahead of the land surface: one kernel for all
    members writes their Rain, SnowMelt and isFrozenSoil rows (which exist once, not per buffer set; frozen soil is per member)
    and advances SnowCoverS and FrostIndex, which are state -- state_names(), analysis_names(), state files, set_member_state,
    download -- while SnowCover (and Snow) are [N] land rows for summary / rasters / sample / track_begin.  Without meteo=
    nothing of this exists: not an allocation, not a launch, not a name.
    Not in this class (HotPathDevice has them): step_profile, state_maps / load_state_maps and mass_balance."""

    def __init__(self, values, scalars, land_mask, ldd_to_chan, ldd_kinematic, members, split=True, device=0, structures=None,
                 compact=True, overlap_channel=True, report=None, pad=0, meteo=None):
        land_mask = self._begin(scalars, land_mask, split, device, overlap_channel, report, meteo, int(members))
        M = self.members = int(members)
        self._gap = 0.0                      # what lies between the members' rows of the channel part (set_gaps)
        N, sc = self.N, self.sc
        kept, wanted = self._kept(), self._wanted
        chan_names = set(RT._STATIC + RT._STATE)
        # ---- overland routers, and the order of every non-channel vector ------------------------------------------------
        self._overland(values, ldd_to_chan, land_mask)
        # ---- land surface: the member rows and shared statics of LandSurfaceEnsemble -------------------------------------
        d = {k: self._ordered(a) for k, a in values.items() if k not in chan_names}
        if self.meteo is not None:
            d.update({k: self._ordered(a) for k, a in self._meteo_values().items()})
        d.update(sc)
        E = self.land = SL.LandSurfaceEnsemble(d, M, device, pad)
        for k in list(E._member):
            if k in OPTIONAL_MAPS and k not in kept:           # a soil diagnostic nobody asked for: no vector, not computed
                E._member.remove(k)
                E.dev.pop(k).free()
                setattr(E.soil, k, None)
        self.stride, self.pstride = E.stride, E.fstride

        def rows(names, group, shape):
            for k in names:
                if k not in E.dev:
                    group.append(k)
                    E._put(k, d[k] if k in d else np.zeros(shape))

        def statics(names):
            for k in names:
                if k not in E.dev:
                    E._put_static(k, d[k])
        # ---- per-pixel aggregates ---------------------------------------------------------------------------------------
        shared_v, shared_n = ["SoilFraction", "SoilDepthTotal"], PA._N_IN[3:]
        statics(shared_v + shared_n)
        rows(wanted(["Theta"]), E._member, (3, N))
        rows(wanted(PA._STATE + PA._OUT), E._pixel, N)
        p = self.pixel = PA._PixelArgs()
        for k in wanted(PA._V_IN + PA._N_IN + PA._STATE + PA._OUT + ["Theta"]):
            setattr(p, k, E.dev[k].ptr.value)
        # ---- overland step ----------------------------------------------------------------------------------------------
        statics(["OFAlpha"])
        E._static.append("IsChannel")
        E.dev["IsChannel"] = DeviceArray.from_host(u8(d["IsChannel"]), device)
        rows(["SurfaceRunSoil"], E._member, (3, N))
        rows(SR._STATE + SR._OUT, E._pixel, N)
        E.dev["scratch"] = DeviceArray(3 * M * self.pstride, np.float64, device).zero()
        f = self.surface = SR._SurfaceArgs()
        for k in SR._V_IN + SR._N_IN + SR._STATE + SR._OUT + ["SurfaceRunSoil", "scratch"]:
            setattr(f, k, E.dev[k].ptr.value)
        self._finish_args(p, f)
        # ---- snow and frost: the kernel writes the member rows of Rain, SnowMelt and isFrozenSoil, which therefore differ from
        # member to member whatever the forcing -- the land surface and the aggregates always get the member forcing stride --
        # and Precipitation and Tavg are forcing rows like EWRef
        if self.meteo is not None:
            statics(SF.STATICS)
            rows(["SnowCoverS"], E._member, (3, N))
            rows(["FrostIndex", "SnowCover"] + (["Snow"] if self.meteo["Snow"] else []), E._pixel, N)
            for k in SF.METEO:
                E._forcing.append(k)
                E._put(k, np.zeros(N))
            for k in ("Rain", "SnowMelt", "isFrozenSoil"):
                E._shared_forcing[k] = False
            self.snow_frost = self._meteo_block(lambda k: E.dev[k].ptr.value)
        # ---- channel domain and channel part; the members' channel rows ---------------------------------------------------
        v, structures = self._channel(values, ldd_kinematic, land_mask, structures, compact)
        m, Nk = self.rmod, self.Nk
        self.kstride, self._qin = Nk + int(pad), {}
        if m is None:
            self.chan = RT.routingEnsemble(v, self.river, M, self.split, self.kstride, device)
        else:
            self.chan = m.ensemble(M, self.kstride)
        self._engine_order()
        # the sideflow rows of the channel loop: ToChanM3RunoffDt of every member in the channel router's engine order
        self._side = DeviceArray(M * self.kstride, np.float64, device).zero()
        if self.rmod is not None:
            a = self.chan._inloop
            a.ToChanM3RunoffDt = self._side.ptr.value
            if "QInM3Old" in structures:       # inflow hydrographs: QInM3Old / QDelta rows with the stride of the sideflow rows
                self._qin_old = np.broadcast_to(f64(np.broadcast_to(structures["QInM3Old"], (Nk,))), (M, Nk)).copy()
                for k in ("QInM3Old", "QDelta"):
                    self._qin[k] = DeviceArray(M * self.kstride, np.float64, device)
                    self._put_qin(k, np.broadcast_to(m._down(m._st["dev"][k].download()), (M, Nk)))
                    setattr(a, k, self._qin[k].ptr.value)
        # ---- forcing: two sets of member rows; set 0 is the land surface's own vectors (see prefetch) -------------------
        self.force = [{k: E.dev[k] for k in self.forcing_names},
                      {k: DeviceArray(M * self.pstride, np.float64, device).zero() for k in self.forcing_names}]
        self._shared = [{k: E._shared_forcing[k] for k in self.forcing_names}, {k: True for k in self.forcing_names}]
        self._cur, self._prefetched, self._prefetched_coefficients, self._keep = 0, None, None, [None, None]
        # forcing_perturbation(): name -> (patterns on the device in sweep order, rank, multiplicative, lower, upper)
        self._perturbations = {}
        # position -> pixel, for the upload (a blocking copy on the main stream: the memsets of set 1 have ended with it,
        # before the copy stream can write the set)
        self._pidx = DeviceArray.from_host(self.pixel_of_position.astype(np.int32), device)
        # summary() / sample(): engine position -> land pixel on the device (made on first use), the product maps, and the
        # threshold rows and gauge tables by the array object they were made from
        self._gpix_dev, self._row_of_pixel, self._products, self._thresholds, self._gauges = None, {}, {}, {}, {}
        # summary_rasters(): product map -> what its pixels outside the channel domain hold (_summary_outside)
        self._outside_held = {}
        # track_begin(): tracked name -> its accumulators on the device and the number of updates so far
        self._trackers = {}
        # transform(): the weight table on the device ([array object it holds, device table], made on first use), the taper /
        # bound rows on the device by the array object they were made from, and the keys the call in hand uses
        self._weights, self._analysis_cache, self._analysis_pinned = None, {}, set()
        # regress(): the resident table of 256 gauges (made on first use) and the default coordinates (made once)
        self._regress_table, self._regress_coords = None, None
        # zonal(): (zones object, weights object, row kind) -> the plan and its device tables (made on first use)
        self._zonal = {}

    def _lai_vectors(self):
        return self.land.dev

    def _put_qin(self, name, rows, staged=False):
        """[members, Nk] in channel-domain pixel order -> the member rows of QInM3Old / QDelta"""
        host = np.full((self.members, self.kstride), self._gap)
        host[:, :self.Nk] = np.asarray(rows)[:, self.perm]
        self._qin[name].upload(host.reshape(-1), staged=staged)

    # ---- one model step ------------------------------------------------------------------------------------------------------
    def set_inflow(self, QInM3):
        """HotPathDevice.set_inflow with QInM3 [N] (every member) or [members, N]"""
        q, delta = self._inflow(QInM3)
        side = self._side_begin()          # on the channel loop's stream, behind the loop of the step before
        try:
            self._put_qin("QInM3Old", self._qin_old, staged=True)
            self._put_qin("QDelta", delta, staged=True)
        finally:
            self._side_end(side)
        self._qin_old = q

    # ---- forcing: two sets of member rows, uploaded on the copy stream and ordered on the device ----------------------------
    def _upload(self, b, forcing, coefficients=None):
        """the five vectors as the caller holds them into set b: one lf_upload_rows each (raw copy + gather / widen kernel on
        the copy stream, behind the kernels that last read set b); the host arrays stay alive until the set is uploaded again.
        A vector with a forcing_perturbation() and coefficients: an [N] vector goes into member 0's row only and
        lf_upload_perturb_rows, behind it on the copy stream, writes every member's row from that one; [members, N] rows go
        up as always and are perturbed where they lie.  Either way the rows differ from then on (_shared)."""
        L, dev, M, N = lib(), self.device, self.members, self.N
        coeff = self._forcing_coefficients(coefficients)
        self._check_forcing(forcing)
        host = []
        for k in self.forcing_names:
            a = np.asarray(forcing[k])
            if a.shape not in ((N,), (M, N)):
                raise ValueError("forcing vector %s must be [%d] or [%d, %d]" % (k, N, M, N))
            host.append(np.ascontiguousarray(a) if a.dtype == np.float32 else f64(a))
        check(L.lf_upload_begin(dev, b))
        try:
            for k, a in zip(self.forcing_names, host):
                c, rows = coeff.get(k), self.force[b][k].ptr
                check(L.lf_upload_rows(dev, rows, self.pstride, 1 if c is not None and a.ndim == 1 else M,
                                       a.ctypes.data_as(C.c_void_p), 1 if a.ndim == 1 else M, 1 if a.dtype == np.float32 else 0,
                                       N, self._pidx.ptr))
                if c is not None:
                    patterns, rank, multiplicative, lower, upper = self._perturbations[k]
                    check(L.lf_upload_perturb_rows(dev, rows, M, self.pstride, N, rows if a.ndim == 1 else None, rank,
                                                   patterns.ptr, N, c.ctypes.data_as(C.c_void_p), multiplicative, None, lower,
                                                   None, upper))
                self._shared[b][k] = a.ndim == 1 and c is None
        finally:
            check(L.lf_upload_end(dev, b))
        self._keep[b] = host

    def forcing_perturbation(self, name, patterns, multiplicative=True, lower=0.0, upper=np.inf):
        """Register the spatial patterns from which the member rows of forcing vector `name` are perturbed on the device:
        with coefficients={name: c} in step() / prefetch(), c [members, rank] float64, member m's row becomes
            bound(f * (1 + sum_r c[m, r] patterns[r]))   (multiplicative)      bound(f + sum_r c[m, r] patterns[r])   (additive)
        element by element, the sum in ascending r with one multiply and one add each, f the vector as uploaded -- [N], one
        row for every member, or [members, N] -- and bound(v) = lower where lower > v, then upper where upper < v (scalars;
        the defaults keep a flux non-negative).  patterns: [rank, N] float64 in pixel order, rank 1 to 16, e.g.
        assimilation.fourier_patterns(); gathered to sweep order and uploaded here, once, with a blocking copy (the copy
        stream reads them, and nothing orders it behind the main stream but the host).  patterns=None removes the
        registration.  Only the [members, rank] table crosses PCIe per step (lf_upload_perturb_rows)."""
        if name not in self.forcing_names:
            raise ValueError("%s is no forcing vector (%s)" % (name, ", ".join(self.forcing_names)))
        if self.members > 128:
            raise ValueError("a forcing perturbation takes at most 128 members (%d)" % self.members)
        new = None
        if patterns is not None:
            host = np.asarray(patterns, np.float64)
            if host.ndim != 2 or host.shape[1] != self.N or not 1 <= host.shape[0] <= 16:
                raise ValueError("patterns must be [rank, %d] in pixel order with rank 1 to 16" % self.N)
            if multiplicative not in (True, False, 0, 1):
                raise ValueError("multiplicative must be True or False")
            lower, upper = float(lower), float(upper)
            if lower > upper:
                raise ValueError("lower %g is greater than upper %g" % (lower, upper))
            new = (np.ascontiguousarray(host[:, self.pixel_of_position]), host.shape[0], int(bool(multiplicative)), lower, upper)
        old = self._perturbations.pop(name, None)
        if old is not None:
            check(lib().lf_device_synchronize(self.device))     # (a kernel on the copy stream may still read the patterns)
            old[0].free()
        if new is not None:
            self._perturbations[name] = (DeviceArray.from_host(new[0].reshape(-1), self.device),) + new[1:]

    def _forcing_coefficients(self, coefficients):
        """coefficients of step() / prefetch() checked -> name -> contiguous float64 [members, rank]"""
        out = {}
        if coefficients is None:
            return out
        if not isinstance(coefficients, dict):
            raise ValueError("coefficients must be a dict: forcing name -> [members, rank] float64")
        for k, c in coefficients.items():
            if k not in self._perturbations:
                raise ValueError("coefficients for %s, which has no forcing_perturbation()" % k)
            rank = self._perturbations[k][1]
            if np.shape(c) != (self.members, rank):
                raise ValueError("coefficients[%s] must be [%d, %d]" % (k, self.members, rank))
            out[k] = f64(c)
        return out

    def _use_set(self, b):
        """point the argument blocks of the stages that read forcing, and the land surface's own table, at set b"""
        E = self.land
        for k in self.forcing_names:
            E.dev[k] = self.force[b][k]
            for st in (E.canopy, E.soil, self.pixel) + (() if self.meteo is None else (self.snow_frost,)):
                if hasattr(type(st), k):
                    setattr(st, k, self.force[b][k].ptr.value)
        E._shared_forcing.update(self._shared[b])
        self._cur = b

    def forcing_member_stride(self):
        """0 exactly when every forcing vector of the set in use (and isFrozenSoil) is one row for all members"""
        return self.land.forcing_member_stride()

    def pinned_forcing(self, dtype=np.float64, per_member=True):
        """HotPathDevice.pinned_forcing for the ensemble: a forcing dict of page-locked [members, N] arrays ([N] with
        per_member=False) in pixel order, to be filled in place and passed to prefetch() / step().  The DMA reads them after
        the call has returned: upload_wait() before refilling a set that was handed over (or alternate between two sets)."""
        return self._pinned_set((self.members, self.N) if per_member else (self.N,), dtype)

    def prefetch(self, forcing, coefficients=None):
        """Start uploading the forcing of the NEXT step(forcing) call now, into the set that is not in use: the copy and the
        ordering kernel run on the copy stream while the kernels of the step just enqueued are still executing.  Pass the
        same dict object to that step(); a step(None) in between stays on the set in use and leaves the prefetch pending.
        coefficients: as step(); the prefetch carries them, the matching step() passes None or the same dict."""
        if forcing is None and coefficients is not None:
            raise ValueError("coefficients without forcing: the rows on the device are perturbed already")
        self._upload(1 - self._cur, forcing, coefficients)
        self._prefetched, self._prefetched_coefficients = forcing, coefficients

    def step(self, forcing, time_since_start=None, QInM3=None, coefficients=None, season=None):
        """forcing: dict of Rain, SnowMelt, EWRef, ETRef, ESRef, each [N] (every member) or [members, N], pixel order,
        float32 or float64 -- or None: the forcing rows of the step before (no PCIe traffic); QInM3 (structures= with inflow
        hydrographs): [N] or [members, N]; coefficients: None or forcing name -> [members, rank] float64 for vectors with a
        forcing_perturbation(), whose member rows are then perturbed on the device behind their upload.
        With meteo=: Precipitation and Tavg take the place of Rain and SnowMelt, season=(SnowSeasonTerm, SummerSeason) of
        the step is required (snow_frost.season_terms), and lf_snow_frost_members_device is the first launch of the step,
        ahead of the land surface: it makes every member's Rain, SnowMelt and isFrozenSoil rows and advances SnowCoverS and
        FrostIndex; step(None, season=...) repeats the meteo of the step before and still advances them."""
        self._season(season)
        if forcing is None and coefficients is not None:
            raise ValueError("coefficients without forcing: the rows on the device are perturbed already")
        if forcing is not None and self._prefetched is forcing and coefficients is not None \
                and coefficients is not self._prefetched_coefficients:
            raise ValueError("this forcing was prefetched with other coefficients: the prefetch carries them, pass None or "
                             "the same dict")
        if forcing is not None and self._prefetched is not forcing:
            self._forcing_coefficients(coefficients)    # (refused before anything of this step is enqueued)
        if QInM3 is not None:
            self.set_inflow(QInM3)
        L, dev, E, M = lib(), self.device, self.land, self.members
        if forcing is not None:
            if self._prefetched is not forcing:
                self._upload(1 - self._cur, forcing, coefficients)
            self._prefetched = self._prefetched_coefficients = None
            self._use_set(1 - self._cur)
        b = self._cur
        check(L.lf_compute_acquire(dev, b))
        try:
            if self.meteo is not None:            # snow.dynamic, frost.dynamic (Precipitation and Tavg: one row for all, or rows)
                one = self._shared[b]["Precipitation"] and self._shared[b]["Tavg"]
                check(L.lf_snow_frost_members_device(dev, C.byref(self.snow_frost), M, self.stride, self.pstride,
                                                     0 if one else self.pstride))
            E.step()                                                                                        # dyn.py:114-123
            self.steps_done += 1
            self.pixel.TimeSinceStart = float(time_since_start if time_since_start else self.steps_done)
            check(L.lf_pixel_aggregates_members_device(dev, C.byref(self.pixel), M, self.stride, self.pstride,
                                                       E.forcing_member_stride()))                          # dyn.py:129-149
            check(L.lf_surface_step_members(self.r_direct._h, self.r_other._h, self.r_forest._h, C.byref(self.surface), M,
                                            self.stride, self.pstride))                                     # dyn.py:165
        finally:                                  # (nothing behind this point reads forcing: set b may be uploaded again)
            check(L.lf_compute_release(dev, b))
        self._track_update(False)                 # trackers of land rows: on the main stream, behind the overland step
        check(L.lf_side_stream_join(dev))         # (before the gather overwrites the sideflow of the loop of the step before)
        check(L.lf_gather_rows_device(dev, self.Nk, self._gidx.ptr, E.dev["ToChanM3RunoffDt"].ptr, self.pstride,
                                      self._side.ptr, self.kstride, M))
        side = self._side_begin()
        try:
            sums, nsteps = self.chan.vectors.dev["sumDisDay"], int(self.sc["NoRoutSteps"])
            for m in range(M):                    # dyn.py:177, row by row: the elements between the rows stay as they are
                check(L.lf_memset(dev, sums.ptr.value + 8 * m * self.kstride, 0, 8 * self.Nk))
            if self.rmod is not None:
                self.river.routing_substeps_structures_members(self.chan.vectors.args, self.chan._inloop, nsteps, M, self.kstride,
                                                               self.chan.n_lakes, self.chan.n_res, self.kstride)
            else:
                args = self.chan.vectors.with_overrides(SideflowChanM3=self._side.ptr.value)
                self.river.routing_substeps_members(args, nsteps, M, self.kstride, 0, self.kstride)          # dyn.py:179-180
            self._track_update(True)              # trackers of channel rows: behind the channel loop, on its stream
        finally:
            self._side_end(side)

    def last_forms(self):
        """the form every stage of the last step took: land / pixel_aggregates / overland 1 single call, 2 members in one
        launch, 3 member after member; channel: the name of the schedule (kinematicWave.last_fused_form)"""
        out = dict(land=self.land.last_form())
        for stage, name in enumerate(("pixel_aggregates", "overland")):
            rc = lib().lf_module_last_form(self.device, stage)
            if rc < 0:
                check(rc)
            out[name] = rc
        out["channel"] = self.chan.last_fused_form()
        return out

    # ---- vectors -------------------------------------------------------------------------------------------------------------
    def _channel_rows(self, name):
        """(device vector, entries of a row, stride) of a member vector of the channel part, or None"""
        if name in ("SideflowChanM3", "ToChanM3RunoffDt") and (self.rmod is None or name == "ToChanM3RunoffDt"):
            return self._side, self.Nk, self.kstride
        if name in self._qin:
            return self._qin[name], self.Nk, self.kstride
        if name in self.chan._groups:
            count, stride, _ = self.chan._groups[name]
            return self.chan._inloop_dev[name], count, stride
        if name in RT._STATE + RT._OUT:
            return self.chan.vectors.dev[name], self.Nk, self.kstride
        return None

    def _rows_of(self, name):
        """[members, width] rows as the device holds them (channel part), and what lies between them"""
        d, width, stride = self._channel_rows(name)
        flat = np.full(self.members * stride, np.nan)
        a = d.download()
        flat[:min(a.size, flat.size)] = a[:flat.size]
        rows = flat.reshape(self.members, stride)
        return rows[:, :width], rows[:, width:]

    def _to_land(self, rows, engine):
        """[members, Nk] (engine order, or channel-domain pixel order) -> [members, N]; pixels outside the channel domain: 0"""
        out = np.zeros((rows.shape[0], self.N), rows.dtype)
        out[:, self.gpix if engine else self.ids] = rows
        return out

    def download(self, name):
        """[members, N] / [members, 3, N] in pixel order of a member vector, the array itself of a shared one; channel
        vectors scattered to the land domain as HotPathDevice.download does.  The accumulators of a tracker (track_begin):
        "<name>.peak" / ".sum" / ".period_mean" [members, N], "<name>.peak_step" int32 [members, N], "<name>.first_above" /
        ".steps_above" int32 [T, members, N]; outside the channel domain a channel row's are 0.0 and, the integer rows, 0
        (they are not tracked there)"""
        E = self.land
        t, key = self._tracked(name)
        if t is not None:
            rows = self._track_rows(t, key)[0]
            rows = self._to_land(rows.reshape(-1, t.n), True).reshape(rows.shape[:-1] + (self.N,)) if t.channel \
                else self._pixel_order(rows)
            return rows / np.float64(t.steps) if key == "period_mean" else rows
        if name in E.dev and name != "scratch":
            return self._pixel_order(E.get(name))
        if name in self.chan._groups and self.chan._groups[name][2] or name in RT._STATE + RT._OUT + ["SideflowChanM3"]:
            return self._to_land(self._rows_of(name)[0], True)
        if name in RT._STATIC:
            dev = self.chan.vectors.dev if self.rmod is None else self.rmod._dev
            out = np.zeros(self.N, dev[name].dtype)
            out[self.gpix] = dev[name].download()[:self.Nk]
            return out
        raise KeyError(name)

    def download_site(self, name):
        """[members, sites] of a lake / reservoir state vector, [members, N] of a dense in-loop vector; the shared site
        parameters as they are"""
        if self.rmod is None:
            raise RuntimeError("download_site() needs structures=")
        if self._channel_rows(name) is not None:
            rows = self._rows_of(name)[0].copy()
            return self._to_land(rows, True) if rows.shape[1] == self.Nk and name not in RT._LAKE_STATE + RT._RES_STATE else rows
        a = self.rmod._st["dev"][name].download()
        if a.size == self.Nk and name not in RT._LAKE_STATE + RT._RES_STATE:      # a dense vector the members share
            out = np.zeros(self.N)
            out[self.ids] = self.rmod._down(a)
            return out
        return a

    # ---- products over the members, made on the device --------------------------------------------------------------------
    _CACHED = 8            # threshold sets / gauge tables kept per object (the oldest goes first)

    def _product_rows(self, name):
        """(device vector, entries of a row, stride, divisor, channel row?) of a vector summary() and sample() take: a member
        vector of a stage (_source_rows) or an fp64 accumulator of a tracker (track_begin)"""
        t, key = self._tracked(name)
        if t is None:
            return self._source_rows(name)
        if key in _TRACK_I32:
            raise ValueError("%s holds integer rows: download() and rasters() take it, products over the members do not" % name)
        if key == "period_mean":                   # the sum row with the number of updates as its divisor
            return t.dev["sum"], t.n, t.stride, float(t.steps), t.channel
        return t.dev[key], t.n, t.stride, 1.0, t.channel

    def _source_rows(self, name):
        """_product_rows of a member vector of the channel or the land part"""
        if name == "ChanQAvg":                     # Lisflood_dynamic.py:209, as chan_q_avg() divides
            return self.chan.vectors.dev["sumDisDay"], self.Nk, self.kstride, float(self.sc["NoRoutSteps"]), True
        if name in RT._STATE + RT._OUT:
            return self.chan.vectors.dev[name], self.Nk, self.kstride, 1.0, True
        if name in self.land._pixel and name in self.land.dev:
            return self.land.dev[name], self.N, self.pstride, 1.0, False
        raise ValueError("%s is neither a channel row (%s, ChanQAvg) nor an [N] member row of the land part"
                         % (name, ", ".join(RT._STATE + RT._OUT)))

    def _row_index(self, channel):
        """device int32: row position -> land pixel (gpix of the channel rows, made once; _pidx of the land rows)"""
        if not channel:
            return self._pidx
        if self._gpix_dev is None:
            self._gpix_dev = DeviceArray.from_host(self.gpix.astype(np.int32), self.device)
        return self._gpix_dev

    def _product(self, key, shape, dtype=np.float64):
        d = self._products.get(key)
        if d is None or d.shape != tuple(np.atleast_1d(shape).tolist()) or d.dtype != np.dtype(dtype):
            if d is not None:
                d.free()
            d = self._products[key] = DeviceArray(shape, dtype, self.device)
            self._outside_held.pop(key, None)
        return d

    def _cached(self, cache, obj, channel, make):
        """make(obj, channel) once per distinct object: the entry holds the object, so its id stays its own"""
        key = (id(obj), channel)
        hit = cache.get(key)
        if hit is None or hit[0] is not obj:
            while len(cache) >= self._CACHED:
                for d in cache.pop(next(iter(cache)))[1:]:
                    if isinstance(d, DeviceArray):
                        d.free()
            hit = cache[key] = (obj,) + tuple(make(obj, channel))
        return hit[1:]

    def _upload_thresholds(self, thresholds, channel):
        """[T, N] or [N] in pixel order -> (device rows in row order, T, what `exceed` is on the pixels outside the channel
        domain, where every member is 0.0).  Everything summary() needs of the host array: it is not looked at again."""
        a = np.asarray(thresholds, np.float64)
        a = a[None] if a.ndim == 1 else a
        if a.ndim != 2 or a.shape[1] != self.N or not 1 <= a.shape[0] <= 4:
            raise ValueError("thresholds must be [%d] or [T, %d] with T from 1 to 4" % (self.N, self.N))
        rows = np.ascontiguousarray(a[:, self.gpix if channel else self.pixel_of_position])
        fill = (self.members * (0.0 > a[:, self._outside])).astype(np.int32) if channel else None
        return DeviceArray.from_host(rows, self.device), a.shape[0], fill

    def summary(self, name, mean=True, minimum=True, maximum=True, thresholds=None, ranks=None):
        """Per-pixel products over the members of one member vector, made on the device in one pass over the rows
        (lf_members_summary_device; the order statistics: lf_members_order_statistics_device): only the product maps cross
        PCIe.  -> dict of arrays in pixel order over the land domain:
            "mean", "min", "max"  [N]: ((x0 + x1) + ...) / members in member order; np.minimum / np.maximum folded in member
                                  order (a NaN sticks, the earlier member wins a tie);
            "exceed"  [T, N] int32 with thresholds= ([T, N] or [N], pixel order, T <= 4): the members above each map (a NaN on
                      either side does not count).  The maps go to the device once per distinct array object: pass the SAME
                      array every step (a changed copy of it is a new array);
            "order"   [R, N] with ranks= (up to 8 of 0 .. members - 1; at most 128 members):
                      np.sort(x, axis=0, kind="stable")[ranks].
        name: a channel row (RT._STATE + RT._OUT), "ChanQAvg" (sumDisDay / NoRoutSteps, the bits of chan_q_avg()) or an [N]
        member row of the land part.  Pixels outside the channel domain are what download() gives there, 0.0 in every member.
        Runs behind the channel loop of the last step (joins the side stream)."""
        q = self._summary_request(name, mean, minimum, maximum, thresholds, ranks)
        check(lib().lf_side_stream_join(self.device))
        maps = self._summary_maps(q)
        self._summary_kernels(q, maps)
        out = {k: d.download() for k, d in maps.items()}
        if q.channel and self._outside.size:         # the kernels wrote the channel domain's pixels only
            for k, a in out.items():
                a[..., self._outside] = q.fill if k == "exceed" else 0.0
        return out

    def _summary_request(self, name, mean, minimum, maximum, thresholds, ranks):
        """the arguments of summary() checked, the thresholds on the device: what _summary_maps and _summary_kernels take"""
        M = self.members
        src, n, stride, divisor, channel = self._product_rows(name)
        want = [k for k, on in (("mean", mean), ("min", minimum), ("max", maximum)) if on]
        if ranks is not None:
            ranks = np.ascontiguousarray(np.atleast_1d(ranks), np.int32)
            if ranks.ndim != 1 or not 1 <= ranks.size <= 8 or ranks.min() < 0 or ranks.max() >= M:
                raise ValueError("ranks must be 1 to 8 values from 0 to members - 1 = %d" % (M - 1))
            if M > 128:
                raise ValueError("order statistics take at most 128 members (%d)" % M)
        if not want and thresholds is None and ranks is None:
            raise ValueError("summary(): nothing requested")
        thr, T, fill = self._cached(self._thresholds, thresholds, channel, self._upload_thresholds) if thresholds is not None \
            else (None, 0, None)
        return types.SimpleNamespace(src=src, n=n, stride=stride, divisor=divisor, channel=channel, want=want, ranks=ranks,
                                     thr=thr, T=T, fill=fill, index=self._row_index(channel))

    def _summary_maps(self, q):
        """the device product maps of a request, [N] / [T, N] / [R, N] in pixel order"""
        maps = {k: self._product(k, self.N) for k in q.want}
        if q.T:
            maps["exceed"] = self._product("exceed", (q.T, self.N), np.int32)
        if q.ranks is not None:
            maps["order"] = self._product("order", (q.ranks.size, self.N))
        if not q.channel:                            # land rows fill every pixel: whatever _summary_outside wrote is gone
            for k in maps:
                self._outside_held.pop(k, None)
        return maps

    def _summary_kernels(self, q, maps):
        L, dev, M, N = lib(), self.device, self.members, self.N
        if q.want or q.T:
            ptr_of = lambda k: maps[k].ptr if k in maps else None
            check(L.lf_members_summary_device(dev, q.src.ptr, M, q.stride, q.n, q.divisor, q.index.ptr, N, ptr_of("mean"),
                                              ptr_of("min"), ptr_of("max"), q.T, q.thr.ptr if q.T else None, q.n, ptr_of("exceed")))
        if q.ranks is not None:
            check(L.lf_members_order_statistics_device(dev, q.src.ptr, M, q.stride, q.n, q.divisor, q.index.ptr, N, q.ranks.size,
                                                       q.ranks.ctypes.data_as(C.c_void_p), maps["order"].ptr))

    def _summary_outside(self, q, maps):
        """The pixels outside the channel domain of the DEVICE product maps as summary() patches them on the host: 0.0, and
        for `exceed` members * (0.0 > threshold).  The kernels of a channel row never write them, so each map gets them once
        -- again only after a land row has filled the map, after the map has been made anew, or for another threshold set."""
        if not (q.channel and self._outside.size):
            return
        for k, d in maps.items():
            if k == "exceed":
                if self._outside_held.get(k) is not q.fill:
                    host = np.zeros((q.T, self.N), np.int32)
                    host[:, self._outside] = q.fill
                    d.upload(host)
                    self._outside_held[k] = q.fill          # (the array itself: the cache entry of the threshold set owns it)
            elif self._outside_held.get(k) is not True:
                d.zero()
                self._outside_held[k] = True

    def summary_rasters(self, name, mean=True, minimum=True, maximum=True, thresholds=None, ranks=None, dtype=np.float32,
                        fill=output.FILL):
        """summary() as rasters, without waiting: the same kernels into the same device product maps, then the pack kernel
        (lf_pack_rasters_device) and an asynchronous copy into page-locked memory on a stream of its own; the next step() may
        be issued at once and runs beside the copy.  -> PendingRasters; wait() gives "mean" / "min" / "max" [H, W] as `dtype`
        (float32 or float64), "exceed" [T, H, W] int32, "order" [R, H, W] -- output.decompress(summary()[k]).astype(dtype)
        with `fill` outside the land mask ((int32)fill for "exceed"), bit for bit.  The arrays live in one of two buffer
        sets that alternate call by call (shared with rasters()): valid until the request after the next."""
        q = self._summary_request(name, mean, minimum, maximum, thresholds, ranks)
        maps = self._summary_maps(q)
        self._summary_outside(q, maps)
        rows = lambda d: d.shape[0] if len(d.shape) == 2 else 1
        sources = [(k, d, rows(d), self.N, 1.0, len(d.shape) == 2) for k, d in maps.items()]
        return self._report_rasters([("pixel", sources)], dtype, fill, side=q.channel,
                                    produce=lambda: self._summary_kernels(q, maps))

    def rasters(self, names, dtype=np.float32, fill=output.FILL):
        """HotPathDevice.rasters for every member: up to 16 of the vectors summary() takes -- channel rows, "ChanQAvg" (the
        bits of chan_q_avg()), [N] member rows of the land part -- as [members, H, W] rasters each, straight from the rows as
        the device holds them.  The accumulators of a tracker (track_begin) too: "<name>.peak" / ".sum" / ".period_mean" like
        any fp64 row, "<name>.peak_step" as int32 [members, H, W], "<name>.first_above" / ".steps_above" as int32
        [T, members, H, W] (the int32 fill outside the mask, 0 on land pixels outside the channel domain: the integer rows
        are not tracked there).  -> PendingRasters"""
        groups = {"channel": [], "land": []}
        for name in names:
            t, key = self._tracked(name)
            if key in _TRACK_I32:
                lead = (self.members,) if key == "peak_step" else (t.T, self.members)
                groups["channel" if t.channel else "land"].append((name, t.dev[key], int(np.prod(lead)), t.stride, 1.0, lead))
                continue
            src, _, stride, divisor, channel = self._product_rows(name)
            groups["channel" if channel else "land"].append((name, src, self.members, stride, divisor, True))
        return self._report_rasters(list(groups.items()), dtype, fill, side=not groups["land"])

    def _position_of_pixel(self, channel):
        """int64 [N]: compressed land index -> row position of the channel rows (or the land rows), -1 outside their domain"""
        if channel not in self._row_of_pixel:
            row = np.full(self.N, -1, np.int64)
            row[self.gpix if channel else self.pixel_of_position] = np.arange(self.Nk if channel else self.N)
            self._row_of_pixel[channel] = row
        return self._row_of_pixel[channel]

    def _gauge_table(self, pixels, channel):
        """compressed land indices -> (device index in row positions, device [members, gauges] rows, gauges inside the
        rows' domain); a gauge outside it reads position 0 and is set to 0.0 afterwards"""
        pix = np.asarray(pixels, np.int64).reshape(-1)
        if pix.size and (pix.min() < 0 or pix.max() >= self.N):
            raise ValueError("pixels must be compressed land indices 0 .. %d" % (self.N - 1))
        row = self._position_of_pixel(channel)[pix]
        inside = row >= 0
        if not pix.size:
            return None, None, inside
        return (DeviceArray.from_host(np.where(inside, row, 0).astype(np.int32), self.device),
                DeviceArray(self.members * pix.size, np.float64, self.device), inside)

    def sample(self, name, pixels):
        """[members, len(pixels)]: the vectors summary() takes at compressed land indices (gauges) -- download(name)[:, pixels]
        without the full vectors: one lf_gather_rows_device and members * len(pixels) doubles over PCIe.  A gauge outside
        the channel domain gives 0.0 for a channel row; "ChanQAvg" divides on the host.  The index table is kept per
        `pixels` array object: pass the same array every step."""
        L, dev, M = lib(), self.device, self.members
        src, n, stride, divisor, channel = self._product_rows(name)
        idx, dst, inside = self._cached(self._gauges, pixels, channel, self._gauge_table)
        G = inside.size
        if G == 0 or n == 0:
            return np.zeros((M, G))
        check(L.lf_side_stream_join(dev))
        check(L.lf_gather_rows_device(dev, G, idx.ptr, src.ptr, stride, dst.ptr, G, M))
        rows = dst.download().reshape(M, G)
        rows[:, ~inside] = 0.0
        return rows / divisor if divisor != 1.0 else rows

    # ---- sums and means of the member rows over zones, in the fixed order of a zonal.ZonePlan ------------------------------
    def _zonal_tables(self, zones, weights, channel):
        """What zonal() keeps per (zones object, weights object, row kind), made once and cached like threshold sets and
        gauge tables: the ZonePlan and on the device its index, its weights, the run table of every pass and the two partial
        buffers the passes alternate between.  The entry holds both objects, so their ids stay their own."""
        key = (id(zones), id(weights), channel)
        hit = self._zonal.get(key)
        if hit is not None and hit.zones is zones and hit.weights is weights:
            return hit
        stale = [key] if hit is not None else list(self._zonal)[:max(0, len(self._zonal) - self._CACHED + 1)]
        for k in stale:                                # (an id that went to another object; beyond _CACHED the oldest)
            for d in self._zonal.pop(k).arrays:
                d.free()
        plan = ZN.row_plan(zones, weights, self.N, self.gpix if channel else self.pixel_of_position, self._position_of_pixel(channel))
        up = lambda a: DeviceArray.from_host(a, self.device) if a is not None and a.size else None
        t = types.SimpleNamespace(zones=zones, weights=weights, plan=plan, index=up(plan.positions), wdev=up(plan.weights),
                                  run_start=[up(s) for s in plan.run_start],
                                  partial=[DeviceArray(self.members * max(1, plan.runs(p)), np.float64, self.device)
                                           for p in range(min(2, plan.passes))])
        t.arrays = [d for d in [t.index, t.wdev] + t.run_start + t.partial if d is not None]
        self._zonal[key] = t
        return t

    def zonal_plan(self, zones, weights=None, name="LZ"):
        """the zonal.ZonePlan zonal(name, zones, weights) sums by: which pixels go into which zone, in what order and in
        which runs (the plan of a channel row differs from that of a land row: other positions, fewer pixels)"""
        return self._zonal_tables(zones, weights, self._product_rows(name)[4]).plan

    def zonal(self, name, zones, weights=None, mean=True):
        """[members, Z]: every member's sum -- or, with mean=True, mean -- of one member vector over Z zones, made on the
        device in a fixed order (lf_members_zonal_device, one call per pass of the plan; include/lisflood_amd.h states the
        arithmetic, zonal.ZonePlan the order): only members * Z doubles cross PCIe, and the bits are those of the numpy
        restatement on download(name) whatever the launch shape.
        name: anything summary() takes -- a channel row, "ChanQAvg" (through the divisor), an [N] member row of the land
        part (Theta1aPixel, SnowCover, LZ ...), an fp64 tracker row such as "LZ.period_mean".
        zones: an int label map [N] in pixel order (labels 0 .. Z - 1, negative: no zone) or a sequence of Z arrays of
        compressed land indices, which may overlap (the nested upstream areas of gauges).  weights: [N] in pixel order, e.g.
        the pixel area; a value is x / divisor * weight, two roundings.  For a channel row a zone holds only its pixels
        inside the channel domain, and so does its weight sum.
        mean=True divides the sums on the host by plan.weight_sum (the same ordered sum over the weights, or the number of
        pixels): an empty zone has the sum 0.0 and the mean NaN.
        The plan and its device tables are kept per (zones object, weights object, row kind): pass the SAME arrays every
        step.  Runs behind the channel loop of the last step (joins the side stream), like sample()."""
        L, dev, M = lib(), self.device, self.members
        src, _, stride, divisor, channel = self._product_rows(name)
        t = self._zonal_tables(zones, weights, channel)
        plan = t.plan
        sums = np.zeros((M, plan.zones))
        if plan.zones == 0:
            return sums
        check(L.lf_side_stream_join(dev))
        rows, entries = src.ptr, plan.entries
        for p in range(plan.passes):
            first, runs, out = p == 0, plan.runs(p), t.partial[p % 2]
            check(L.lf_members_zonal_device(dev, rows, M, stride, divisor if first else 1.0, entries,
                                            t.index.ptr if first and t.index else None, t.wdev.ptr if first and t.wdev else None,
                                            runs, t.run_start[p].ptr, out.ptr, runs))
            rows, stride, entries = out.ptr, runs, runs
        check(L.lf_memcpy_d2h(dev, ptr(sums), rows, sums.nbytes))
        if not mean:
            return sums
        with np.errstate(divide="ignore", invalid="ignore"):
            return sums / plan.weight_sum

    # ---- products over the steps of a run: accumulators per member, updated on the device by every step -------------------
    _TRACK_MAX = 4         # names tracked at once

    def track_begin(self, name, thresholds=None):
        """From now on every step() folds the member rows of `name` -- anything summary() takes: a channel row, "ChanQAvg",
        an [N] member row of the land part -- into accumulators that stay on the device (lf_members_track_device, one call
        per tracked name and step, no host synchronisation; a channel row behind the channel loop on its stream, a land row
        on the main stream behind the overland step):
            "<name>.peak"         the largest value of every member so far (np.maximum in step order: a NaN sticks, the
                                  earlier step wins a tie), "<name>.peak_step" int32: the update it came with (0-based);
            "<name>.sum"          the sum in step order, "<name>.period_mean": the sum / track_steps(name);
            "<name>.first_above"  int32 [T, members, .]: the first update with value > threshold map t (-1: none yet),
            "<name>.steps_above"  int32 [T, members, .]: how many updates had it above -- with thresholds= ([T, N] or [N] in
                                  pixel order, T <= 4, uploaded here once).
        The accumulators lie as their source does, same stride: the three fp64 names go wherever the source's name goes
        (summary, summary_rasters, rasters, sample, download), so summary("ChanQAvg.peak", thresholds=...)["exceed"] is the
        members that exceeded a map at any time of the horizon.  The int32 names go to download() and rasters().  On land
        pixels outside the channel domain a channel row's fp64 accumulators read 0.0 like every channel row; the int32 ones
        read 0: they are not tracked there.  Until the first update every derived name raises RuntimeError.  At most 4
        names at once.  Trackers are not part of save_state() / load_state()."""
        if name in self._trackers:
            raise ValueError("%s is tracked already" % name)
        if len(self._trackers) >= self._TRACK_MAX:
            raise ValueError("at most %d names are tracked at once (%s)" % (self._TRACK_MAX, ", ".join(self._trackers)))
        _, n, stride, _, channel = self._source_rows(name)
        thr, T = None, 0
        if thresholds is not None:
            thr, T, _ = self._upload_thresholds(thresholds, channel)
        M, dev = self.members, {}
        for key, rows, dtype, gap in (("peak", M, np.float64, self._gap), ("sum", M, np.float64, self._gap),
                                      ("peak_step", M, np.int32, TRACK_GAP_I32), ("first_above", T * M, np.int32, TRACK_GAP_I32),
                                      ("steps_above", T * M, np.int32, TRACK_GAP_I32)):
            if rows:                      # (what lies between the rows is set here and never touched again)
                dev[key] = DeviceArray.from_host(np.full(rows * stride, gap, dtype), self.device)
        self._trackers[name] = types.SimpleNamespace(name=name, n=n, stride=stride, channel=channel, thr=thr, T=T, dev=dev, steps=0)

    def _tracker(self, name):
        if name not in self._trackers:
            raise ValueError("%s is not tracked (track_begin)" % name)
        return self._trackers[name]

    def _tracked(self, name):
        """(tracker, key) of a derived name "<tracked name>.<key>", (None, None) of any other name"""
        base, _, key = str(name).rpartition(".")
        t = self._trackers.get(base)
        if t is None or key not in _TRACK_F64 + _TRACK_I32:
            return None, None
        if key in ("first_above", "steps_above") and not t.T:
            raise ValueError("%s is tracked without thresholds" % base)
        if t.steps == 0:
            raise RuntimeError("%s: no step() since track_begin / track_reset, the accumulators hold nothing yet" % name)
        return t, key

    def _track_update(self, channel):
        """one lf_members_track_device per tracked channel row (or land row) on the stream the calls go to now"""
        L, M = lib(), self.members
        for t in self._trackers.values():
            if t.channel is not channel:
                continue
            src, n, stride, divisor, _ = self._source_rows(t.name)
            p = lambda k: t.dev[k].ptr if k in t.dev else None
            check(L.lf_members_track_device(self.device, src.ptr, M, stride, n, divisor, t.steps, int(t.steps == 0), t.stride,
                                            p("peak"), p("peak_step"), p("sum"), t.T, t.thr.ptr if t.T else None, n,
                                            p("first_above"), p("steps_above")))
            t.steps += 1

    def track_steps(self, name):
        """the updates of a tracker since track_begin() / track_reset(): the next one's step index"""
        return self._tracker(name).steps

    def track_reset(self, name):
        """a new horizon: the next step() starts the accumulators over (it reads none of them) with step index 0.  Nothing
        is enqueued; until that step the derived names raise RuntimeError."""
        self._tracker(name).steps = 0

    def track_end(self, name):
        """stop tracking `name` and free its accumulators (waits for the step in flight)"""
        t = self._tracker(name)
        check(lib().lf_device_synchronize(self.device))
        for d in list(t.dev.values()) + [t.thr]:
            if d is not None:
                d.free()
        del self._trackers[name]

    def _track_rows(self, t, key):
        """(rows, what lies between them) of an accumulator as the device holds it: [members, .] or [T, members, .]"""
        d = t.dev["sum" if key == "period_mean" else key]
        lead = (t.T, self.members) if key in ("first_above", "steps_above") else (self.members,)
        rows = d.download().reshape(lead + (t.stride,))
        return rows[..., :t.n], rows[..., t.n:]

    def track_gaps(self, name, key):
        """gaps() of an accumulator (key: "peak", "sum", "peak_step", "first_above", "steps_above"): the elements between
        its rows, which no call reads or writes -- in the fp64 rows the gap value at the time of track_begin() (set_gaps()
        does not reach the trackers), TRACK_GAP_I32 in the int32 rows"""
        t = self._tracker(name)
        if key not in t.dev:
            raise ValueError("%s has no accumulator %s" % (name, key))
        return self._track_rows(t, key)[1]

    def state_names(self):
        return [k for k in self.STATE if k in self.land.dev or k in RT._STATE]

    def set_member_state(self, name, rows):
        """a state vector of every member from [members, N] / [members, 3, N] in pixel order"""
        if name not in self.state_names():
            raise ValueError("%s is no state vector of this object" % name)
        rows = np.asarray(rows, np.float64)
        if name not in RT._STATE:
            shape = (self.members, 3, self.N) if name in self.land._member else (self.members, self.N)
            if rows.shape != shape:
                raise ValueError("%s must be %s" % (name, list(shape)))
            return self.land.set(name, self._ordered(rows))
        if rows.shape != (self.members, self.N):
            raise ValueError("%s must be [%d, %d]" % (name, self.members, self.N))
        self._check_inside(rows, "state file holds water in %s on pixels this object left out of the channel "
                                 "domain; build it with compact=False" % name)
        self._set_channel_rows(name, rows[:, self.gpix])

    def _set_channel_rows(self, name, rows):
        """rows as the device holds them; the elements between them keep the gap value"""
        d, width, stride = self._channel_rows(name)
        host = np.full((self.members, stride), self._gap)
        host[:, :width] = rows
        d.upload(np.ascontiguousarray(host.reshape(-1)[:d.nbytes // 8]), prefix=False)

    # ---- the analysis step: every member's state rewritten on the device from the members' rows as they lie --------------------
    _ROWS_CACHED = 64      # taper / bound rows kept on the device (per array object and row order; the oldest goes first)

    def analysis_names(self):
        """what transform() and resample() rewrite by default: every vector of state_names() and, with structures=, the lake
        and reservoir state rows and TransCum that save_state() writes"""
        names = self.state_names()
        if self.rmod is not None:
            names += [k for k in RT._LAKE_STATE + RT._RES_STATE + ["TransCum"] if k in self.chan._groups]
        return names

    def _analysis_names(self, names):
        known = self.analysis_names()
        if names is None:
            return known
        names = [names] if isinstance(names, str) else list(names)
        for k in names:
            if k not in known:
                raise ValueError("%s is no state vector of this object (analysis_names(): %s)" % (k, ", ".join(known)))
        if len(set(names)) != len(names):
            raise ValueError("names holds a vector twice: it would be rewritten twice")
        return names

    def _analysis_rows(self, name):
        """the row sets of a state vector -> [(address of member 0's row, entries, stride, row order, row of a [3, N] vector)]:
        a [3, N] member vector is three sets on the offsets v N, a site vector's rows lie back to back"""
        E = self.land
        if name in E.dev and name not in RT._STATE:
            base = E.dev[name].ptr.value
            if name in E._member:
                return [(base + 8 * v * self.N, self.N, self.stride, "land", v) for v in range(E.V)]
            return [(base, self.N, self.pstride, "land", None)]
        d, width, stride = self._channel_rows(name)
        order = "lake" if name in RT._LAKE_STATE else "res" if name in RT._RES_STATE else "channel"
        return [(d.ptr.value, width, stride, order, None)]

    def _pixel_rows(self, a, order, v=None):
        """The device row of a per-pixel host array ([N] in pixel order, or row v of a [3, N] one; v = "all": every row of a
        [rank, N] one, N' entries apart, the patterns of perturb()) in the order of a row set:
        "land" sweep order, "channel" engine order, "lake" / "res" the site's pixel.  Gathered and uploaded once per array
        object and order: pass the SAME array every cycle (a changed copy of it is a new array).  The rows a transform() call
        has resolved are pinned (_analysis_pinned) until its kernels are enqueued: what makes room for a new row is the row
        used longest ago that the call in hand does NOT use, and where it uses them all the cache grows instead."""
        key = (id(a), order, v)
        self._analysis_pinned.add(key)
        hit = self._analysis_cache.pop(key, None)                   # (the entry holds its array, so the id is the array's own)
        if hit is not None:
            self._analysis_cache[key] = hit                         # (used last: to the back of the queue)
        else:
            if order in ("lake", "res"):
                var = self.rmod.var
                index = self.ids[np.asarray(var.LakeIndex if order == "lake" else var.ReservoirIndex, np.int64)]
            else:
                index = self.pixel_of_position if order == "land" else self.gpix
            host = np.asarray(a, np.float64)
            host = host if host.ndim == 1 or v == "all" else host[v]
            while len(self._analysis_cache) >= self._ROWS_CACHED:
                old = next((k for k in self._analysis_cache if k not in self._analysis_pinned), None)
                if old is None:
                    break
                check(lib().lf_device_synchronize(self.device))     # (a kernel of an earlier call may still read it)
                self._analysis_cache.pop(old)[1].free()
            rows = np.ascontiguousarray(host[..., index]).reshape(-1)
            hit = self._analysis_cache[key] = (a, DeviceArray.from_host(rows, self.device))
        return hit[1]

    def _analysis_bounds(self, names, bounds):
        """bounds of transform() checked -> name -> (lower, upper), each None, a float or an array"""
        out = {}
        for name, pair in (bounds or {}).items():
            if name not in names:
                raise ValueError("bounds for %s, which is not among the names of this call" % name)
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError("bounds[%s] must be (lower, upper)" % name)
            shapes = [(self.N,)] + ([(self.land.V, self.N)] if name in self.land._member else [])
            checked = []
            for b in pair:
                if b is not None and np.ndim(b) == 0:
                    b = float(b)
                elif b is not None and np.shape(b) not in shapes:
                    raise ValueError("a bound of %s must be None, a scalar or an array of shape %s"
                                     % (name, " or ".join(str(list(s)) for s in shapes)))
                checked.append(b)
            if isinstance(checked[0], float) and isinstance(checked[1], float) and checked[0] > checked[1]:
                raise ValueError("bounds[%s]: lower %g is greater than upper %g" % ((name,) + tuple(checked)))
            out[name] = tuple(checked)
        return out

    def transform(self, weights, names=None, taper=None, bounds=None):
        """The update of an ensemble Kalman analysis (stochastic EnKF, ETKF, an ensemble smoother) on the device: for every
        element i of every state vector, x_new[m, i] = sum_k x[k, i] weights[k][m], summed in ascending k with one multiply
        and one add each, in place on the member rows as they lie (lf_members_transform_device: one call per row set, a
        [3, N] vector three).  Only `weights` -- [members, members] float64, e.g. assimilation.enkf_weights() of sample() at
        the gauges -- crosses PCIe: into one resident table, asynchronously, whenever the array object is not the one of the
        call before (a changed copy of it is a new array); at most 64 members.
        names: the vectors to rewrite, by default analysis_names().  NOT touched, whatever the names: the forcing sets, the
        inflow-hydrograph rows (QInM3Old, QDelta and the host's copy of the last inflow), the trackers' accumulators, the
        optional diagnostic maps and every output of a step -- each belongs to the member's slot, not to the particle.
        taper: None or [N] in pixel order, the localisation: x_new = x + taper * (x_new - x) element by element (a site
        row takes the taper at the site's pixel).
        bounds: name -> (lower, upper), applied after the taper; each None, a scalar or an array in pixel order -- [N], or
        [3, N] for a [3, N] vector -- and v = lower where lower > v or lower is a NaN, then the same with upper from above.
        Arrays go to the device once per object, like thresholds.  Names without an entry are unbounded.
        Joins the side stream (runs behind the channel loop of the last step) and enqueues: no host synchronisation, the
        next step() sees the new state; steps_done stays."""
        M, N = self.members, self.N
        if M > 64:
            raise ValueError("transform() takes at most 64 members (%d)" % M)
        if not (isinstance(weights, np.ndarray) and weights.dtype == np.float64 and weights.shape == (M, M)):
            raise ValueError("weights must be a float64 array of shape [%d, %d]" % (M, M))
        if taper is not None and np.shape(taper) != (N,):
            raise ValueError("taper must be [%d] in pixel order" % N)
        names = self._analysis_names(names)
        bounds = self._analysis_bounds(names, bounds)
        calls = []
        self._analysis_pinned = set()             # the rows this call uses stay until its kernels are enqueued (_pixel_rows)
        try:
            for name in names:
                lower, upper = bounds.get(name, (None, None))
                for base, n, stride, order, v in self._analysis_rows(name):
                    arg = lambda b, inf: (None, inf) if b is None else (None, b) if isinstance(b, float) \
                        else (self._pixel_rows(b, order, v).ptr, 0.0)
                    if n:
                        calls.append((base, stride, n, None if taper is None else self._pixel_rows(taper, order).ptr)
                                     + arg(lower, -np.inf) + arg(upper, np.inf))
            L, dev = lib(), self.device
            check(L.lf_side_stream_join(dev))
            # ONE weight table on the device.  A new array object (enkf_weights() returns one every cycle) goes into it through
            # a page-locked staging slot, in order on the main stream behind the kernels of the call before: nothing is
            # allocated or freed from cycle to cycle, so nothing synchronises.  The same object again: no upload.
            if self._weights is None:
                self._weights = [None, DeviceArray(M * M, np.float64, dev)]
            if self._weights[0] is not weights:
                self._weights[1].upload(np.ascontiguousarray(weights).reshape(-1), staged=True)
                self._weights[0] = weights
            w = self._weights[1]
            for base, stride, n, tp, lo_dev, lo, hi_dev, hi in calls:
                check(L.lf_members_transform_device(dev, base, M, stride, n, w.ptr, tp, lo_dev, lo, hi_dev, hi))
        finally:
            self._analysis_pinned = set()

    _REGRESS_GAUGES = 256  # gauges of one lf_members_regress_device call: what the resident table is sized for

    def regress(self, increments, names=None, coords=None, bounds=None):
        """The localised serial analysis on the device (the two-step filter of Anderson 2003 with Gaspari-Cohn localisation):
        the observation-space increments of ALL gauges -- `increments`, what assimilation.serial_increments() made of
        sample() at the gauges -- regressed onto every element of every state vector in ONE pass over the state, each gauge
        weighted by gaspari_cohn(distance to the gauge / its half-width) computed on the device from coordinates, in place
        on the member rows as they lie (lf_members_regress_device, whose header entry states the arithmetic: one call per
        row set, a [3, N] vector three).  The same analysis through transform() is one pass and one [N] taper map per gauge.
        Only the table of increments.gauges (2 members + 5) doubles crosses PCIe, through a page-locked slot into one
        resident buffer made on first use for 256 gauges.  The page-locked slots are the device's ring of eight, shared with
        every other staged upload, and a slot grows the first time it meets a table larger than itself: the first eight or so
        calls, or a later call with more gauges than any before, may each allocate page-locked memory once; after that
        nothing is allocated from cycle to cycle.  More than 256 gauges
        go in several calls, in order: the filter is serial, so that is the same arithmetic.  2 to 64 members.
        names, bounds, what stays untouched and the ordering (joins the side stream, enqueues, no host synchronisation):
        as transform().  Without bounds an element beyond every gauge's reach (twice the half-width) keeps its bits.
        coords: None or (X, Y), two [N] float64 arrays in pixel order, the coordinates the distances are taken in -- the
        gauges' in `increments` are in the same.  None: the pixel's (row, column) on the land mask, made once and kept.
        They go to the device once per array object and row order, like taper and bound rows: pass the SAME arrays every
        cycle.  A site row takes its pixel's coordinates.  No gauge kept in `increments`: nothing is launched."""
        M, N = self.members, self.N
        if not 2 <= M <= 64:
            raise ValueError("regress() takes 2 to 64 members (%d)" % M)
        sections = ("anomalies", "increments", "scale", "gx", "gy", "halfwidth", "cut2", "gauges", "members", "chunk")
        if not all(hasattr(increments, k) for k in sections):
            raise ValueError("increments must be what assimilation.serial_increments() returns")
        if increments.members != M:
            raise ValueError("increments are of %d members, the ensemble has %d" % (increments.members, M))
        if coords is None:
            if self._regress_coords is None:
                rows, cols = np.nonzero(self.land_mask)
                self._regress_coords = (rows.astype(np.float64), cols.astype(np.float64))
            coords = self._regress_coords
        if not (isinstance(coords, (tuple, list)) and len(coords) == 2
                and all(isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (N,) for a in coords)):
            raise ValueError("coords must be None or (X, Y), two float64 arrays of shape [%d] in pixel order" % N)
        names = self._analysis_names(names)
        bounds = self._analysis_bounds(names, bounds)
        G = int(increments.gauges)
        if G == 0:
            return
        calls = []
        self._analysis_pinned = set()
        try:
            for name in names:
                lower, upper = bounds.get(name, (None, None))
                for base, n, stride, order, v in self._analysis_rows(name):
                    arg = lambda b, inf: (None, inf) if b is None else (None, b) if isinstance(b, float) \
                        else (self._pixel_rows(b, order, v).ptr, 0.0)
                    if n:
                        calls.append((base, stride, n, self._pixel_rows(coords[0], order).ptr, self._pixel_rows(coords[1], order).ptr)
                                     + arg(lower, -np.inf) + arg(upper, np.inf))
            L, dev = lib(), self.device
            check(L.lf_side_stream_join(dev))
            if self._regress_table is None:
                self._regress_table = DeviceArray(self._REGRESS_GAUGES * (2 * M + 5), np.float64, dev)
            t = self._regress_table
            for first in range(0, G, self._REGRESS_GAUGES):
                last = min(first + self._REGRESS_GAUGES, G)
                # in order on the stream behind the kernels of the chunk before, which read the table it overwrites
                t.upload(increments.table if (first, last) == (0, G) else increments.chunk(first, last), staged=True, prefix=True)
                for base, stride, n, cx, cy, lo_dev, lo, hi_dev, hi in calls:
                    check(L.lf_members_regress_device(dev, base, M, stride, n, last - first, cx, cy, t.ptr, lo_dev, lo, hi_dev, hi))
        finally:
            self._analysis_pinned = set()

    def perturb(self, coefficients, patterns, names, multiplicative=False, bounds=None):
        """Model error or jitter on the device: for every element i of the state vectors `names`, in place on the member
        rows as they lie,  x[m, i] = x[m, i] + sum_r coefficients[m, r] patterns[r, i]  (multiplicative: x[m, i] * (1 + sum)),
        summed in ascending r with one multiply and one add each (lf_members_perturb_device: one call per row set, a [3, N]
        vector three, each with the same patterns).  It is what keeps the copies that resample() made from staying copies.
        coefficients: [members, rank] float64, e.g. assimilation.ar1_coefficients(); only they cross PCIe, through a
        page-locked slot.  patterns: [rank, N] float64 in pixel order, rank 1 to 16, e.g. assimilation.fourier_patterns();
        laid out per row order and uploaded once per array object, like taper and bound rows (pass the SAME array every
        cycle); a site row takes the pattern at the site's pixel.  names: required -- a vector of analysis_names() or a list
        of them.  bounds: as transform().  At most 128 members.  Ordered like transform(): joins the side stream and
        enqueues, no host synchronisation."""
        M, N = self.members, self.N
        if M > 128:
            raise ValueError("perturb() takes at most 128 members (%d)" % M)
        if not (isinstance(patterns, np.ndarray) and patterns.dtype == np.float64 and patterns.ndim == 2
                and patterns.shape[1] == N and 1 <= patterns.shape[0] <= 16):
            raise ValueError("patterns must be a float64 array of shape [rank, %d] in pixel order with rank 1 to 16" % N)
        rank = patterns.shape[0]
        if np.shape(coefficients) != (M, rank):
            raise ValueError("coefficients must be [%d, %d]" % (M, rank))
        if names is None:
            raise ValueError("names is required: the state vectors to perturb")
        c = f64(coefficients)
        names = self._analysis_names(names)
        bounds = self._analysis_bounds(names, bounds)
        calls = []
        self._analysis_pinned = set()
        try:
            for name in names:
                lower, upper = bounds.get(name, (None, None))
                for base, n, stride, order, v in self._analysis_rows(name):
                    arg = lambda b, inf: (None, inf) if b is None else (None, b) if isinstance(b, float) \
                        else (self._pixel_rows(b, order, v).ptr, 0.0)
                    if n:
                        calls.append((base, stride, n, self._pixel_rows(patterns, order, "all").ptr)
                                     + arg(lower, -np.inf) + arg(upper, np.inf))
            L, dev = lib(), self.device
            check(L.lf_side_stream_join(dev))
            for base, stride, n, pt, lo_dev, lo, hi_dev, hi in calls:
                check(L.lf_members_perturb_device(dev, base, M, stride, n, None, rank, pt, n, c.ctypes.data_as(C.c_void_p),
                                                  int(bool(multiplicative)), lo_dev, lo, hi_dev, hi))
        finally:
            self._analysis_pinned = set()

    def resample(self, parents, names=None):
        """The resampling step of a particle filter on the device: member m becomes a copy, bit for bit, of member
        parents[m] in every state vector (lf_members_resample_device; names and what stays untouched: as transform()).
        parents: [members] integers 0 .. members - 1, e.g. assimilation.systematic_parents(); a member that keeps itself is
        not written, with the identity nothing is launched.  At most 128 members.  Ordered like transform()."""
        M = self.members
        p = np.asarray(parents)
        if p.shape != (M,) or p.dtype.kind not in "iu" or p.min() < 0 or p.max() >= M:
            raise ValueError("parents must be [%d] integers from 0 to members - 1 = %d" % (M, M - 1))
        if M > 128:
            raise ValueError("resample() takes at most 128 members (%d)" % M)
        p = np.ascontiguousarray(p, np.int32)
        calls = [row for name in self._analysis_names(names) for row in self._analysis_rows(name) if row[1]]
        L, dev = lib(), self.device
        check(L.lf_side_stream_join(dev))
        for base, n, stride, _, _ in calls:
            check(L.lf_members_resample_device(dev, base, M, stride, n, p.ctypes.data_as(C.c_void_p)))

    def gaps(self, name, buffer_set=None):
        """[members, pad]: the elements between the members' rows of a member vector, which no call reads or writes (the
        last member's gap of a channel vector may lie beyond the vector: NaN here).  A forcing vector: of the set in use,
        or of buffer_set 0 / 1 (waits for an upload into that set)"""
        if buffer_set is not None:
            self.upload_wait(buffer_set)
            rows = self.force[int(buffer_set)][name].download().reshape(self.members, self.pstride)
            return rows[:, self.N:]
        if name in self.land.dev:
            return self.land.gaps(name)
        return self._rows_of(name)[1]

    def gap_names(self):
        """every vector that holds member rows"""
        E = self.land
        dense = [k for k, (_, _, pixels) in self.chan._groups.items() if pixels]      # (site-state rows lie back to back)
        chan = RT._STATE + RT._OUT + dense + list(self._qin) + ["ToChanM3RunoffDt"]
        return E._member + E._forcing + E._pixel + list(dict.fromkeys(chan))

    def set_gaps(self, value):
        """plant `value` between the members' rows of every member vector of every stage"""
        check(lib().lf_device_synchronize(self.device))
        self._gap = float(value)
        self.land.set_gaps(value)
        for d in self.force[1 - self._cur].values():          # (the land surface has planted it in the set in use)
            host = d.download().reshape(self.members, self.pstride)
            host[:, self.N:] = self._gap
            d.upload(host.reshape(-1))
        for name in self.gap_names():
            if name not in self.land.dev:
                self._set_channel_rows(name, self._rows_of(name)[0])
        scratch = self.land.dev["scratch"]
        host = scratch.download().reshape(3 * self.members, self.pstride)
        host[:, self.N:] = self._gap
        scratch.upload(host.reshape(-1))

    # ---- warm start: HotPathDevice's state file with a leading member axis -------------------------------------------------
    def save_state(self, path):
        out = {k: self.download(k) for k in self.state_names()}
        if self.rmod is not None:
            for k in RT._LAKE_STATE + RT._RES_STATE + ["TransCum"]:
                if k in self.chan._groups:
                    out["site_" + k] = self.download_site(k)
        out["steps_done"] = np.int64(self.steps_done)
        if self._qin_old is not None:
            out["qin_old"] = self._qin_old
        np.savez(path, **out)

    def load_state(self, path):
        z = np.load(path)
        self._check_state_file(z.files)
        for k in self.state_names():
            if k not in z.files and k in OPTIONAL_MAPS:
                continue
            self.set_member_state(k, z[k])
        if self.rmod is not None:
            for k in RT._LAKE_STATE + RT._RES_STATE + ["TransCum"]:
                if "site_" + k in z.files:
                    a = z["site_" + k]
                    self._set_channel_rows(k, a[:, self.gpix] if k == "TransCum" else a)
        if "qin_old" in z.files and self._qin_old is not None:
            self._qin_old = np.array(z["qin_old"], np.float64)
        self.steps_done = int(z["steps_done"])

    def free(self):
        check(lib().lf_device_synchronize(self.device))
        self.chan.free()
        self.land.free()
        products = [d for cache in (self._thresholds, self._gauges, self._analysis_cache) for hit in cache.values()
                    for d in hit if isinstance(d, DeviceArray)] + list(self._products.values()) + [self._gpix_dev]
        products += [self._weights[1]] if self._weights else []
        products += [self._regress_table] if self._regress_table else []
        self._regress_table = None
        products += [d for t in self._trackers.values() for d in list(t.dev.values()) + [t.thr]]
        products += [p[0] for p in self._perturbations.values()]
        products += [d for t in self._zonal.values() for d in t.arrays]
        self._perturbations, self._zonal = {}, {}
        self._thresholds, self._gauges, self._products, self._gpix_dev, self._outside_held = {}, {}, {}, None, {}
        self._trackers, self._weights, self._analysis_cache = {}, None, {}
        self._free_shared([self._gidx, self._side, self._pidx] + list(self._qin.values()) +
                          list(self.force[1 - self._cur].values()) + [d for d in products if d is not None])
