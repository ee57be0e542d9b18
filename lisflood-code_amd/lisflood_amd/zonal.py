"""The order of a zonal sum: which elements of a member row go into which zone, and in what order they are added.  Host
only, numpy only.  HotPathEnsemble.zonal() runs the plan on the device (lf_members_zonal_device, one call per pass); the
arithmetic of a run sum is stated in include/lisflood_amd.h and restated here (run_sums) for the plan's own weight sums.

Entries: the (zone, row position) pairs sorted by zone and, within a zone, by ascending row position -- the order in which
the source row lies on the device -- a stable sort, so equal pairs keep the caller's order.  Positions need not be unique
across zones: zones may overlap.
Pass 1 cuts each zone's entries into consecutive runs of at most 256 entries; a run never crosses a zone boundary and a
zone without entries gets one run of length 0.  The values of pass p + 1 are pass p's run sums, one per run, in run order,
and each zone's values are cut into runs of at most 256 again.  The passes end when every zone has exactly one run: run r
of the last pass is zone r.  A zone of 256^2 entries takes 2 passes, one of 256^2 + 1 entries takes 3."""
import numpy as np

RUN = 256          # entries of a run: four per lane of a wavefront
_CHUNK = 1 << 14   # (row, run) pairs padded to RUN at a time in run_sums: 32 MiB


def cut_runs(counts):
    """counts [Z]: values per zone, laid out zone after zone -> (run_start int64 [runs + 1], zone_of_run int64 [runs]):
    max(1, ceil(count / 256)) runs per zone, all but a zone's last one full"""
    counts = np.asarray(counts, np.int64)
    Z = counts.size
    runs = np.maximum(1, -(-counts // RUN))
    zone_of_run = np.repeat(np.arange(Z, dtype=np.int64), runs)
    first_value = np.concatenate([[0], np.cumsum(counts)])
    first_run = np.concatenate([[0], np.cumsum(runs)])
    within = np.arange(zone_of_run.size, dtype=np.int64) - first_run[zone_of_run]
    run_start = np.concatenate([first_value[zone_of_run] + RUN * within, first_value[-1:]])
    return run_start, zone_of_run


def run_sums(values, run_start):
    """values [..., E], run_start [runs + 1] -> [..., runs]: the run sum of lf_members_zonal_device -- the run padded to 256
    with +0.0, lane l of 64 adds v[l], v[l + 64], v[l + 128], v[l + 192] to 0.0 in that order, then s[l] = s[l] + s[l + d]
    for d = 32 .. 1"""
    values = np.asarray(values, np.float64)
    run_start = np.asarray(run_start, np.int64)
    runs, E = run_start.size - 1, values.shape[-1]
    out = np.zeros(values.shape[:-1] + (runs,))
    lane = np.arange(RUN, dtype=np.int64)
    chunk = max(1, _CHUNK // max(1, int(np.prod(values.shape[:-1]))))
    with np.errstate(all="ignore"):
        for r0 in range(0, runs, chunk):
            r1 = min(runs, r0 + chunk)
            at = run_start[r0:r1, None] + lane[None, :]
            on = at < run_start[r0 + 1:r1 + 1, None]
            v = np.where(on, values[..., np.where(on, at, 0)], 0.0) if E else np.zeros(values.shape[:-1] + on.shape)
            v = v.reshape(v.shape[:-1] + (RUN // 64, 64))
            s = np.zeros(v.shape[:-2] + (64,))
            for k in range(RUN // 64):
                s = s + v[..., k, :]
            d = 32
            while d >= 1:
                s = s[..., :d] + s[..., d:2 * d]
                d //= 2
            out[..., r0:r1] = s[..., 0]
    return out


class ZonePlan:
    """ZonePlan(zone_of_entry, position_of_entry, zones, pixel_of_position=None, weight_of_entry=None): the plan of the
    (zone, row position) pairs given, zones 0 .. zones - 1.  pixel_of_position: row position -> compressed land index
    (None: the position itself);  weight_of_entry: the weight of every pair, in the order of the pairs.
        entries, zones   their numbers
        zone_of_entry    int32 [entries], in summation order (ascending)
        positions        int32 [entries]: the row position of every entry -- the index table of pass 1
        pixels           int64 [entries]: the compressed land index of every entry
        weights          float64 [entries] or None
        passes           their number;  run_start[p] int32 [runs_p + 1] and zone_of_run[p] int32 [runs_p] of pass p
        weight_sum       float64 [zones]: the same sum over the weights -- without weights over 1.0 per entry, which is the
                         zone's number of entries whatever the order"""

    def __init__(self, zone_of_entry, position_of_entry, zones, pixel_of_position=None, weight_of_entry=None):
        zone = np.asarray(zone_of_entry, np.int64).reshape(-1)
        pos = np.asarray(position_of_entry, np.int64).reshape(-1)
        Z = int(zones)
        if zone.shape != pos.shape:
            raise ValueError("zone_of_entry and position_of_entry must have one length")
        if Z < 0 or zone.size and (zone.min() < 0 or zone.max() >= Z):
            raise ValueError("zones of the entries must lie in 0 .. zones - 1 = %d" % (Z - 1))
        if pos.size and pos.min() < 0:
            raise ValueError("row positions must not be negative")
        if pos.size > 0x7fffffff or pos.size and pos.max() > 0x7fffffff:
            raise ValueError("entries and row positions must stay inside the 32-bit range of a launch")
        order = np.lexsort((pos, zone))                      # (stable: equal pairs keep their order)
        self.zones, self.entries = Z, int(zone.size)
        self.zone_of_entry = zone[order].astype(np.int32)
        self.positions = pos[order].astype(np.int32)
        self.pixels = pos[order] if pixel_of_position is None else np.asarray(pixel_of_position, np.int64)[pos[order]]
        self.weights = None
        if weight_of_entry is not None:
            w = np.asarray(weight_of_entry, np.float64).reshape(-1)
            if w.shape != zone.shape:
                raise ValueError("weight_of_entry must have the length of the entries")
            self.weights = np.ascontiguousarray(w[order])
        self.run_start, self.zone_of_run = [], []
        counts = np.bincount(zone, minlength=Z).astype(np.int64)
        while True:
            start, zr = cut_runs(counts)
            self.run_start.append(start.astype(np.int32))
            self.zone_of_run.append(zr.astype(np.int32))
            counts = np.bincount(zr, minlength=Z).astype(np.int64)
            if zr.size == Z:                                 # every zone one run: run r is zone r
                break
        self.passes = len(self.run_start)
        self.weight_sum = np.bincount(zone, minlength=Z).astype(np.float64) if self.weights is None else self.sums(self.weights)

    def runs(self, p):
        """the number of runs of pass p (0-based)"""
        return int(self.zone_of_run[p].size)

    def sums(self, values):
        """values [..., entries] in summation order (already divided and weighted) -> [..., zones]: every pass on the host"""
        for start in self.run_start:
            values = run_sums(values, start)
        return values


def zone_pairs(zones, n):
    """The two forms HotPathEnsemble.zonal() takes -> (zone of every pair, compressed land index of every pair, Z):
    an int label map [n] in pixel order, labels 0 .. Z - 1 with Z = the largest label + 1, negative: no zone;  or a sequence
    of Z arrays of compressed land indices, which may overlap"""
    if isinstance(zones, np.ndarray) and zones.ndim == 1 and zones.dtype != object:
        if zones.shape != (n,) or zones.dtype.kind not in "iu":
            raise ValueError("a label map must be an integer array [%d] in pixel order" % n)
        pix = np.flatnonzero(zones >= 0)
        zone = zones[pix].astype(np.int64)
        return zone, pix, int(zone.max()) + 1 if zone.size else 0
    lists = [np.asarray(z, np.int64).reshape(-1) for z in zones]
    pix = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    if pix.size and (pix.min() < 0 or pix.max() >= n):
        raise ValueError("zone pixels must be compressed land indices 0 .. %d" % (n - 1))
    return np.repeat(np.arange(len(lists), dtype=np.int64), [z.size for z in lists]), pix, len(lists)


def row_plan(zones, weights, n, pixel_of_position, row_of_pixel=None):
    """The plan of HotPathEnsemble.zonal() on rows whose position p holds land pixel pixel_of_position[p] of n: zones and
    weights ([n] in pixel order, or None) as zonal() takes them.  A pixel the rows do not hold (a channel row's pixels
    outside the channel domain) is in no zone, and in no weight sum.  row_of_pixel: the inverse table, -1 outside, where
    the caller has it already."""
    pixel_of_position = np.asarray(pixel_of_position, np.int64)
    if row_of_pixel is None:
        row_of_pixel = np.full(n, -1, np.int64)
        row_of_pixel[pixel_of_position] = np.arange(pixel_of_position.size)
    zone, pix, Z = zone_pairs(zones, n)
    w = None
    if weights is not None:
        w = np.asarray(weights, np.float64)
        if w.shape != (n,):
            raise ValueError("weights must be [%d] in pixel order" % n)
    row = row_of_pixel[pix]
    inside = row >= 0
    return ZonePlan(zone[inside], row[inside], Z, pixel_of_position, None if w is None else w[pix[inside]])
