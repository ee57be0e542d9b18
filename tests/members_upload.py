"""Helpers of tests/test_members_upload_gpu.py: sources with the special values planted, one lf_upload_rows call between
lf_upload_begin and lf_upload_end, and the chain of hotpath.HotPathEnsemble beside one HotPathDevice per member."""
import ctypes as C

import numpy as np

SENTINEL = -777.25                  # what lies between the rows of a destination before and after a call
FORCING = ("Rain", "SnowMelt", "EWRef", "ETRef", "ESRef")
F32 = np.finfo(np.float32)
SPECIAL = {                         # per source type: values whose widening / copy must be exact
    np.float32: [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, float(F32.tiny) * 0.75, float(F32.tiny), float(F32.max),
                 -float(F32.max), 1.0 + float(F32.eps)],
    np.float64: [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, np.finfo(np.float64).tiny, np.finfo(np.float64).max,
                 -np.finfo(np.float64).max, 1e-45, float(F32.max), 1.0 + np.finfo(np.float64).eps],
}


def same_bits(a, b):
    """float64 arrays equal bit for bit (the sign of a zero counts); a NaN must be a NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def first_difference(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return "shapes %s != %s" % (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~(na | nb) & (a.view(np.uint64) != b.view(np.uint64)))
    if not bad.any():
        return "equal"
    i = tuple(int(x) for x in np.argwhere(bad)[0])
    return "%d differ, first at %s: %r != %r" % (int(bad.sum()), i, float(a[i]), float(b[i]))


def source(rng, src_rows, n, dtype):
    """[src_rows, n] random values of `dtype` with the special values planted (as many as fit, at random places)"""
    with np.errstate(over="ignore"):
        a = (rng.standard_normal((src_rows, n)) * 10.0 ** rng.integers(-30, 30, (src_rows, n))).astype(dtype)
    special = np.array(SPECIAL[dtype], dtype)
    k = min(special.size, a.size)
    first = int(rng.integers(0, special.size))                    # (a source of one element gets another value every time)
    a.reshape(-1)[rng.choice(a.size, k, replace=False)] = np.roll(special, -first)[:k]
    return a


def reference(src, rows, index):
    """what lf_upload_rows leaves in the first n elements of every row: [rows, n] float64"""
    wide = src.astype(np.float64)
    if index is not None:
        wide = wide[..., index]
    return np.broadcast_to(wide, (rows, wide.shape[-1]))


def upload_rows(amd, dst, dst_stride, rows, src, n, index_dev, buffer_set=0, wait=True):
    """one lf_upload_rows of the host array src ([src_rows, n], float32 / float64) inside the protocol of buffer_set"""
    L = amd.lib()
    assert src.flags.c_contiguous and src.dtype in (np.float32, np.float64)
    amd.check(L.lf_upload_begin(0, buffer_set))
    amd.check(L.lf_upload_rows(0, dst.ptr, dst_stride, rows, src.ctypes.data_as(C.c_void_p), src.shape[0],
                               1 if src.dtype == np.float32 else 0, n, None if index_dev is None else index_dev.ptr))
    amd.check(L.lf_upload_end(0, buffer_set))
    if wait:
        amd.check(L.lf_upload_wait(0, buffer_set))


def check_rows(dst, rows, n, dst_stride, want, what):
    """the destination holds `want` in its rows and still the sentinel between them"""
    got = dst.download().reshape(-1)[:rows * dst_stride].reshape(rows, dst_stride)
    assert same_bits(got[:, :n], want), (what, first_difference(got[:, :n], want))
    assert (got[:, n:] == SENTINEL).all(), (what, "padding written")


# ---- the chain ------------------------------------------------------------------------------------------------------------
H, W, MEMBERS, STEPS, PAD = 48, 60, 3, 3, 5
N = H * W
PLANNED = 24                        # structures_scenario seed with which the time-major site plan applies
KINDS = ("float64", "float32", "mixed")


def cp(d):
    return {k: (np.array(a, copy=True) if isinstance(a, np.ndarray) else a) for k, a in d.items()}


def make_scenario():
    from lisflood_amd import synthetic as syn
    values, sc, mask, ldd_to_chan, ldd_kin = syn.hotpath_scenario(H, W)
    st, cut = syn.structures_scenario(ldd_kin, (H, W), values["ChanQ"], sc["DtRouting"], n_lakes=3, n_res=5, seed=PLANNED)
    return values, sc, mask, ldd_to_chan, ldd_kin, st, cut


def build(scenario, cls, structures, **kw):
    values, sc, mask, ldd_to_chan, ldd_kin, st, cut = scenario
    return cls(cp(values), sc, mask, ldd_to_chan, cut if structures else ldd_kin, split=True,
               structures=cp(st) if structures else None, **kw)


def member_forcing(kind, m, s):
    """the forcing of member m at step s as the ensemble's caller holds it, vector by vector: float64 / float32 rows of the
    member, or (mixed) Rain float32 of the member and the other four float64 and the same for every member"""
    from lisflood_amd import synthetic as syn
    f = syn.hotpath_forcing(N, s + 10 * m)
    if kind == "float32":
        return {k: a.astype(np.float32) for k, a in f.items()}
    if kind == "mixed":
        shared = syn.hotpath_forcing(N, s + 1000)
        return dict(shared, Rain=f["Rain"].astype(np.float32))
    return f


def ensemble_forcing(kind, s, members=MEMBERS):
    """-> the dict for HotPathEnsemble.step / prefetch: [members, N] rows; mixed: Rain [members, N] float32, the others [N]"""
    f = [member_forcing(kind, m, s) for m in range(members)]
    rows = {k: np.stack([x[k] for x in f]) for k in FORCING}
    if kind == "mixed":
        rows.update({k: f[0][k] for k in FORCING if k != "Rain"})
    return rows


def member_inflow(st, m, s):
    return st["QInM3Old"] * (1.0 + 0.1 * s + 0.05 * m)


def inflow_rows(scenario, structures, s, members=MEMBERS):
    return np.stack([member_inflow(scenario[5], m, s) for m in range(members)]) if structures else None


def compared(obj):
    """the vectors the chain is compared on: every state vector, the sideflow and the discharge output"""
    out = {k: obj.download(k) for k in obj.state_names() + ["ToChanM3RunoffDt"]}
    out["chan_q_avg"] = obj.chan_q_avg()
    return out


_alone = {}


def alone(scenario, structures, kind):
    """per step, per member: `compared` of that member's own HotPathDevice fed the same arrays by its blocking step; worked
    out once per (structures, kind) and left unchanged"""
    from lisflood_amd.hotpath import HotPathDevice
    key = (bool(structures), kind)
    if key not in _alone:
        out = [[None] * MEMBERS for _ in range(STEPS)]
        for m in range(MEMBERS):
            hp = build(scenario, HotPathDevice, structures)
            for s in range(STEPS):
                hp.step(member_forcing(kind, m, s), time_since_start=s + 1,
                        QInM3=member_inflow(scenario[5], m, s) if structures else None)
                out[s][m] = compared(hp)
            hp.free()
        _alone[key] = out
    return _alone[key]


def assert_members(ens, want, step):
    """want: per member, name -> array"""
    got = compared(ens)
    assert set(got) <= set(want[0]) and len(got) >= 40, sorted(set(got) - set(want[0]))
    for k, rows in got.items():
        assert rows.shape[0] == ens.members and rows.ndim == np.ndim(want[0][k]) + 1, k
        for m in range(ens.members):
            assert same_bits(rows[m], want[m][k]), (step, k, m, first_difference(rows[m], want[m][k]))


def assert_gaps(ens):
    """the sentinel between the rows of every member vector, of both forcing sets"""
    from lisflood_amd.soilloop import GAP_BYTE
    for k in ens.gap_names():
        g = ens.gaps(k)
        assert g.shape == (ens.members, PAD), (k, g.shape)
        if g.dtype == np.uint8:
            assert (g == GAP_BYTE).all(), k
        else:                       # (the last member's gap of a channel vector may lie beyond the vector: NaN)
            assert ((g == SENTINEL) | np.isnan(g)).all() and not np.isnan(g[:-1]).any(), (k, g)
    for b in (0, 1):
        for k in FORCING:
            g = ens.gaps(k, buffer_set=b)
            assert g.shape == (ens.members, PAD) and (g == SENTINEL).all(), (b, k, g)
