"""-m gpu: the wide levels of an ordered beta = 3/5 call take a cell's upstream range from one count byte per cell and one
table entry per wavefront (k_level<.., STATICS = 2>, csrc/lf_sweep.h) instead of two ups_ptr entries per cell.  That is an
encoding of the graph, not arithmetic: LF_LEVEL_COUNTS=1 against 0 bit for bit, the oracle at the routing tolerance of
test_gpu_parity.py (rtol 1e-9 / atol 1e-12), and the shapes at which the range arithmetic can go wrong shown to be in the
rasters."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-12
H, W = 420, 380
N = H * W
# what makes levels of this small raster wide levels (k_level), and the size above which a level certainly is one: above
# 2000 cells among the level blocks, or above 1024 with one launch per level
CASES = {"shallow": ({"LF_FUSED_WIDE": "2000"}, 2000), "river": ({"LF_ROUTE_CONES": "0"}, 1024)}
CALLS = 4

_inputs, _results = {}, {}


@pytest.fixture(scope="module")
def amd():
    from lisflood_amd import _lib
    if _lib.device_count() == 0:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X box")
    assert _lib.device_name(0).startswith("gfx950"), _lib.device_name(0)
    return _lib


def inputs(family):
    """raster, a router with floodplains and per-pixel channel lengths, lateral inflow of four calls (built once)"""
    if family not in _inputs:
        from lisflood_amd import synthetic as syn
        p = syn.router_params(N, seed=8)
        alpha2 = p["alpha"] * np.random.default_rng(3).uniform(1.2, 2.0, N)
        _inputs[family] = (syn.make_ldd(family, H, W, 5), p, alpha2, [syn.lateral_inflow(N, i) for i in range(CALLS)])
    return _inputs[family]


def routed(family, monkeypatch, counts, statics="1"):
    """both sections after four ordered calls, pixel order, and the wide launches of a call (computed once per setting)"""
    key = (family, counts, statics)
    if key in _results:
        return _results[key]
    from lisflood_amd import _lib
    from lisflood_amd.kinematic_wave_parallel import Graph, kinematicWave
    codes, p, alpha2, lat = inputs(family)
    for k, v in CASES[family][0].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("LF_LEVEL_COUNTS", counts)
    monkeypatch.setenv("LF_LEVEL_STATICS", statics)
    g = Graph(ldd_raster=codes)
    kw = kinematicWave(None, None, p["alpha"], p["beta"], p["dx"], p["dt"], alpha_floodplains=alpha2, graph=g)
    tmp = _lib.DeviceArray(N)
    out, wide = [], 0
    for section in ("main_channel", "floodplains"):
        Q = _lib.DeviceArray.from_host(p["Q0"])
        kw.to_engine_order(Q, tmp); Q.copy_from(tmp)
        for i in range(CALLS):
            q = _lib.DeviceArray.from_host(lat[i])
            kw.to_engine_order(q, tmp); q.copy_from(tmp)
            kw.route_ordered(Q, q, section)
            q.free()
        wide = kw.last_launches()["wide"]
        kw.from_engine_order(Q, tmp)
        out.append(tmp.download().copy())
        Q.free()
    tmp.free(); kw.close()
    _results[key] = (out, wide)
    return _results[key]


def range_edge_cases(codes, wide_min):
    """Which shapes the levels of more than wide_min cells have, from the layout alone.  A wavefront is a group of 64
    consecutive cells of a level counted from the level's first cell; its cells' upstream runs follow one another, the first
    one at ups_ptr of the group's first cell."""
    from lisflood_amd.kinematic_wave_parallel import Graph
    g = Graph(ldd_raster=codes)
    _, ups_ptr, level_start = g.layout()
    g.close()
    cnt = np.diff(ups_ptr.astype(np.int64))
    assert cnt.min() >= 0 and cnt.max() <= 8               # a count fits four bits
    have = dict(not_64=0, not_256=0, start_off_64=0, eight=0, all_sources=0, straddle=0, tail=0)
    for k in range(len(level_start) - 1):
        first, n = int(level_start[k]), int(level_start[k + 1] - level_start[k])
        if n <= wide_min:
            continue
        have["not_64"] += n % 64 != 0
        have["not_256"] += n % 256 != 0
        have["start_off_64"] += first % 64 != 0
        c = np.zeros((n + 63) // 64 * 64, np.int64)
        c[:n] = cnt[first:first + n]
        c = c.reshape(-1, 64)
        # the encoding itself: group start + counts of the lanes below = ups_ptr of every cell of the level
        start = ups_ptr[first:first + n:64].astype(np.int64)
        u0 = (start[:, None] + np.cumsum(c, axis=1) - c).reshape(-1)[:n]
        assert np.array_equal(u0, ups_ptr[first:first + n]) and np.array_equal(u0 + c.reshape(-1)[:n], ups_ptr[first + 1:first + n + 1])
        have["eight"] += int((c == 8).sum())
        have["all_sources"] += int((c[:n // 64].sum(axis=1) == 0).sum())   # (full wavefronts only)
        # a run ends at the boundary and the next wavefront starts with one: lane 63 and the next lane 0 both have upstream
        # cells, so the next group's start is this group's start plus all 64 counts, the last one included
        have["straddle"] += int(((c[:-1, 63] > 0) & (c[1:, 0] > 0)).sum())
        have["tail"] += int(n % 64 != 0 and c[-1].sum() > 0)
    return have


@pytest.mark.parametrize("family", ["shallow", "river"])
def test_count_bytes_of_the_wide_levels_leave_the_bits_alone(amd, oracle, monkeypatch, family):
    """Both sections of a router with floodplains and per-pixel channel lengths, four calls: with the count bytes and with
    ups_ptr (LF_LEVEL_COUNTS=1 / 0) bit for bit, and the oracle."""
    codes, p, alpha2, lat = inputs(family)
    (m1, f1), wide = routed(family, monkeypatch, "1")
    assert wide >= 1, wide                                # the case is about the wide levels
    (m0, f0), _ = routed(family, monkeypatch, "0")
    assert np.array_equal(m1, m0) and np.array_equal(f1, f0)
    assert np.isfinite(m1).all() and m1.max() > 0
    cpu = oracle.kinematicWave(codes.reshape(-1).astype(np.float64), np.ones((H, W), bool), p["alpha"], p["beta"], p["dx"],
                               p["dt"], alpha_floodplains=alpha2)
    for got, section in ((m1, "main_channel"), (f1, "floodplains")):
        Q = p["Q0"].copy()
        for i in range(CALLS):
            cpu.kinematicWaveRouting(Q, lat[i], section)
        np.testing.assert_allclose(got, Q, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=str((family, section)))


def test_the_rasters_hold_the_shapes_where_the_range_arithmetic_can_go_wrong(amd):
    """The wide levels of the two rasters of the bit-identity test, from Graph.layout(): sizes that are no multiple of 64
    and of 256, a level that does not start at a multiple of 64, a cell with 8 upstream cells (shallow), a wavefront of 64
    sources, a run that ends at a wavefront's last lane with the next wavefront starting on a run, and a last, partial
    wavefront with non-source cells."""
    for family, (_, wide_min) in CASES.items():
        have = range_edge_cases(inputs(family)[0], wide_min)
        for shape, count in have.items():
            if shape == "eight" and family == "river":     # (its confluences are narrow levels)
                continue
            assert count >= 1, (family, shape, have)


def test_without_the_records_the_count_bytes_are_not_used(amd, monkeypatch):
    """LF_LEVEL_STATICS=0 sends the wide levels to the kernel of the separate streams whatever LF_LEVEL_COUNTS says: the
    same bits as with the records and with the count bytes."""
    (m, f), wide = routed("shallow", monkeypatch, "1", statics="0")
    assert wide >= 1, wide
    (m1, f1), _ = routed("shallow", monkeypatch, "1")
    (m0, f0), _ = routed("shallow", monkeypatch, "0")
    assert np.array_equal(m, m1) and np.array_equal(f, f1)
    assert np.array_equal(m, m0) and np.array_equal(f, f0)
