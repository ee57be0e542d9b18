"""Inputs that put cells on both sides -- and on the ties -- of every comparison of one routing.dynamic() sub-step
(routing.py:512-603, 693-703), a census that shows it from the values alone, a guard for the one materially discontinuous
branch, and a numpy restatement of the element-wise lines around the two router calls.  A plain helper module:
tests/test_substep_edges_cpu.py pins the C oracle to the restatement bit for bit, tests/test_substep_edges_gpu.py runs the
same inputs through every copy of the arithmetic on the device (the stage kernels of lf_routing_substep and the four fused
forms).

The raster is 96 x 80, all land, in two LDD families of synthetic.make_ldd: "deep" (98 levels of ~80 cells: level blocks of
8 levels, so the cone kernels run) and "shallow" (a handful of wide levels: the time-major kernel and, with level blocks
switched off, the level kernel).  Random fill as synthetic.model_step_values (the discharge capped, see substep_inputs); the
edge cases sit on planted cells -- one near the front of the raster and its mirror near the end (module_edges.spots).  The
isolated ones all lie in the last level of the engine's layout, whose last workgroup is a partial one that carries some of
them (tests/test_substep_edges_cpu.py); the others lie where their distance to a pit puts them.  The LDD around a planted
cell is only ever CUT (cells made pits), never
redirected, so it stays acyclic: "source" cells lose their upstream cells (their router constant is then known), "isolated"
cells lose their downstream link too (they sit in the last level with the pits), "connected" cells are chosen where the
graph gives them both.

Planted ties are exact in the inputs themselves: the routing time step is 4096 s and the planted reaches are 2048 m long, so
SideflowChanM3 * InvChanLength * InvDtRouting is a scaling by 2^-23, and the volumes are powers of two and binary fractions.
None depends on the result of a pow.

Every planted cell that carries water has a router constant c of at least 0.01: the reference's Newton iteration stops at
|q + a q^beta - c| <= 1e-12, which leaves q undetermined by up to 1e-12 / (beta c) relative -- below the suite's rtol of
1e-9 only for c >= 2e-3.
"""
import math

import numpy as np

from module_edges import same_bits, spots

H, W = 96, 80
N = H * W
DT = 4096.0                       # routing time step [s]: InvDtRouting = 2^-12
NSTEPS = 5
BETA = 0.6
LEN = 2048.0                      # length of a planted reach [m]: InvChanLength = 2^-11
FAMILIES = ("deep", "shallow")
STATE = "ChanQKin ChanM3Kin Chan2QKin Chan2M3Kin CrossSection2Area Sideflow1Chan ChanQ sumDisDay".split()
STATIC = ("ChanLength InvChanLength ChannelAlpha InvChannelAlpha ChannelAlpha2 InvChannelAlpha2 Chan2M3Start Chan2QStart "
          "M3Limit QLimit PixelArea IsChannelKinematic").split()
OUT = "FlowVelocity TravelDistance".split()
INERT_TESTED = "ChanQKin ChanM3Kin ChanQ Chan2QKin Chan2M3Kin CrossSection2Area Sideflow1Chan".split()  # fused_cell's test
SIDE_TIE = 1e-7
RTOL, ATOL = 1e-9, 1e-12          # device against oracle: the routing tolerance of test_gpu_parity.py
HUGE_Q = 2.0 ** 170               # a discharge whose router constant a q^0.6 (~2^101) is beyond lf_fast_range (1e30)
_SHIFT = {2: (1, 0), 3: (1, 1), 6: (0, 1), 9: (-1, 1), 8: (-1, 0), 7: (-1, -1), 4: (0, -1), 1: (1, -1)}  # synthetic.IX_ADDS


def downstream(codes):
    """[N] pixel id a cell drains into (-1: pit) of an [H, W] raster of keypad codes"""
    down = np.full(codes.size, -1, np.int64)
    for code, (dr, dc) in _SHIFT.items():
        r, c = np.nonzero(codes == code)
        down[r * codes.shape[1] + c] = (r + dr) * codes.shape[1] + (c + dc)
    return down


class _Planter:
    """places the planted cells (at least three cells apart) and cuts the LDD around them"""

    def __init__(self, codes):
        self.codes, self.blocked = codes, np.zeros(codes.shape, bool)
        self.cells = {}

    def _ups(self, p):
        r, c = divmod(p, W)
        out = []
        for code, (dr, dc) in _SHIFT.items():
            rr, cc = r - dr, c - dc
            if 0 <= rr < H and 0 <= cc < W and self.codes[rr, cc] == code:
                out.append(rr * W + cc)
        return out

    def _down(self, p):
        r, c = divmod(p, W)
        code = int(self.codes[r, c])
        if code == 5:
            return -1
        dr, dc = _SHIFT[code]
        return (r + dr) * W + (c + dc)

    def _free(self, p):
        r, c = divmod(p, W)
        return 2 <= r < H - 2 and 2 <= c < W - 2 and not self.blocked[r, c]

    def _block(self, p):
        r, c = divmod(p, W)
        self.blocked[max(r - 2, 0):r + 3, max(c - 2, 0):c + 3] = True

    def _cut_ups(self, p):
        for u in self._ups(p):
            self.codes[divmod(u, W)] = 5

    def place(self, name, k, kind):
        """the two cells of planted case `name` (nominal places: spots(k)), -> [front cell, mirror cell]"""
        base = 3 * W + 2
        got = []
        for nominal, step in zip(spots(k, N - 2 * base, 7), (1, -1)):
            p = base + nominal
            while True:
                ok = self._free(p)
                if ok and kind == "connected":
                    ok = self._down(p) >= 0 and len(self._ups(p)) > 0
                if ok and kind == "pair":          # p drains into d; d becomes a pit fed by p alone
                    d = self._down(p)
                    ok = d >= 0 and self._free(d)
                if ok:
                    break
                p += step
            if kind in ("source", "isolated", "pair"):
                self._cut_ups(p)
            if kind == "isolated":
                self.codes[divmod(p, W)] = 5
            if kind == "pair":
                d = self._down(p)
                self.codes[divmod(d, W)] = 5
                for u in self._ups(d):
                    if u != p:
                        self.codes[divmod(u, W)] = 5
                self._block(d)
            self._block(p)
            got.append(p)
        self.cells[name] = got
        return got


def _q_of(m3, alpha, length=LEN):
    return (m3 / (length * alpha)) ** (1 / BETA)


def substep_inputs(split, seed, family="deep"):
    """-> dict: `codes` [H, W] and `mask` of the all-land raster, `vals` (the lf_substep_args vectors in pixel order,
    statics and initial state, regular statics), `irregular` (the vectors that replace theirs in the irregular set),
    `sideflows` [NSTEPS, N] SideflowChanM3 (the planted sideflows in every sub-step), `staggered` [NSTEPS, N] (cases d, g and
    n in sub-steps 1, 2 and 3 only), `cells` (case -> its two pixels), the scalars.  `split` only goes into the dict: the
    inputs of single and split routing are the same."""
    from lisflood_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    codes = syn.make_ldd(family, H, W, seed).astype(np.uint8)
    P = _Planter(codes)
    p = syn.router_params(N, seed=seed + 1)
    # QLimit = 2 Q0 U(0.3, 1.2) stays below 1000: ChanQ = ChanQKin + Chan2QKin - QLimit, and a floodplain at its threshold volume
    # has Chan2QKin == QLimit up to the last ulps of two pows (~4 ulp, 9e-16 QLimit), which must stay below the atol of
    # 1e-12 where the main channel has run nearly dry (substep_conditioning counts the cells where it would not)
    p["Q0"] = np.minimum(p["Q0"], 400.0)
    v, _ = syn.model_step_values(N, p, seed=seed + 2)
    v = {k: np.array(a, copy=True) for k, a in v.items()}
    del v["SideflowChanM3"]
    for k in ("CrossSection2Area", "Sideflow1Chan", "ChanQ", "sumDisDay"):
        v[k] = np.zeros(N)
    v["sumDisDay"] = rng.uniform(0.0, 3.0, N)
    side = np.stack([syn.lateral_inflow(N, 50 * seed + s) for s in range(NSTEPS)])        # per metre of reach
    staggered_plain = {}
    k_next = [0]
    nan_cells, inert_cells = [], {}

    def plant(name, kind="source", chan=True, side_m=1e-4, stagger=None, **kw):
        """plain column: a reach of 2048 m, alpha 1 / 2, discharge 1, above the M3Limit test (2048 + 512 - 512 > 1024)"""
        col = dict(ChanLength=LEN, ChannelAlpha=1.0, ChannelAlpha2=2.0, PixelArea=2.0 ** 24, ChanQKin=1.0, ChanM3Kin=2048.0,
                   QLimit=0.5, M3Limit=1024.0, Chan2M3Start=512.0, Chan2QStart=2.0 ** -4, Chan2M3Kin=512.0,
                   CrossSection2Area=0.0, Sideflow1Chan=0.0, ChanQ=0.0, sumDisDay=0.0)
        col.update(kw)
        if "Chan2QKin" not in col:
            col["Chan2QKin"] = _q_of(col["Chan2M3Kin"], col["ChannelAlpha2"], col["ChanLength"]) if col["Chan2M3Kin"] > 0 else 0.0
        cells = P.place(name, k_next[0], kind)
        k_next[0] += 1
        for c in cells:
            for key, x in col.items():
                v[key][c] = x
            v["IsChannelKinematic"][c] = chan
            side[:, c] = side_m
            if stagger is not None:
                staggered_plain[c] = (stagger, side_m)
        return cells

    zero = dict(ChanQKin=0.0, ChanM3Kin=0.0, Chan2QKin=0.0, Chan2M3Kin=0.0)
    inert = dict(zero, QLimit=0.0, Chan2QStart=0.0, Chan2M3Start=0.0, M3Limit=1.0)   # (M3Limit is not part of the inert test)
    # a
    plant("a", "connected", chan=False)
    # b
    inert_cells["plus"] = plant("b_plus", "isolated", chan=False, **inert)
    inert_cells["minus"] = plant("b_minus", "isolated", chan=False, **dict(inert, **{k: -0.0 for k in INERT_TESTED}))
    for k in ("ChanQKin", "ChanM3Kin", "ChanQ", "Chan2QKin", "Chan2M3Kin", "CrossSection2Area", "Sideflow1Chan"):
        inert_cells[k] = plant("b_" + k, "isolated", chan=False, **dict(inert, **{k: 0.25}))
    # c
    plant("c_QLimit", "isolated", chan=False, **dict(inert, QLimit=0.5))
    plant("c_Chan2QStart", "isolated", chan=False, **dict(inert, Chan2QStart=2.0 ** -4))
    plant("c_Chan2M3Start", "isolated", chan=False, **dict(inert, Chan2M3Start=512.0, Chan2M3Kin=512.0))
    # d (on plain columns: above the M3Limit test, ratio = 0.8)
    plant("d_plus", side_m=9.9e-8, stagger=1)
    plant("d_minus", side_m=-9.9e-8, stagger=1)
    plant("d_tie", side_m=SIDE_TIE, stagger=1)
    plant("d_below", side_m=float(np.nextafter(SIDE_TIE, 0.0)), stagger=1)
    # e: start = 2^8, M3Limit = 2^9, Chan2M3Kin = 2^8; tot lies in [512, 1024) where 2^-43 is one ulp
    e = dict(Chan2M3Start=256.0, M3Limit=512.0, Chan2M3Kin=256.0)
    plant("e_below", ChanM3Kin=448.0, ChanQKin=_q_of(448.0, 1.0), **e)
    plant("e_tie", ChanM3Kin=512.0, ChanQKin=_q_of(512.0, 1.0), **e)
    plant("e_above", ChanM3Kin=512.0 + 2.0 ** -43, ChanQKin=_q_of(512.0, 1.0), **e)
    # f
    plant("f_tot0", **dict(zero, Chan2M3Start=-2.0, M3Limit=1.0))
    plant("f_m3_0", ChanQKin=0.0, ChanM3Kin=0.0, M3Limit=-1.0)
    # g
    plant("g_main", side_m=-1e-3, stagger=2)
    plant("g_flood", side_m=-1e-3, stagger=2, ChanM3Kin=1.0, Chan2M3Kin=4096.0)
    plant("g_tiny", side_m=2.0 ** -62, ChanQKin=0.0, ChanM3Kin=0.0)
    # h
    plant("h_huge", "isolated", ChanQKin=HUGE_Q, ChanM3Kin=2.0 ** 113)
    plant("h_pow", "isolated", ChanQKin=1e31, ChanM3Kin=2048.0 * 1e31 ** BETA)
    # i
    plant("i_clamp", side_m=2e-5, Chan2QKin=0.0)
    plant("i_start0", Chan2M3Start=0.0)
    # j
    plant("j_clamp", QLimit=1024.0)
    plant("j_zero", QLimit=0.0)
    # k: 64 m3 over 8192 m; no sideflow, so the reach drains and stays below 0.01 m2 to the last sub-step
    plant("k_small", side_m=0.0, ChanLength=8192.0, ChannelAlpha=0.5, ChannelAlpha2=1.0, ChanM3Kin=64.0, ChanQKin=2.0 ** -10)
    # l
    plant("l_below", PixelArea=2.0 ** 20)
    plant("l_tie", PixelArea=2.0 ** 22)
    plant("l_above", PixelArea=2.0 ** 24)
    # m
    plant("m_pow", ChannelAlpha=0.25, ChannelAlpha2=0.5, ChanM3Kin=512.0)
    plant("m_ratio", ChannelAlpha=16.0, ChannelAlpha2=32.0, ChanM3Kin=32768.0, M3Limit=2.0 ** 16)
    # n
    nan_cells += plant("n_pit", "isolated", side_m=np.nan, stagger=3)
    nan_cells += plant("n_upstream", "pair", side_m=np.nan, stagger=3)
    # the irregular statics: ChannelAlpha = 0 on isolated non-channel cells, one InvChanLength off by an ulp
    alpha0 = plant("irr_alpha0", "isolated", chan=False, **inert) + plant("irr_alpha0b", "isolated", chan=False, **inert)
    off = plant("irr_len", "connected", ChanLength=3000.0)[0]

    for k, inv in (("ChanLength", "InvChanLength"), ("ChannelAlpha", "InvChannelAlpha"), ("ChannelAlpha2", "InvChannelAlpha2")):
        v[inv] = 1.0 / v[k]
    irregular = dict(ChannelAlpha=v["ChannelAlpha"].copy(), InvChanLength=v["InvChanLength"].copy())
    irregular["ChannelAlpha"][alpha0] = 0.0
    with np.errstate(divide="ignore"):
        irregular["InvChannelAlpha"] = 1.0 / irregular["ChannelAlpha"]
    irregular["InvChanLength"][off] = np.nextafter(v["InvChanLength"][off], 1.0)
    sideflows = side * (v["ChanLength"] * DT)[None, :]
    stag = side.copy()
    for c, (s, x) in staggered_plain.items():
        stag[:, c] = 1e-4
        stag[s, c] = x
    staggered = stag * (v["ChanLength"] * DT)[None, :]
    down = downstream(codes)
    has_ups = np.bincount(down[down >= 0], minlength=N) > 0
    return dict(family=family, seed=seed, split=bool(split), codes=codes, mask=np.ones((H, W), bool), vals=v, irregular=irregular,
                sideflows=sideflows, staggered=staggered, cells=dict(P.cells), nan_cells=sorted(nan_cells), inert_cells=inert_cells,
                down=down, has_ups=has_ups, isolated=~has_ups & (down < 0), Beta=BETA, DtRouting=DT, NoRoutSteps=NSTEPS,
                irregular_cells=dict(alpha0=alpha0, length=off))


def statics(d, irregular=False):
    """the vectors of the call (statics and initial state, pixel order) with the regular or the irregular statics"""
    v = {k: a.copy() for k, a in d["vals"].items()}
    if irregular:
        v.update({k: a.copy() for k, a in d["irregular"].items()})
    return v


def derived_relations(v, a1, a2, dt=DT):
    """the five relations of k_check_derived (lf_fused.h), cell by cell, with its expressions.  a1 / a2: the router's own
    alpha dx / dt of the main channel / the floodplains (kinematic_wave_parallel.py:127), the router built with
    alpha = ChannelAlpha(2), dx = ChanLength and this dt -> name -> [N] bool"""
    bits = lambda a, b: np.ascontiguousarray(a, np.float64).view(np.uint64) == np.ascontiguousarray(b, np.float64).view(np.uint64)
    with np.errstate(divide="ignore"):
        return {"InvChanLength": bits(v["InvChanLength"], 1.0 / v["ChanLength"]),
                "InvChannelAlpha": bits(v["InvChannelAlpha"], 1.0 / v["ChannelAlpha"]),
                "a1": bits(a1, v["ChannelAlpha"] * v["ChanLength"] / dt),
                "InvChannelAlpha2": bits(v["InvChannelAlpha2"], 1.0 / v["ChannelAlpha2"]),
                "a2": bits(a2, v["ChannelAlpha2"] * v["ChanLength"] / dt)}


# ----------------------------------------------------------------------------------------------------------------------
def _pow_each(x, y):
    """libm pow element by element, as the oracle calls it (numpy's SIMD loops differ by a few ulp)"""
    out = np.empty(x.shape)
    for i, xi in enumerate(x):
        try:
            out[i] = math.pow(xi, y)
        except OverflowError:
            out[i] = math.inf
        except ValueError:
            out[i] = math.nan
    return out


def substep_reference(d, state, side, split, qr1, qr2=None):
    """One routing.dynamic() sub-step restated around the two router calls.  d: statics by name plus Beta, InvDtRouting,
    DtSec; state: the vectors of STATE at the start of the sub-step; side: SideflowChanM3; qr1 / qr2: what the main-channel /
    floodplain router call returns.  -> (new state + FlowVelocity + TravelDistance, intermediates for the census).  The
    sideflows handed to the router calls are mid['s1'] and mid['s2']."""
    beta, inv_beta = d["Beta"], 1.0 / d["Beta"]
    length, inv_len = d["ChanLength"], d["InvChanLength"]
    is_chan = np.asarray(d["IsChannelKinematic"]).astype(bool)
    o = {k: np.array(a, copy=True) for k, a in state.items()}
    with np.errstate(all="ignore"):
        side_ch = np.where(is_chan, side * inv_len * d["InvDtRouting"], 0.0)                  # :512
        mid = dict(split=bool(split), is_chan=is_chan, side_m3=side, side=side_ch)
        if not split:
            s1 = np.where(np.isnan(side_ch), 0.0, side_ch)                                    # :524
            s2 = None
        else:
            m3, m3_2, start, limit = state["ChanM3Kin"], state["Chan2M3Kin"], d["Chan2M3Start"], d["M3Limit"]
            tot = m3 + m3_2
            ratio = np.where(tot > 0, m3 / tot, 0.0)                                          # :549
            s1 = np.where((tot - start) > limit, ratio * side_ch, side_ch)                    # :557
            s1 = np.where(np.abs(side_ch) < 1e-7, side_ch, s1)                                # :563
            s2 = (side_ch - s1) + d["Chan2QStart"] * inv_len                                  # :565-567
            o["Sideflow1Chan"] = s1
            mid.update(tot=tot, m3=m3, start=start, limit=limit, excess=tot - start)
        # main channel, :527-532 / 574-578
        vol = np.maximum(length * d["ChannelAlpha"] * _pow_each(qr1, beta), 0.0)
        q = _pow_each(vol * inv_len * d["InvChannelAlpha"], inv_beta)
        o["ChanM3Kin"], o["ChanQKin"] = vol, q
        if not split:
            o["ChanQ"] = q.copy()
        else:                                                                                 # :584-597
            raw2 = length * d["ChannelAlpha2"] * _pow_each(qr2, beta)
            vol2 = np.where((raw2 - start) < 0.0, start, raw2)
            q2 = _pow_each(vol2 * inv_len * d["InvChannelAlpha2"], inv_beta)
            qsum = q + q2 - d["QLimit"]
            o["Chan2M3Kin"], o["Chan2QKin"] = vol2, q2
            o["CrossSection2Area"] = (vol2 - start) * inv_len
            o["ChanQ"] = np.where((qsum > 0.0) | np.isnan(qsum), qsum, 0.0)
            mid.update(below_start=raw2 - start, qsum=qsum, qlimit=d["QLimit"])
        o["sumDisDay"] = state["sumDisDay"] + o["ChanQ"]
        # velocity, :693-703
        area_raw = vol * inv_len
        area = np.where(area_raw < 0.01, 0.01, area_raw)
        v1, v2 = q / area, 0.36 * _pow_each(q, 0.24)
        vel = np.where(v2 < v1, v2, v1)
        vel = np.where(np.isnan(v2), v2, vel)
        sinu_raw = np.sqrt(d["PixelArea"]) * inv_len
        vel = vel * np.where(sinu_raw > 1, 1.0, sinu_raw)
        o["FlowVelocity"], o["TravelDistance"] = vel, vel * d["DtSec"]
    mid.update(s1=s1, s2=s2, qr1=qr1, qr2=qr2, area_raw=area_raw, v1=v1, v2=v2, sinu_raw=sinu_raw, q=q,
               state_before={k: state[k] for k in INERT_TESTED})
    return o, mid


def substep_census(mid):
    """how many cells of one sub-step take each side and each tie of the sub-step's comparisons.  mid: substep_reference's
    intermediates, with the graph's `isolated` / `has_ups` / `pit_below` masks and the router constants c1 (and c2) that
    oracle_run adds."""
    m = mid
    n = lambda x: int(np.count_nonzero(x))
    chan, side, iso = m["is_chan"], m["side"], m["isolated"]
    before = m["state_before"]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    all_plus = np.logical_and.reduce([bits(before[k]) == 0 for k in INERT_TESTED])
    all_minus = np.logical_and.reduce([bits(before[k]) == bits(np.float64(-0.0)) for k in INERT_TESTED])
    nonzero = sum((before[k] != 0).astype(int) for k in INERT_TESTED)
    c = {
        "a: connected non-channel cell with sideflow": n(~chan & ~iso & (m["side_m3"] != 0)),
        "b: isolated non-channel, state all +0.0": n(~chan & iso & all_plus),
        "b: isolated non-channel, state all -0.0": n(~chan & iso & all_minus),
        "b: isolated non-channel, one vector non-zero": n(~chan & iso & (nonzero == 1)),
        "g: c <= 0 in the main channel, sideflow < 0": n((m["c1"] < 0) & (side < 0)),
        "g: 0 < c <= 1e-12 in the main channel": n((m["c1"] > 0) & (m["c1"] <= 1e-12)),
        "g: c > 1e-12 in the main channel": n(m["c1"] > 1e-12),
        "h: old discharge beyond 1e30": n(m["qold"] > 1e30),
        "h: c beyond 1e30 in the main channel": n(m["c1"] > 1e30),
        "k: area < 0.01": n(m["area_raw"] < 0.01), "k: area >= 0.01": n(m["area_raw"] >= 0.01),
        "l: sinuosity factor < 1": n(m["sinu_raw"] < 1), "l: sinuosity factor == 1": n(m["sinu_raw"] == 1),
        "l: sinuosity factor > 1": n(m["sinu_raw"] > 1),
        "m: q / area is the smaller": n(m["v1"] <= m["v2"]), "m: 0.36 q^0.24 is the smaller": n(m["v2"] < m["v1"]),
        "n: NaN sideflow on an isolated pit": n(np.isnan(side) & iso),
        "n: NaN sideflow just upstream of a pit": n(np.isnan(side) & m["pit_below"]),
        "later: NaN discharge": n(np.isnan(m["q"])),
    }
    if m["split"]:
        ex, lim = m["excess"], m["limit"]
        above = ex > lim
        c.update({
            "c: isolated non-channel, QLimit / Chan2QStart / Chan2M3Start non-zero":
                n(~chan & iso & ((m["qlimit"] != 0) | (m["q2start"] != 0) | (m["start"] != 0))),
            "d: 0 < side < 1e-7, above the limit": n(above & (side > 0) & (side < SIDE_TIE)),
            "d: -1e-7 < side < 0, above the limit": n(above & (side < 0) & (side > -SIDE_TIE)),
            "d: side == 1e-7, above the limit": n(above & (side == SIDE_TIE)),
            "d: side == nextafter(1e-7, 0), above the limit": n(above & (side == np.nextafter(SIDE_TIE, 0.0))),
            "d: |side| > 1e-7, above the limit": n(above & (np.abs(side) > SIDE_TIE)),
            "e: tot - start < M3Limit": n(ex < lim), "e: tot - start == M3Limit": n(ex == lim),
            "e: tot - start == nextafter(M3Limit)": n(ex == np.nextafter(lim, np.inf)), "e: tot - start > M3Limit": n(above),
            "f: tot == 0, above the limit": n(above & (m["tot"] == 0)),
            "f: tot > 0 and ChanM3Kin == 0, above the limit": n(above & (m["tot"] > 0) & (m["m3"] == 0)),
            "g: c <= 0 in the floodplain, sideflow < 0": n((m["c2"] < 0) & (side < 0)),
            "i: floodplain volume below Chan2M3Start": n(m["below_start"] < 0),
            "i: floodplain volume at or above Chan2M3Start": n(m["below_start"] >= 0),
            "i: Chan2M3Start == 0": n(chan & (m["start"] == 0)),
            "j: ChanQ clamped to 0": n(m["qsum"] < 0), "j: ChanQ > 0": n(m["qsum"] > 0), "j: QLimit == 0": n(chan & (m["qlimit"] == 0)),
            "later: NaN discharge where the cell's own sideflow is finite": n(np.isnan(m["q"]) & ~np.isnan(side) & chan),
        })
    return c


LATER_ROWS = ("later: NaN discharge", "later: NaN discharge where the cell's own sideflow is finite")


def substep_guard(mid):
    """cells of a split sub-step whose tot - start lies within 1e-9 (relative) of M3Limit: there the last ulp of a pow
    decides the side of the one discontinuous branch, so device and oracle could legitimately part"""
    if not mid["split"]:
        return 0
    with np.errstate(invalid="ignore"):
        near = np.abs(mid["excess"] - mid["limit"]) <= 1e-9 * np.maximum(np.abs(mid["tot"]), np.abs(mid["limit"]))
    return int(np.count_nonzero(near))


def substep_conditioning(mid, after, rtol=1e-9, atol=1e-12):
    """cells of a split sub-step whose ChanQ = ChanQKin + Chan2QKin - QLimit is a difference too ill-conditioned for the
    suite's tolerance: 4 ulp of the largest term exceed atol + rtol ChanQ"""
    if not mid["split"]:
        return 0
    with np.errstate(invalid="ignore"):
        largest = np.maximum(np.abs(after["ChanQKin"]) + np.abs(after["Chan2QKin"]), np.abs(mid["qlimit"]))
        bad = 4 * np.finfo(np.float64).eps * largest > atol + rtol * np.abs(after["ChanQ"])
    return int(np.count_nonzero(bad))


# ----------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """an oracle router that keeps what every call returned"""

    def __init__(self, router):
        self.r, self.out = router, []

    def kinematicWaveRouting(self, discharge, lateral, section="main_channel"):
        self.r.kinematicWaveRouting(discharge, lateral, section)
        self.out.append(discharge.copy())


def reference_scalars(v, beta, nsteps=NSTEPS):
    return dict(v, Beta=beta, InvBeta=1.0 / beta, InvDtRouting=1.0 / DT, DtSec=DT * nsteps)


def oracle_run(orc, d, split, irregular=False, beta=BETA, sideflows=None):
    """oracle.RoutingSubstep.dynamic over the sub-steps of `sideflows` (default d['sideflows']) -> per sub-step a dict:
    `before` / `after` (STATE, and OUT afterwards), `side`, the router outputs `qr1` / `qr2`"""
    import types
    sideflows = d["sideflows"] if sideflows is None else sideflows
    vals = statics(d, irregular)
    v = types.SimpleNamespace(**reference_scalars(vals, beta, len(sideflows)))
    v.DtRouting, v.NoRoutSteps = DT, len(sideflows)
    codes = d["codes"][d["mask"]].astype(np.float64)
    kw = orc.kinematicWave(codes, d["mask"], v.ChannelAlpha, beta, v.ChanLength, DT, alpha_floodplains=v.ChannelAlpha2)
    rec = _Recorder(kw)
    sub = orc.RoutingSubstep(rec, v)
    steps = []
    for side in sideflows:
        before = {k: getattr(v, k).copy() for k in STATE}
        rec.out = []
        with np.errstate(all="ignore"):
            sub.dynamic(split=split, sideflow_m3=side)
        after = {k: np.array(getattr(v, k), copy=True) for k in STATE + OUT}
        steps.append(dict(before=before, after=after, side=side, qr1=rec.out[0], qr2=rec.out[1] if split else None))
    return steps


def census_mid(d, vals, step, mid, beta=BETA):
    """adds to `mid` what the census needs beyond the restatement: the graph masks and the router constants
    c = upstream sum + a q_old^beta + sideflow dx (numpy's pow: they are only counted, with planted margins)"""
    down = d["down"]
    link = down >= 0
    pit_below = np.zeros(N, bool)
    pit_below[link] = down[down[link]] < 0
    mid.update(isolated=d["isolated"], has_ups=d["has_ups"], pit_below=pit_below & ~d["has_ups"], qold=step["before"]["ChanQKin"],
               q2start=vals["Chan2QStart"])
    with np.errstate(all="ignore"):
        for i, (qr, alpha, s, old) in enumerate(((step["qr1"], vals["ChannelAlpha"], mid["s1"], step["before"]["ChanQKin"]),
                                                 (step["qr2"], vals["ChannelAlpha2"], mid["s2"], step["before"]["Chan2QKin"]))):
            if qr is None:
                continue
            ups = np.bincount(down[link], weights=qr[link], minlength=N)
            mid["c%d" % (i + 1)] = ups + alpha * vals["ChanLength"] / DT * old ** beta + s * vals["ChanLength"]
    return mid


# ---- what the device files assert on these inputs --------------------------------------------------------------------
def close_to_oracle(got, want, names, vals, what):
    """device vectors against the oracle's: NaN exactly where the oracle has it, rtol 1e-9, atol 1e-12 (CrossSection2Area, a
    difference: 1e-9 max|Chan2M3Start / ChanLength|)"""
    for k in names:
        g, w = got[k], want[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), "%s, %s: NaN at %s / %s" % (what, k, np.flatnonzero(np.isnan(g))[:8],
                                                                                    np.flatnonzero(np.isnan(w))[:8])
        atol = RTOL * float(np.max(np.abs(vals["Chan2M3Start"] / vals["ChanLength"]))) if k == "CrossSection2Area" else ATOL
        np.testing.assert_allclose(g, w, rtol=RTOL, atol=atol, equal_nan=True, err_msg="%s, %s" % (what, k))


def inert_cells_are_left_alone(d, got, want, split):
    """the all-+0.0 candidates are still all +0.0; every other candidate holds what the sequential engine left (-0.0 has
    become +0.0 where the arithmetic says so).  (What this can see is a sub-step skipped on a state that still moves: a
    discharge, or the last sub-step.  An inert test that took -0.0 for +0.0 leaves the same bits, because the last sub-step
    of a call always runs and maps -0.0 to +0.0 as the skipped ones would have.)"""
    tested = INERT_TESTED if split else ["ChanQKin", "ChanM3Kin", "ChanQ"]
    plus = d["inert_cells"]["plus"]
    for k in tested:
        assert (np.ascontiguousarray(got[k][plus]).view(np.uint64) == 0).all(), k
    for name, cells in d["inert_cells"].items():
        for k in got:
            assert same_bits(got[k][cells], want[k][cells]), (name, k)
    minus = d["inert_cells"]["minus"]
    for k in tested:
        assert (got[k][minus] == 0).all() and not np.signbit(got[k][minus]).any(), k
