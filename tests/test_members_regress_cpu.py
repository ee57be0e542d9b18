"""No GPU: the host side of the localised serial analysis -- lf_members_regress_device is in the header, the library and
the ctypes table and refuses, device-free, what its header entry lists; HotPathEnsemble.regress() refuses what it can
judge before it touches a device; assimilation.gaspari_cohn against the textbook polynomials; serial_increments() with
the localisation switched off (a half-width of 1e9) against the Kalman mean and covariance, both kinds; one gauge against
the transform route it replaces; the restatement the GPU tests compare with (members_regress.py) against the same lines one
float at a time, and the census of the cases its inputs plant."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import members_regress as MR
import members_transform as MX
from lisflood_amd import _lib
from lisflood_amd import assimilation as AS

HEADER = os.path.join(ROOT, "include", "lisflood_amd.h")
NAME, SIGNATURE = "lf_members_regress_device", "ipiqqippppdpd"
N = 600
FAKE = C.c_void_p(64)              # a pointer that is never dereferenced: every call here ends before a device is touched
U = 2.0 ** -53                     # the unit roundoff of a double


def last_error():
    return _lib.lib().lf_last_error()


def test_the_export_is_in_the_header_the_library_and_the_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dynamic = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    table = {"lf_" + n: sig for sig, names in _lib._SIGNATURES.items() for n in names.split()}
    f = getattr(_lib.lib(), NAME)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text)
    assert re.search(r"\sT\s+%s$" % NAME, dynamic, flags=re.M)
    assert table[NAME] == SIGNATURE
    assert list(f.argtypes) == [_lib._KIND[k] for k in SIGNATURE] and f.restype is C.c_int


def test_the_header_states_the_arithmetic_and_that_the_column_is_not_centred():
    text = " ".join(open(HEADER).read().replace("\n *", " ").split())
    for line in ("d2 = dx * dx + dy * dy", "if !(d2 < cut2[j])", "p = -0.25 * z + 0.5", "rho = q - C23 / z", "if !(rho > 0)",
                 "cov = cov + x[k] * A[j][k]", "g = rho * (cov * s[j])", "x[k] = x[k] + g * D[j][k]"):
        assert line in text, line
    assert "WITHOUT centring x" in text and "anomalies sum to zero to rounding" in text


def regress(**kw):
    a = dict(rows=FAKE, members=3, stride=N + 5, n=N, gauges=4, cx=FAKE, cy=FAKE, table=FAKE, lower_dev=None, lower=-np.inf,
             upper_dev=None, upper=np.inf)
    a.update(kw)
    return _lib.lib().lf_members_regress_device(0, a["rows"], a["members"], a["stride"], a["n"], a["gauges"], a["cx"], a["cy"],
                                                a["table"], a["lower_dev"], a["lower"], a["upper_dev"], a["upper"])


REFUSED = {                        # arguments, the word of the message
    "members_1": (dict(members=1), b"members must be 2 to 64"),
    "members_0": (dict(members=0), b"members must be 2 to 64"),
    "members_65": (dict(members=65), b"members must be 2 to 64"),
    "gauges_0": (dict(gauges=0), b"gauges must be 1 to 256"),
    "gauges_257": (dict(gauges=257), b"gauges must be 1 to 256"),
    "n_negative": (dict(n=-1, stride=0), b"n = -1"),
    "n_beyond_32_bits": (dict(n=2 ** 31, stride=2 ** 31), b"outside the 32-bit range"),
    "stride_short": (dict(stride=N - 1), b"stride"),
    "rows_null": (dict(rows=None), b"rows_dev"),
    "cx_null": (dict(cx=None), b"cx_dev"),
    "cy_null": (dict(cy=None), b"cy_dev"),
    "table_null": (dict(table=None), b"table_dev"),
    "lower_above_upper": (dict(lower=2.0, upper=1.0), b"lower = 2 is greater than upper = 1"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_the_call_refuses_before_a_device_is_touched(case):
    kw, word = REFUSED[case]
    assert regress(**kw) == _lib.LF_E_INVALID, case
    assert word in last_error(), (case, last_error())


def test_what_needs_no_device_is_ok_without_one():
    """n == 0 launches nothing, and the limits themselves pass: 2 and 64 members, 1 and 256 gauges, NULL pointers with no
    element to read; bounds the wrong way round are refused only where both are scalars"""
    assert regress(n=0, stride=0) == _lib.LF_OK
    assert regress(n=0, stride=0, members=2, gauges=1) == _lib.LF_OK
    assert regress(n=0, stride=0, members=64, gauges=256) == _lib.LF_OK
    assert regress(n=0, stride=0, rows=None, cx=None, cy=None, table=None) == _lib.LF_OK
    assert regress(n=0, stride=0, lower=2.0, upper=1.0, lower_dev=FAKE) == _lib.LF_OK
    assert regress(n=0, stride=0, lower=np.nan, upper=1.0) == _lib.LF_OK


def test_regress_of_the_ensemble_refuses_before_a_device_is_touched():
    """what HotPathEnsemble.regress() judges from its arguments alone, on an object that never saw a device (the refusals
    of names and bounds are transform()'s own code and need a whole object: test_hotpath_regress_gpu.py)"""
    from lisflood_amd.hotpath import HotPathEnsemble
    mask = np.ones((4, 5), bool)
    hx = np.random.default_rng(0).standard_normal((3, 2))
    inc = AS.serial_increments(hx, np.zeros(2), np.ones(2), np.array([[1.0, 1.0], [2.0, 3.0]]), 2.0)

    def ens(members):
        e = object.__new__(HotPathEnsemble)
        e.members, e.N, e.land_mask, e._regress_coords, e._regress_table = members, 20, mask, None, None
        return e
    good = (np.zeros(20), np.zeros(20))
    for e, args, word in [(ens(1), (inc,), "2 to 64 members"), (ens(65), (inc,), "2 to 64 members"),
                          (ens(3), (inc.table,), "serial_increments"), (ens(4), (inc,), "of 3 members"),
                          (ens(3), (inc, None, (good[0],)), "coords must be"),
                          (ens(3), (inc, None, (good[0], np.zeros(19))), "coords must be"),
                          (ens(3), (inc, None, (good[0], np.zeros(20, np.float32))), "coords must be"),
                          (ens(3), (inc, None, np.zeros((2, 20))), "coords must be")]:
        with pytest.raises(ValueError, match=word):
            e.regress(*args)
        assert e._regress_table is None


# ---- Gaspari and Cohn's function ---------------------------------------------------------------------------------------------
def textbook(z):
    """Gaspari & Cohn 1999, eq. 4.10, term by term in extended precision"""
    z = np.asarray(z, np.longdouble)
    L = np.longdouble
    inner = 1 - L(5) / 3 * z ** 2 + L(5) / 8 * z ** 3 + z ** 4 / 2 - z ** 5 / 4
    with np.errstate(all="ignore"):
        outer = 4 - 5 * z + L(5) / 3 * z ** 2 + L(5) / 8 * z ** 3 - z ** 4 / 2 + z ** 5 / 12 - L(2) / (3 * z)
    return np.where(z <= 1, inner, np.where(z < 2, outer, 0))


def test_gaspari_cohn_is_the_textbook_function():
    """The Horner form against the polynomials term by term in extended precision.  The intermediate values of the outer
    branch reach 5 z = 10 and the form has eleven operations: eleven roundings of values up to 10 are 11 x 10 x 2^-53 =
    1.2e-14 at the very most.  The arithmetic was measured at 4e-15 when it was laid down; asserted at four times that,
    1.6e-14, absolute."""
    z = np.concatenate([np.linspace(0.0, 2.0, 20001), np.nextafter(1.0, [0.0, 2.0]), np.nextafter(2.0, 0.0)[None]])
    got, want = AS.gaspari_cohn(z), textbook(z)
    worst = float(np.abs(got - want).max())
    print("gaspari_cohn: largest difference from the textbook polynomials %.3e" % worst)
    assert worst <= 1.6e-14
    assert AS.gaspari_cohn(0.0) == 1.0 and AS.gaspari_cohn(1.0) == MR.RHO_AT_ONE and abs(MR.RHO_AT_ONE - 5.0 / 24.0) <= 4 * U
    assert (AS.gaspari_cohn(np.array([2.0, 2.5, 1e9, np.inf, np.nan])) == 0).all() and (got >= 0).all() and (got <= 1).all()
    assert (np.diff(got[:20001]) <= 1.6e-14).all()                    # decreasing, to the same rounding
    assert np.array_equal(MR.horner(z[z < 2]), AS._gc_horner(z[z < 2]))      # the tests' own copy of the form is the same form
    # localisation() is the device's two tests: the tie d2 == cut2 is outside, one ulp inside it is inside
    c = 2.5
    cut2 = (2.0 * c) * (2.0 * c)
    assert AS.localisation(3.0, 4.0, c, cut2) == 0.0 and AS.localisation(0.0, 0.0, c, cut2) == 1.0
    assert AS.localisation(3.0, 4.0, 5.0, 100.0) == MR.RHO_AT_ONE
    assert AS.localisation(np.nan, 4.0, 5.0, 100.0) == 0.0
    assert AS.localisation(9.0, 12.0, MR.WIDTH_TWO_ULP, (2 * MR.WIDTH_TWO_ULP) ** 2) == 0.0      # inside, the form not above 0


# ---- serial_increments without localisation: the Kalman filter ----------------------------------------------------------------
M_KF, S_KF, AT = 40, 500, (31, 207, 455)


def kalman_problem(state=S_KF, at=AT):
    """40 members, `state` elements on a 50-wide raster, 3 gauges that observe three of the elements"""
    rng = np.random.default_rng(1999)
    X = rng.standard_normal((M_KF, state)) @ (np.eye(state) + 0.3 * rng.standard_normal((state, state)) / np.sqrt(state)) * 3.0
    X = X + rng.uniform(-5, 5, state)
    at = np.asarray(at)
    hx = X[:, at].copy()
    obs_var = np.array([0.5, 1.5, 1.0]) * hx.var(axis=0, ddof=1)
    obs = hx.mean(axis=0) + rng.standard_normal(3) * np.sqrt(obs_var)
    cx, cy = (np.arange(state) // 50).astype(np.float64), (np.arange(state) % 50).astype(np.float64)
    return X, hx, obs, obs_var, cx, cy, np.stack([cx[at], cy[at]], axis=1), at


def test_eakf_increments_without_localisation_are_the_kalman_filter():
    """serial_increments(kind="eakf") with a half-width of 1e9 pixels, regressed onto the state by the restatement of the
    device's arithmetic, against the Kalman update of the SAMPLE mean and covariance: mean + K (obs - H mean) and
    (I - K H) P with K = P H^T (H P H^T + R)^-1.  For a deterministic square-root filter with uncorrelated observation
    errors, processing the gauges one after the other is the batch update exactly.  At half-width 1e9 the weight of a
    distance of 50 pixels is 1 - 5/3 (5e-8)^2 = 1 - 4e-15.  Asserted at 1e-10 of the largest covariance entry (the mean:
    of the largest |X|); measured 1e-15 when the arithmetic was laid down, printed here."""
    X, hx, obs, obs_var, cx, cy, gxy, at = kalman_problem()
    inc = AS.serial_increments(hx, obs, obs_var, gxy, 1e9)
    assert inc.gauges == 3 and inc.kept.tolist() == [0, 1, 2] and inc.dropped.size == 0
    assert inc.table.flags.c_contiguous and inc.table.dtype == np.float64 and inc.table.shape == (3 * (2 * M_KF + 5),)
    A, D, s, gx, gy, c, cut2 = MR.sections(inc.table, M_KF, 3)
    assert np.abs(A.sum(axis=1)).max() <= 8 * M_KF * U * np.abs(A).max()           # the anomalies sum to zero to rounding
    assert np.array_equal(s, 1.0 / (A * A).sum(axis=1)) and np.array_equal(cut2, (2.0 * c) * (2.0 * c)) and (c == 1e9).all()
    assert np.array_equal(np.stack([gx, gy], axis=1), gxy)
    got, touched = MR.regress(X, cx, cy, inc.table, 3)
    assert touched.all()
    mean, Xc = X.mean(axis=0), X - X.mean(axis=0)
    P = Xc.T @ Xc / (M_KF - 1)
    Hm = np.zeros((3, S_KF))
    Hm[np.arange(3), at] = 1.0
    K = P @ Hm.T @ np.linalg.inv(Hm @ P @ Hm.T + np.diag(obs_var))
    want_mean, want_P = mean + K @ (obs - Hm @ mean), (np.eye(S_KF) - K @ Hm) @ P
    gc = got - got.mean(axis=0)
    got_P = gc.T @ gc / (M_KF - 1)
    e_mean = np.abs(got.mean(axis=0) - want_mean).max() / np.abs(X).max()
    e_cov = np.abs(got_P - want_P).max() / np.abs(P).max()
    print("eakf: mean %.3e of max |X|, covariance %.3e of its largest entry %.3f" % (e_mean, e_cov, np.abs(P).max()))
    assert e_mean <= 1e-10 and e_cov <= 1e-10
    assert np.abs(got - X).max() > 0.01 * np.abs(X).max()               # (the update moved the state: something to compare)
    # the posterior at the gauges is the state's own posterior there
    assert np.abs(inc.posterior - got[:, at]).max() <= 1e-10 * np.abs(X).max()


def test_perturbed_increments_without_localisation_are_the_enkf_weights():
    """kind="perturbed" against assimilation.enkf_weights() applied in numpy, X_a[m] = sum_k X[k] W[k][m].  The batch
    update and the serial one are the same filter only where the sample covariance after each gauge is the Kalman
    posterior, which holds when the observation perturbations are uncorrelated IN THE SAMPLE with the members and with
    each other and have exactly the sample variance obs_var.  Such draws exist while state + gauges + 1 < members, so
    the state here has 20 elements: random draws are projected off the constant and the members' anomalies,
    orthogonalised and scaled.  Same tolerance as above, 1e-10 of the largest covariance entry."""
    X, hx, obs, obs_var, cx, cy, gxy, at = kalman_problem(state=20, at=(3, 11, 17))
    rng = np.random.default_rng(7)
    basis = np.linalg.qr(np.concatenate([np.ones((M_KF, 1)), X - X.mean(axis=0)], axis=1))[0]
    E = rng.standard_normal((M_KF, 3))
    E = E - basis @ (basis.T @ E)
    E = np.linalg.qr(E)[0] * np.sqrt((M_KF - 1) * obs_var)
    Y = obs + E
    assert np.abs(E.sum(axis=0)).max() < 1e-12 and np.abs(E.T @ (X - X.mean(axis=0))).max() < 1e-11
    assert np.abs(E.T @ E / (M_KF - 1) - np.diag(obs_var)).max() < 1e-12
    inc = AS.serial_increments(hx, obs, obs_var, gxy, 1e9, kind="perturbed", perturbed_obs=Y)
    got, _ = MR.regress(X, cx[:20], cy[:20], inc.table, 3)
    want = MX.transform(X, AS.enkf_weights(hx, obs, obs_var, Y))
    Xc = X - X.mean(axis=0)
    scale = np.abs(Xc.T @ Xc / (M_KF - 1)).max()
    gc, wc = got - got.mean(axis=0), want - want.mean(axis=0)
    e_state = np.abs(got - want).max() / np.abs(X).max()
    e_cov = np.abs(gc.T @ gc - wc.T @ wc).max() / (M_KF - 1) / scale
    print("perturbed: members %.3e of max |X|, covariance %.3e of its largest entry %.3f" % (e_state, e_cov, scale))
    assert e_state <= 1e-10 and e_cov <= 1e-10
    assert np.abs(got - X).max() > 0.01 * np.abs(X).max()
    for bad in (dict(kind="perturbed"), dict(kind="perturbed", perturbed_obs=Y[:, :2]), dict(kind="etkf")):
        with pytest.raises(ValueError):
            AS.serial_increments(hx, obs, obs_var, gxy, 1e9, **bad)


def test_one_gauge_is_the_transform_route():
    """One gauge through the route regress() replaces: transform with W = I + s A D^T (W[k][m] = delta_km + s A[k] D[m]) and the
    taper rho, through the transform's restatement.  Both compute x[m] + rho s D[m] sum_k x[k] A[k], in different orders.
    With S = sum_k |x[k] A[k]| and T = |x[m]| + s |D[m]| S, to first order in u = 2^-53:
      the transform: an entry of W has 3 roundings, a product 1, the sum M - 1: (M + 3) u T; then t - x[m], the product
      with the taper (<= 1) and the sum with x[m]: 3 u T more;
      the regression: the products and the sum M u s |D[m]| S, then cov s, rho ., g D[m] and the last sum: 4 u T more.
    The bound asserted is their sum, (2 M + 10) u T, entry by entry."""
    M, n = 7, 1000
    x, cx, cy, table = MR.make_case(n, M, 7, 31)
    A, D, s, gx, gy, c, cut2 = MR.sections(table, M, 7)
    fine = np.isfinite(x).all(axis=0) & np.isfinite(cx) & np.isfinite(cy)
    x, cx, cy = x[:, fine], cx[fine], cy[fine]
    worst = 0.0
    for j in (0, 1, 2, 6):
        one = np.concatenate([A[j], D[j], [s[j], gx[j], gy[j], c[j], cut2[j]]])
        got, touched = MR.regress(x, cx, cy, one, 1)
        rho = AS.localisation(cx - gx[j], cy - gy[j], c[j], cut2[j])
        assert np.array_equal(rho > 0, touched) and touched.sum() > 5 and not touched.all()
        want = MX.transform(x, np.eye(M) + s[j] * np.outer(A[j], D[j]), rho)
        S = (np.abs(x) * np.abs(A[j])[:, None]).sum(axis=0)
        T = np.abs(x) + s[j] * np.abs(D[j])[:, None] * S[None, :]
        bound = (2 * M + 10) * U * T
        assert np.array_equal(MR.bits(got[:, ~touched]), MR.bits(x[:, ~touched]))
        assert np.abs(want[:, ~touched] - x[:, ~touched]).max() == 0          # (a taper of 0 on finite values: the member's own)
        worst = max(worst, float((np.abs(got - want) / bound)[:, touched].max()))
        assert (np.abs(got - want) <= bound).all(), j
        assert np.abs(got - x)[:, touched].max() > 1e-3
    print("one gauge against the transform route: the largest difference is %.3f of its bound" % worst)


def test_a_gauge_without_spread_is_dropped_and_reported():
    rng = np.random.default_rng(3)
    hx = rng.standard_normal((6, 4)) + 5.0
    hx[:, 2] = 1.25                                                     # every member equal: no spread at its turn
    xy = np.array([[0.0, 0.0], [40.0, 0.0], [80.0, 0.0], [120.0, 0.0]])  # half-width 4: no gauge moves another
    inc = AS.serial_increments(hx, np.full(4, 5.0), np.ones(4), xy, 4.0)
    assert inc.kept.tolist() == [0, 1, 3] and inc.dropped.tolist() == [2] and inc.gauges == 3 and inc.members == 6
    assert inc.table.shape == (3 * (2 * 6 + 5),) and np.array_equal(inc.gx, [0.0, 40.0, 120.0])
    assert np.array_equal(inc.posterior[:, 2], hx[:, 2]) and inc.posterior.shape == (6, 4)
    assert np.array_equal(inc.chunk(1, 3), np.concatenate([inc.anomalies[1:3].ravel(), inc.increments[1:3].ravel(), inc.scale[1:3],
                                                           inc.gx[1:3], inc.gy[1:3], inc.halfwidth[1:3], inc.cut2[1:3]]))
    # a scalar half-width is the same as a row of it; each gauge is pulled toward its observation and loses spread
    again = AS.serial_increments(hx, np.full(4, 5.0), np.ones(4), xy, np.full(4, 4.0))
    assert np.array_equal(again.table, inc.table)
    for j in (0, 1, 3):
        assert inc.posterior[:, j].var() < hx[:, j].var()
        assert abs(inc.posterior[:, j].mean() - 5.0) < abs(hx[:, j].mean() - 5.0)
    # within reach, an earlier gauge moves a later one: its anomalies in the table are no longer those of hx
    near = AS.serial_increments(hx, np.full(4, 5.0), np.ones(4), xy / 40.0, 4.0)
    assert np.array_equal(near.anomalies[0], inc.anomalies[0]) and not np.array_equal(near.anomalies[1], inc.anomalies[1])
    every = AS.serial_increments(np.full((3, 2), 2.0), np.zeros(2), np.ones(2), xy[:2], 4.0)
    assert every.gauges == 0 and every.table.shape == (0,) and every.dropped.tolist() == [0, 1]
    for bad in (dict(hx=hx[:1]), dict(obs=np.zeros(3)), dict(obs_var=np.zeros(4)), dict(gauge_xy=xy[:, :1]), dict(halfwidth=0.0),
                dict(halfwidth=np.ones(3))):
        a = dict(hx=hx, obs=np.full(4, 5.0), obs_var=np.ones(4), gauge_xy=xy, halfwidth=4.0)
        a.update(bad)
        with pytest.raises(ValueError):
            AS.serial_increments(**a)


# ---- the restatement and its inputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower,upper", [("absent", "absent"), ("scalar", "row"), ("row", "scalar")])
def test_the_restatement_is_the_header_one_float_at_a_time(lower, upper):
    M, n, G = 5, 230, 7
    x, cx, cy, table = MR.make_case(n, M, G, 11)
    lo, hi = MR.bound_of(lower, n, 7, True)[0], MR.bound_of(upper, n, 8, False)[0]
    got, touched = MR.regress(x, cx, cy, table, G, lo, hi)
    want = MR.regress_by_element(x, cx, cy, table, G, lo, hi)
    assert not MR.agree(got, want, touched).any() and np.array_equal(MR.bits(got), MR.bits(want))
    assert touched.any() and not touched.all() and np.isnan(got).any()
    if lower == "absent":                                               # no bounds: what no gauge touched keeps its raw bits
        assert np.array_equal(MR.bits(got[:, ~touched]), MR.bits(x[:, ~touched]))


def test_the_census_finds_every_planted_case():
    """the family the GPU tests draw from, at its full size: each case the inputs are built to plant is counted from the
    values, and a family that lost one fails here"""
    M, n, G = 5, 1000, 7
    x, cx, cy, table = MR.make_case(n, M, G, 3)
    found = MR.census(x, cx, cy, table, G)
    print(found)
    missing = [k for k, v in found.items() if v == 0]
    assert not missing, missing
    assert found["nan_coordinate"] == 2 and found["wave_one_beside_none"] == 1 and found["payload_untouched"] >= 2
    d2, z, rho, inside, active = MR.reach(cx, cy, table, M, G)
    assert d2[0, 1] == 25.0 and not inside[0, 1]                        # offset (3, 4), c = 2.5: d2 == cut2 skips
    assert z[1, 2] == 1.0 and rho[1, 2] == MR.RHO_AT_ONE == 0.20833333333333326 and active[1, 2]
    assert z[2, 3] == np.nextafter(2.0, 0.0) and inside[2, 3] and 0 < rho[2, 3] < 2e-16
    assert inside[3, 6] and rho[3, 6] < 0 and not active[3, 6]          # two ulp below 2: inside, and left alone
    assert z[0, 0] == 0.0 and rho[0, 0] == 1.0 and active[:, 0].all()   # on gauge 0, and reached by every gauge
    assert active[:, 9].sum() == 1 and active[G - 1, 9]                 # reached by the last gauge alone
    assert not inside[:, 64:128].any() and (inside[:, 128:192].sum(axis=1) == 1).all() and inside[:, MR.ONE_LANE].all()
    assert not inside[:, 4].any() and not inside[:, 5].any()            # a NaN coordinate is in no gauge's reach
    for members, n, G in ((2, 65, 1), (9, 257, 64), (64, 255, 256)):    # the smaller draws keep what their size allows
        small = MR.census(*MR.make_case(n, members, G, 5), G)
        assert small["on_gauge"] and small["tie_cut"] and small["reached_0"] and small["minus_zero_untouched"], (members, n, G)
