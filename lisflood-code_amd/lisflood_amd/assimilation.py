"""Host side of an assimilation cycle on a HotPathEnsemble: what is computed from the members at the gauges
(ens.sample(), [members, gauges] -- a few KB) and handed to ens.transform() / ens.resample(), which rewrite the state on
the device.  numpy only; members are rows throughout, as the ensemble holds them.

A cycle of the localised serial filter (serial_increments() + ens.regress(): every gauge corrects the pixels near it, all
gauges in one pass over the state), with model error as the forecast half:

    P = fourier_patterns(land_mask, 8, 30.0, rng)           # once: [8, N] patterns for the model error
    c = ar1_coefficients(None, (members, 8), 0.02, rng)
    ens.step(forcing)                                        # forecast
    hx = ens.sample("ChanQ", gauge_pixels)                   # [members, G]: the members at the gauges, a few KB
    inc = serial_increments(hx, obs, obs_var, gauge_rc, halfwidth=25.0)          # gauge_rc [G, 2]: (row, column) of the gauges
    ens.regress(inc, bounds={"W1a": (0.0, None), "ChanQ": (0.0, None)})          # analysis: inc.table goes up, nothing else
    c = ar1_coefficients(c, 0.9, 0.02, rng)
    ens.perturb(c, P, ["W1a", "W1b"], multiplicative=True)   # model error, so that the spread does not collapse
    ens.step(forcing)                                        # the next forecast sees the analysed state

inc.dropped lists the gauges that had no spread at their turn, inc.posterior is the analysed ensemble at the gauges.
kind="perturbed" with perturbed_obs=obs + sqrt(obs_var) N(0, 1) gives the stochastic filter instead of the square-root
one; coords=(X, Y) in regress() and the same coordinates in gauge_rc put the distances on any other two-coordinate map.

Areal observations -- satellite soil-moisture or snow footprints, basin averages -- enter the same way: the members' zone
means take the place of the members at the gauges, the zones' centroids that of the gauges' places:

    xy, radius = zone_geometry(footprints, land_mask)        # once: [Z, 2] centroids, [Z] equivalent radii in pixels
    hx = ens.zonal("Theta1aPixel", footprints)               # [members, Z] footprint means, made on the device
    inc = serial_increments(hx, obs, obs_var, xy, halfwidth=np.maximum(25.0, radius))
    ens.regress(inc, bounds={"W1a": (0.0, None)})"""
import numpy as np


def enkf_weights(hx, obs, obs_var, perturbed_obs=None):
    """The transform of the stochastic ensemble Kalman filter (Evensen 2003, perturbed observations) as a
    [members, members] matrix W with  X_a[m] = sum_k X[k] W[k][m]  for ANY state row set X [members, .] of the ensemble:

        W = I + (I - 1 1^T / M) A C^-1 (Y - HX)^T,     A = HX - mean over the members,  C = A^T A + (M - 1) diag(obs_var)

    hx [members, G]: the members at the gauges;  obs [G]: the observations;  obs_var [G]: their error variances (> 0);
    perturbed_obs [members, G]: Y, each member's own draw obs + N(0, obs_var) -- None: every member gets obs itself (the
    update of the mean is the same, the spread comes out too small: for smoothers that inflate afterwards).  This is
    X_a = X + K (Y - HX) with the gain K = P_xy (P_yy + R)^-1 of the sample covariances, the (M - 1) cancelled; C is solved
    with np.linalg.solve, never inverted.  Y == HX gives the identity exactly."""
    hx = np.asarray(hx, np.float64)
    if hx.ndim != 2:
        raise ValueError("hx must be [members, gauges]")
    M, G = hx.shape
    obs, obs_var = np.asarray(obs, np.float64), np.asarray(obs_var, np.float64)
    if obs.shape != (G,) or obs_var.shape != (G,):
        raise ValueError("obs and obs_var must be [%d]" % G)
    Y = np.broadcast_to(obs, (M, G)) if perturbed_obs is None else np.asarray(perturbed_obs, np.float64)
    if Y.shape != (M, G):
        raise ValueError("perturbed_obs must be [%d, %d]" % (M, G))
    if M < 2:
        raise ValueError("an ensemble covariance needs at least 2 members")
    A = hx - hx.mean(axis=0)
    Cm = A.T @ A + (M - 1) * np.diag(obs_var)
    S = np.linalg.solve(Cm, (Y - hx).T)                   # [G, members]
    centre = np.eye(M) - np.full((M, M), 1.0 / M)
    return np.eye(M) + centre @ (A @ S)


_C53, _C112, _C23 = 5.0 / 3.0, 1.0 / 12.0, 2.0 / 3.0


def _gc_horner(z):
    """both branches of Gaspari & Cohn's function in the Horner form of lf_members_regress_device, chosen by z <= 1"""
    with np.errstate(all="ignore"):
        p = -0.25 * z + 0.5
        p = p * z + 0.625
        p = p * z - _C53
        p = p * z
        p = p * z + 1.0
        q = _C112 * z - 0.5
        q = q * z + 0.625
        q = q * z + _C53
        q = q * z - 5.0
        q = q * z + 4.0
        q = q - _C23 / z
    return np.where(z <= 1.0, p, q)


def gaspari_cohn(z):
    """Gaspari & Cohn's (1999, eq. 4.10) compactly supported fifth-order correlation function of z = distance / half-width:
    1 at z = 0, 5/24 at z = 1, 0 from z = 2 on -- in the Horner form the device evaluates (include/lisflood_amd.h).  The form
    dips to about -3e-16 just below z = 2; what is not above 0 there, z >= 2 and a NaN give 0."""
    z = np.asarray(z, np.float64)
    rho = _gc_horner(z)
    return np.where((z < 2.0) & (rho > 0.0), rho, 0.0)


def localisation(dx, dy, halfwidth, cut2):
    """the weight lf_members_regress_device gives a gauge at the offset (dx, dy) -- its two tests included: 0 where
    !(dx dx + dy dy < cut2) and where the Horner form is not above 0"""
    dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    with np.errstate(all="ignore"):
        d2 = dx * dx + dy * dy
        inside = d2 < cut2
        rho = _gc_horner(np.sqrt(d2) / halfwidth)
    return np.where(inside & (rho > 0.0), rho, 0.0)


class SerialIncrements:
    """What serial_increments() hands to HotPathEnsemble.regress(): the sections of lf_members_regress_device's table for
    the gauges that were kept, in the order they were processed.
    anomalies, increments [K, members]; scale, gx, gy, halfwidth, cut2 [K];  kept: the K indices into the caller's gauges,
    dropped: the others (no spread at their turn);  posterior [members, G]: the members at ALL gauges after the last
    update (a dropped gauge is still moved by the others);  table: the whole table, one contiguous float64 array."""

    def __init__(self, anomalies, increments, scale, gx, gy, halfwidth, kept, dropped, posterior):
        self.anomalies, self.increments, self.scale = anomalies, increments, scale
        self.gx, self.gy, self.halfwidth = gx, gy, halfwidth
        self.cut2 = (2.0 * halfwidth) * (2.0 * halfwidth)
        self.kept, self.dropped, self.posterior = kept, dropped, posterior
        self.members, self.gauges = anomalies.shape[1], anomalies.shape[0]
        self.table = self.chunk(0, self.gauges)

    def chunk(self, first, last):
        """the table of the gauges first .. last - 1 alone: (last - first) (2 members + 5) doubles"""
        k = slice(first, last)
        return np.concatenate([self.anomalies[k].reshape(-1), self.increments[k].reshape(-1), self.scale[k], self.gx[k],
                               self.gy[k], self.halfwidth[k], self.cut2[k]])


def serial_increments(hx, obs, obs_var, gauge_xy, halfwidth, kind="eakf", perturbed_obs=None):
    """The observation-space half of the two-step serial ensemble filter (Anderson 2003; Whitaker & Hamill 2002) with
    Gaspari-Cohn localisation: the gauges are processed one after the other, in ascending order, and for each one the
    anomalies of its CURRENT prior (as the gauges before it left it) and the increments of the members are noted down --
    HotPathEnsemble.regress() then regresses all of them onto the state in one pass over it.

    hx [members, G]: the members at the gauges (ens.sample());  obs, obs_var [G]: observations and their error variances
    (> 0);  gauge_xy [G, 2]: the gauges' coordinates, in the coordinates regress() is given (by default the pixel's row and
    column);  halfwidth: the localisation half-width c, a scalar or [G], > 0 -- the weight is gaspari_cohn(distance / c),
    zero from 2 c on.  For gauge j with prior y, mean ym, a = y - ym, ss = sum a^2, var = ss / (M - 1), r = obs_var[j]:
        kind "eakf":       pv = 1 / (1 / var + 1 / r);  pm = pv (ym / var + obs / r);  d = (pm - ym) + (sqrt(pv / var) - 1) a
        kind "perturbed":  d = var / (var + r) (perturbed_obs[:, j] - y)          (perturbed_obs [members, G], required)
    and every OTHER gauge l moves as the state element at its place does:  y_l += rho (sum_k y_l[k] a[k] / ss) d  with rho
    the localisation weight of the distance between the two gauges -- a later gauge's prior, an earlier one's posterior,
    so that .posterior is the state's own posterior at the gauges.  The sum is taken without centring y_l, as on the
    device: a sums to zero to rounding.  A gauge whose ss is 0 at its turn (every member equal) says nothing about
    the state: it is dropped from the table and listed in .dropped.  -> SerialIncrements."""
    hx = np.asarray(hx, np.float64)
    if hx.ndim != 2:
        raise ValueError("hx must be [members, gauges]")
    M, G = hx.shape
    if M < 2:
        raise ValueError("an ensemble covariance needs at least 2 members")
    obs, obs_var = np.asarray(obs, np.float64), np.asarray(obs_var, np.float64)
    if obs.shape != (G,) or obs_var.shape != (G,):
        raise ValueError("obs and obs_var must be [%d]" % G)
    if not np.all(obs_var > 0):
        raise ValueError("obs_var must be above 0")
    xy = np.asarray(gauge_xy, np.float64)
    if xy.shape != (G, 2):
        raise ValueError("gauge_xy must be [%d, 2]" % G)
    c = np.asarray(halfwidth, np.float64)
    if c.ndim == 0:
        c = np.full(G, float(c))
    if c.shape != (G,) or not np.all(c > 0):
        raise ValueError("halfwidth must be a scalar or [%d], above 0" % G)
    if kind not in ("eakf", "perturbed"):
        raise ValueError("kind must be \"eakf\" or \"perturbed\"")
    if kind == "perturbed":
        if perturbed_obs is None or np.shape(perturbed_obs) != (M, G):
            raise ValueError("kind \"perturbed\" takes perturbed_obs [%d, %d]" % (M, G))
        Y = np.asarray(perturbed_obs, np.float64)
    cut2 = (2.0 * c) * (2.0 * c)
    y = hx.copy()
    kept, dropped, anomalies, increments, scale = [], [], [], [], []
    for j in range(G):
        yj = y[:, j].copy()
        ym = yj.mean()
        a = yj - ym
        ss = float((a * a).sum())
        if ss == 0.0:
            dropped.append(j)
            continue
        var, r = ss / (M - 1), obs_var[j]
        if kind == "eakf":
            pv = 1.0 / (1.0 / var + 1.0 / r)
            pm = pv * (ym / var + obs[j] / r)
            d = (pm - ym) + (np.sqrt(pv / var) - 1.0) * a
        else:
            d = var / (var + r) * (Y[:, j] - yj)
        s = 1.0 / ss
        # every other gauge moves as the state element at its place does: the later ones' priors, the earlier ones' posteriors
        rho = localisation(xy[:, 0] - xy[j, 0], xy[:, 1] - xy[j, 1], c[j], cut2[j])
        g = rho * ((a @ y) * s)
        y += d[:, None] * g[None, :]
        y[:, j] = yj + d                                      # (the gauge itself: rho = 1 and sum a a / ss = 1)
        kept.append(j)
        anomalies.append(a)
        increments.append(d)
        scale.append(s)
    K = np.asarray(kept, np.int64)
    return SerialIncrements(np.array(anomalies, np.float64).reshape(len(kept), M), np.array(increments, np.float64).reshape(len(kept), M),
                            np.asarray(scale, np.float64), xy[K, 0].copy(), xy[K, 1].copy(), c[K].copy(), K,
                            np.asarray(dropped, np.int64), y)


def zone_geometry(zones, land_mask, weights=None):
    """Where an areal observation sits, for serial_increments() and regress(): zones as HotPathEnsemble.zonal() takes them
    (an int label map [N] in pixel order, negative: no zone; or a sequence of Z arrays of compressed land indices) on the
    land pixels of land_mask [H, W], weights [N] in pixel order as zonal() takes them (None: every pixel 1).
    -> (centroids float64 [Z, 2]: the weighted mean (row, column) of the zone's pixels -- gauge_xy in regress()'s default
    coordinates;  radius float64 [Z]: sqrt(pixels / pi), the radius of the disc with the zone's number of pixels, a lower
    bound for the localisation half-width).  A zone without pixels, or whose weights sum to 0, has a NaN centroid."""
    mask = np.asarray(land_mask)
    if mask.ndim != 2 or mask.dtype != np.bool_:
        raise ValueError("land_mask must be a boolean [H, W] array")
    from .zonal import zone_pairs
    rows, cols = np.nonzero(mask)
    zone, pix, Z = zone_pairs(zones, rows.size)
    w = np.ones(rows.size) if weights is None else np.asarray(weights, np.float64)
    if w.shape != (rows.size,):
        raise ValueError("weights must be [%d] in pixel order" % rows.size)
    total = np.bincount(zone, w[pix], minlength=Z)
    with np.errstate(divide="ignore", invalid="ignore"):
        centroids = np.stack([np.bincount(zone, w[pix] * rows[pix], minlength=Z) / total,
                              np.bincount(zone, w[pix] * cols[pix], minlength=Z) / total], axis=1)
    return centroids, np.sqrt(np.bincount(zone, minlength=Z) / np.pi)


def systematic_parents(weights, u):
    """Systematic resampling (Kitagawa 1996): member k is drawn as often as the points (u + j) / M, j = 0 .. M - 1, fall
    into [c[k-1], c[k]) of the cumulated normalised weights c -- at most one draw differs from M weights[k] either way.
    weights [members] >= 0, not all zero (normalised here);  u in [0, 1).
    -> int32 [members] for HotPathEnsemble.resample(): every member that was drawn at all keeps its own slot, the further
    copies go to the slots of the members that were not drawn, in ascending order -- so resample() writes as few rows as
    there are members lost."""
    w = np.asarray(weights, np.float64)
    if w.ndim != 1 or w.size < 1 or not np.all(w >= 0) or not np.isfinite(w).all() or not w.sum() > 0:
        raise ValueError("weights must be [members], finite, not negative and not all zero")
    if not 0.0 <= u < 1.0:
        raise ValueError("u must lie in [0, 1)")
    M = w.size
    c = np.cumsum(w)
    c = c / c[-1] * M
    # point j lies at or beyond c[k] where c[k] - j <= u: the difference is exact where it matters (c[k] close to j), while
    # u + j would round a u just below 1 up to the next integer
    drawn = np.minimum((c[None, :] - np.arange(M)[:, None] <= np.float64(u)).sum(axis=1), M - 1)
    counts = np.bincount(drawn, minlength=M)
    parents = np.arange(M, dtype=np.int32)
    free = np.flatnonzero(counts == 0)
    spare = np.repeat(np.arange(M), np.maximum(counts - 1, 0))
    parents[free] = spare
    return parents


def fourier_patterns(land_mask, rank, length_scale, rng):
    """Static spatial patterns for HotPathEnsemble.forcing_perturbation() / perturb(): random Fourier features (Rahimi &
    Recht 2007) of a Gaussian covariance with the given length scale, in pixels, on the land pixels of land_mask [H, W]:

        P_r(x) = sqrt(2 / rank) cos(w_r . x + phi_r),   w_r ~ N(0, I / length_scale^2),   phi_r ~ U[0, 2 pi),   x = (row, column)

    With iid N(0, 1) coefficients c [members, rank], c @ P is a smooth field of (approximately, for the rank is small) unit
    variance and covariance exp(-|x - y|^2 / (2 length_scale^2)); |P| <= sqrt(2 / rank) everywhere.
    -> float64 [rank, N] in pixel order (the land pixels in row-major order), rank 1 to 16.  rng: a numpy Generator, which
    is drawn from in a fixed order (the rank frequencies, then the rank phases)."""
    mask = np.asarray(land_mask)
    if mask.ndim != 2 or mask.dtype != np.bool_:
        raise ValueError("land_mask must be a boolean [H, W] array")
    if not (isinstance(rank, (int, np.integer)) and 1 <= rank <= 16):
        raise ValueError("rank must be an integer from 1 to 16")
    if not (np.ndim(length_scale) == 0 and np.isfinite(length_scale) and length_scale > 0):
        raise ValueError("length_scale must be a finite number of pixels above 0")
    rows, cols = np.nonzero(mask)
    w = rng.standard_normal((rank, 2)) / float(length_scale)
    phi = rng.uniform(0.0, 2.0 * np.pi, rank)
    x = np.stack([rows, cols]).astype(np.float64)                     # [2, N]
    return np.sqrt(2.0 / rank) * np.cos(w @ x + phi[:, None])


def ar1_coefficients(previous, rho, sigma, rng):
    """One step of the AR(1) process that perturbed-forcing and model-error schemes run on their coefficients:

        c = rho previous + sqrt(1 - rho^2) sigma N(0, 1)

    whose stationary standard deviation is sigma.  previous: [members, rank] -- or None with rho = (members, rank): a first
    draw, sigma N(0, 1).  rho in [-1, 1]; sigma >= 0, a scalar or anything that broadcasts to [members, rank] (a value
    per pattern).  rho = 1 returns a copy of previous bit for bit (nothing is added, so a -0.0 keeps its sign); the rng is
    drawn from all the same, so a run's random stream does not depend on rho.  -> float64 [members, rank]."""
    sigma = np.asarray(sigma, np.float64)
    if not (np.all(np.isfinite(sigma)) and np.all(sigma >= 0)):
        raise ValueError("sigma must be finite and not negative")
    if previous is None:
        shape = tuple(rho) if np.ndim(rho) == 1 and len(rho) == 2 else None
        if shape is None or not all(isinstance(k, (int, np.integer)) and k >= 1 for k in shape):
            raise ValueError("a first draw (previous=None) takes rho = (members, rank)")
        try:
            np.broadcast_to(sigma, shape)
        except ValueError:
            raise ValueError("sigma does not broadcast to [%d, %d]" % shape) from None
        return sigma * rng.standard_normal(shape)
    previous = np.asarray(previous, np.float64)
    if previous.ndim != 2:
        raise ValueError("previous must be [members, rank]")
    if not (np.ndim(rho) == 0 and -1.0 <= rho <= 1.0):
        raise ValueError("rho must lie in [-1, 1]")
    try:
        np.broadcast_to(sigma, previous.shape)
    except ValueError:
        raise ValueError("sigma does not broadcast to [%d, %d]" % previous.shape) from None
    noise = rng.standard_normal(previous.shape)
    scale = np.sqrt(1.0 - float(rho) * float(rho))
    if scale == 0.0:
        return float(rho) * previous
    return float(rho) * previous + (scale * sigma) * noise
