"""Host side of an assimilation cycle on a HotPathEnsemble: what is computed from the members at the gauges
(ens.sample(), [members, gauges] -- a few KB) and handed to ens.transform() / ens.resample(), which rewrite the state on
the device.  numpy only; members are rows throughout, as the ensemble holds them."""
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
