"""The channel router's domain: all land pixels, or only the ones whose routing sub-step is not the identity.  One rule,
asked by hotpath.HotPathDevice, hotpath.HotPathEnsemble and routing.attach_router(compact=True) alike, so that they cannot
disagree on which pixels exist.  Host code: numpy and the host half of `ldd` only."""
import numpy as np

from . import ldd as L


def inert_pixels(values, ldd_kinematic, land_mask, split, structures=None):
    """Land pixels whose routing sub-step is the identity for the whole run: no upstream and no downstream pixel in the
    kinematic LDD, not a channel pixel (so no sideflow, routing.py:512), regular parameters (0 * inf would turn the
    zero state into NaN, as it does in the reference), zero split-routing thresholds, an all-zero state, and no part
    in a structure.  Host mirror of k_inert_flags + the state test of the cell kernel (csrc/lf_router.hip)."""
    N = int(np.asarray(land_mask, bool).sum())
    get = lambda k, default=0.0: np.broadcast_to(np.asarray(values.get(k, default), dtype=np.float64), (N,))
    plus0 = lambda a: np.ascontiguousarray(a).view(np.int64) == 0
    down = L.downstream_index(ldd_kinematic, land_mask)
    has_up = np.bincount(down[down >= 0], minlength=N) > 0
    ok = (down < 0) & ~has_up & ~np.broadcast_to(np.asarray(values["IsChannelKinematic"], bool), (N,))
    with np.errstate(all="ignore"):
        t = get("InvChanLength") * get("ChanLength") * get("ChannelAlpha") * get("InvChannelAlpha")
        ok &= np.isfinite(t) & (get("InvChanLength") >= 0)
        names = ["ChanQKin", "ChanM3Kin", "ChanQ"]
        if split:
            ok &= np.isfinite(get("ChannelAlpha2") * get("InvChannelAlpha2"))
            names += ["QLimit", "Chan2QStart", "Chan2M3Start", "Chan2QKin", "Chan2M3Kin", "CrossSection2Area",
                      "Sideflow1Chan"]
    for k in names:
        ok &= plus0(get(k))
    if structures is not None:
        for k in ("LakeIndex", "ReservoirIndex"):
            if k in structures:
                ok[np.asarray(structures[k]).astype(np.int64)] = False
        for k in ("QInM3Old", "QDelta", "TransCum"):
            if k in structures:
                ok &= np.broadcast_to(np.asarray(structures[k], np.float64), (N,)) == 0
        if "InflowPoints" in structures:      # pixels that receive a hydrograph in later steps
            ok &= ~np.broadcast_to(np.asarray(structures["InflowPoints"], bool), (N,))
    return ok


def channel_domain(values, ldd_kinematic, land_mask, split, structures=None, compact=True):
    """-> (ids, chan_mask): channel-domain pixel -> land pixel, and the 2-D mask of the channel domain.  With `compact` the
    inert pixels (inert_pixels) are left out -- but only where they are at least a tenth of the domain: below that a
    second numbering costs more than the cells it saves.  Nothing dropped: ids = arange(N) and the mask is `land_mask`
    itself.  The caller subsets what it holds: ldd_kinematic[ids], its [N] channel vectors, its structures
    (_structures_on_subdomain)."""
    land_mask = np.asarray(land_mask, bool)
    N = int(land_mask.sum())
    if compact:
        drop = inert_pixels(values, np.asarray(ldd_kinematic, np.float64), land_mask, split, structures)
        if drop.sum() >= 0.1 * N:
            chan_mask = np.zeros(land_mask.shape, bool)
            chan_mask[land_mask] = ~drop
            return np.nonzero(~drop)[0], chan_mask
    return np.arange(N), land_mask


def _structures_on_subdomain(st, ids, N):
    """The structure attributes (routing.attach_structures) renumbered for the channel domain `ids` of an N-pixel one."""
    Nk = ids.size
    new_id = np.full(N + 1, Nk, np.int64)
    new_id[ids] = np.arange(Nk)
    out = {}
    for k, a in st.items():
        if k in ("LakeIndex", "ReservoirIndex"):
            out[k] = new_id[np.asarray(a).astype(np.int64)]
            if (out[k] == Nk).any():
                raise ValueError("a structure sits on a pixel outside the channel domain")
        elif k == "downstruct":
            out[k] = new_id[np.minimum(np.asarray(a).astype(np.int64), N)][ids].astype(np.int32)
        elif isinstance(a, np.ndarray) and a.shape == (N,):
            out[k] = a[ids]
        else:
            out[k] = a
    return out
