"""routing.substep_host_vectors: the one place where the host vectors behind lf_substep_args are broadcast, gathered
into the device order and converted (no device needed); routing.SubstepVectors: those vectors on the device and the
argument block that points at them, without a router (gpu)."""
import ctypes as C

import numpy as np
import pytest

from lisflood_amd._lib import DeviceArray
from lisflood_amd.routing import _OUT, _STATE, _STATIC, SubstepVectors, _SubstepArgs, result_names, substep_host_vectors

N, PERM = 6, np.array([4, 1, 5, 2])            # a shuffled subset: a compact domain of 4 of the 6 host pixels


def first_case():
    """name -> host value: a scalar, a float32 vector, a non-contiguous flag vector, ChannelAlpha2 absent, and a
    distinct float64 vector under every other name"""
    values = {k: (i + 1) * 10.0 + np.arange(N) + 0.125 for i, k in enumerate(_STATIC + _STATE)}
    values["ChanLength"] = 250.0
    values["ChannelAlpha"] = (0.3 * np.arange(1, N + 1)).astype(np.float32)
    values["IsChannelKinematic"] = np.array([1, 0, 0, 1, 1, 0, 1, 1, 0, 0, 1, 0], bool)[::2]
    del values["ChannelAlpha2"]
    assert not values["IsChannelKinematic"].flags.c_contiguous
    return values


def test_broadcast_gather_and_dtype_name_by_name():
    values = first_case()
    out = substep_host_vectors(values, N, PERM)
    assert list(out) == _STATIC + _STATE
    for k, a in out.items():
        want = np.broadcast_to(values.get(k, 0.0), (N,))[PERM]
        assert a.dtype == (np.uint8 if k == "IsChannelKinematic" else np.float64), k
        assert a.shape == (PERM.size,) and a.flags.c_contiguous, k
        assert np.array_equal(a, want), k
    assert not out["ChannelAlpha2"].any()                   # the zero default
    assert out["IsChannelKinematic"].tolist() == [0, 0, 1, 1]
    assert out["ChannelAlpha"].tolist() == [float(values["ChannelAlpha"][i]) for i in PERM]
    assert list(substep_host_vectors(values, N, PERM, ["QLimit"])) == ["QLimit"]


def test_a_namespace_is_read_like_a_mapping():
    import types
    values = first_case()
    a, b = substep_host_vectors(types.SimpleNamespace(**values), N, PERM), substep_host_vectors(values, N, PERM)
    for k in b:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_missing_channel_flag_is_ones():
    values = first_case()
    del values["IsChannelKinematic"]
    a = substep_host_vectors(values, N, PERM)["IsChannelKinematic"]
    assert a.dtype == np.uint8 and a.flags.c_contiguous and a.tolist() == [1, 1, 1, 1]


def test_no_perm_is_identity_order():
    values = first_case()
    out = substep_host_vectors(values, N)
    for k, a in out.items():
        assert a.shape == (N,) and a.flags.c_contiguous, k
        assert np.array_equal(a, np.broadcast_to(values.get(k, 0.0), (N,))), k


def test_empty_domain_gives_empty_arrays():
    out = substep_host_vectors({"ChanLength": 250.0, "ChannelAlpha": np.zeros(0, np.float32)}, 0)
    assert list(out) == _STATIC + _STATE
    for k, a in out.items():
        assert a.shape == (0,) and a.dtype == (np.uint8 if k == "IsChannelKinematic" else np.float64), k


def test_result_names():
    assert result_names(True) == _STATE + ["FlowVelocity", "TravelDistance"]
    assert result_names(False) == ["ChanQKin", "ChanM3Kin", "ChanQ", "sumDisDay", "FlowVelocity", "TravelDistance"]


POINTERS = [k for k, t in _SubstepArgs._fields_ if t is C.c_void_p]
SCALARS = dict(Beta=0.6, InvDtRouting=1 / 3600.0, DtSec=86400.0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "state_size", "sideflow", "empty", "two_stage"])
def test_vectors_and_argument_block(case):
    n_dev = 0 if case == "empty" else PERM.size
    host = substep_host_vectors({}, 0) if case == "empty" else substep_host_vectors(first_case(), N, PERM)
    opts = {}
    if case == "state_size":
        opts["state_size"] = 7
    if case == "sideflow":
        opts["sideflow"] = 0.5 + np.arange(3 * n_dev, dtype=np.float64).reshape(3, n_dev)
    split, engine_order = (0, 1) if case == "plain" else (1, 0)
    if case == "two_stage":         # a caller that keeps its own allocation order: some names now, the rest later
        opts["order"] = _STATIC + _STATE
    sv = SubstepVectors(host, n_dev, split=split, engine_order=engine_order, **SCALARS, **opts)
    try:
        if case == "two_stage":
            assert list(sv.dev) == _STATIC + _STATE and not sv.args.scratch0
            sv.allocate(["SideflowChanM3"] + _OUT + ["scratch0", "scratch1"])
        assert sorted(sv.dev) == sorted(POINTERS) == sorted(_STATIC + _STATE + _OUT + ["SideflowChanM3", "scratch0", "scratch1"])
        want = dict(host)
        want["SideflowChanM3"] = opts["sideflow"].reshape(-1) if case == "sideflow" else np.zeros(n_dev)
        for k in _OUT + ["scratch0", "scratch1"]:
            want[k] = np.zeros(n_dev)
        for k in POINTERS:
            got = sv.download(k)
            size = 7 if case == "state_size" and k in ("ChanQKin", "Chan2QKin") else max(want[k].size, 1)
            assert got.shape == (size,) and got.dtype == want[k].dtype, k          # no buffer shorter than one element
            assert got[:want[k].size].tobytes() == want[k].tobytes(), k
            assert not got[want[k].size:].any(), k                                 # ghost slots / the padding element: zero
            assert getattr(sv.args, k) == sv.dev[k].ptr.value != 0, k
        a = sv.args
        assert (a.Beta, a.InvBeta, a.InvDtRouting, a.DtSec) == (0.6, 1 / 0.6, 1 / 3600.0, 86400.0)
        assert (a.split, a.engine_order) == (split, engine_order)
        # with_overrides: a copy with the pointer replaced; the resident block stays as it is
        before = bytes(a)
        other = DeviceArray(3)
        b = sv.with_overrides(sumDisDay=other.ptr.value)
        assert b.sumDisDay == other.ptr.value != a.sumDisDay and bytes(a) == before
        b.sumDisDay = a.sumDisDay
        assert bytes(b) == before
        other.free()
        # upload: a vector of the name's own length, ghost slots behind it untouched; any other length is refused
        sv.upload("ChanQKin", np.arange(7.0, 7.0 + n_dev))
        assert sv.download("ChanQKin")[:n_dev].tolist() == list(range(7, 7 + n_dev)) and not sv.download("ChanQKin")[n_dev:].any()
        with pytest.raises(AssertionError):
            sv.upload("ChanQ", np.zeros(n_dev + 1))
        if n_dev:
            with pytest.raises(AssertionError):
                sv.upload("ChanQ", np.zeros(n_dev - 1))
    finally:
        sv.free()
        sv.free()           # harmless
    assert all(not d.ptr.value for d in sv.dev.values())
