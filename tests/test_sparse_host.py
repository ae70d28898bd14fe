"""tn.sparse_tt_svd on the CPU (the mirror the device path is compared with) and the argument envelope of its C entries.

The golden data (tests/golden/sparse_tt_svd_f64.npz, tools/gen_sparse_golden.py) are runs of the unmodified reference in fp64.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import tntorch_amd as tn
from tntorch_amd import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sparse_tt_svd_f64.npz")
CASES = ("dense", "s200", "s200r", "n2")


def golden_case(name):
    z = np.load(GOLDEN)
    rmax = int(z[name + "_rmax"])
    return (torch.from_numpy(z[name + "_X"]), torch.from_numpy(z[name + "_y"]), float(z[name + "_eps"]), rmax or None,
            [int(r) for r in z[name + "_ranks"]], torch.from_numpy(z[name + "_recon"]))


def golden_bound(name):
    """Relative to ||y||: the larger of 100 x the worst distance of the CPU mirror from the reference's reconstruction over the
    golden cases (recorded in golden/sparse_tt_svd_meta.json when the mirror was written) and nrows x 2.2e-16, nrows the tallest unfolding."""
    with open(os.path.join(HERE, "golden", "sparse_tt_svd_meta.json")) as f:
        meta = json.load(f)
    X, y, eps, rmax, ranks, recon = golden_case(name)
    nrows = max(ranks[n] * recon.shape[n] for n in range(recon.dim() - 1))
    return max(100.0 * meta["mirror_worst_distance"], nrows * 2.2e-16)


def zero_filled(X, y, shape=None):
    shape = shape or [int(v) + 1 for v in X.max(dim=0)[0]]
    D = torch.zeros(shape, dtype=y.dtype)
    D[tuple(X.t())] = y
    return D


@pytest.mark.parametrize("name", CASES)
def test_golden_replay(name):
    X, y, eps, rmax, ranks, recon = golden_case(name)
    t = tn.sparse_tt_svd(X, y, eps, rmax=rmax)
    assert [int(r) for r in t.ranks_tt] == ranks
    assert t.cores[0].dtype == torch.float64
    dist = float(torch.norm(t.torch() - recon) / torch.norm(y))
    print(name, "distance from the reference's reconstruction / ||y|| =", dist, "bound", golden_bound(name))
    assert dist <= golden_bound(name)


@pytest.mark.parametrize("eps", [0.3, 0.05, 1e-6])
@pytest.mark.parametrize("name", ["dense", "s200"])
def test_eps_guarantee(name, eps):
    X, y = golden_case(name)[:2]
    t = tn.sparse_tt_svd(X, y, eps)
    D = zero_filled(X, y, [6, 5, 7, 4])
    err = float(torch.norm(t.torch() - D) / torch.norm(D))
    print(name, eps, "ranks", t.ranks_tt.tolist(), "relative error", err)
    assert err <= eps * (1 + 1e-6)


def test_rmax_caps_every_rank_and_shape_gives_zero_slices():
    X, y = golden_case("s200")[:2]
    for rmax in (1, 2, 5):
        t = tn.sparse_tt_svd(X, y, 1e-9, rmax=rmax)
        assert max(int(r) for r in t.ranks_tt) <= rmax
    shape = [8, 5, 9, 6]
    t = tn.sparse_tt_svd(X, y, 1e-9, shape=shape)
    assert list(t.shape) == shape
    full = t.torch()
    assert float(torch.norm(full - zero_filled(X, y, shape)) / torch.norm(y)) < 1e-12
    assert float(full[6:].abs().max()) == 0.0 and float(full[:, :, 7:].abs().max()) == 0.0 and float(full[..., 4:].abs().max()) == 0.0


def test_rank_is_capped_by_the_column_count():
    X, y = golden_case("s200")[:2]
    t = tn.sparse_tt_svd(X, y, 1e-9)
    assert int(t.ranks_tt[-2]) <= 4  # the last unfolding has at most 4 columns (the reference returns 64 here)
    cols = [len(torch.unique(X[:, n:], dim=0)) for n in range(1, 4)]
    assert all(int(t.ranks_tt[n + 1]) <= cols[n] for n in range(3))
    assert float(torch.norm(t.torch() - zero_filled(X, y, [6, 5, 7, 4])) / torch.norm(y)) < 1e-12


def test_value_errors():
    X = torch.tensor([[0, 1, 2], [1, 0, 1], [2, 2, 0]])
    y = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    bad = X.clone()
    bad[1, 2] = -1
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(bad, y, 0.1)
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(bad, y, 0.1, shape=[3, 3, 3])
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(X, y, 0.1, shape=[3, 3, 2])  # index 2 in a mode of size 2
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(torch.cat([X, X[:1]]), torch.cat([y, y[:1]]), 0.1)  # a repeated position
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(X[:, :1], y, 0.1)  # N = 1
    with pytest.raises(ValueError):
        tn.sparse_tt_svd(X[:0], y[:0], 0.1)  # P = 0


def test_dtype_follows_y_and_numpy_inputs():
    X, y = golden_case("s200")[:2]
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    try:
        t64 = tn.sparse_tt_svd(X, y, 0.05)
        t32 = tn.sparse_tt_svd(X.numpy().astype(np.int32), y.numpy().astype(np.float32), 0.05)
    finally:
        torch.set_default_dtype(old)
    assert all(c.dtype == torch.float64 for c in t64.cores) and all(c.dtype == torch.float32 for c in t32.cores)
    D = zero_filled(X, y, [6, 5, 7, 4])
    assert float(torch.norm(t32.torch().double() - D) / torch.norm(D)) <= 0.05 * (1 + 1e-4)


def test_one_sample_and_two_modes():
    t = tn.sparse_tt_svd(torch.tensor([[2, 1]]), torch.tensor([3.0], dtype=torch.float64), 0.1, shape=[4, 3])
    full = t.torch()
    assert [int(r) for r in t.ranks_tt] == [1, 1, 1] and float(full[2, 1]) == pytest.approx(3.0, rel=1e-14)
    full[2, 1] = 0
    assert float(full.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ C-ABI envelope
SPARSE_SIGNATURES = {
    "ttr_sparse_keys": ("c_int", ["c_long", "c_long", "c_void_p", "c_long", "c_long", "c_void_p", "c_void_p", "c_void_p", "c_void_p"]),
    "ttr_sparse_levels": ("c_int", ["c_long", "c_long", "c_void_p", "c_long", "c_long", "c_void_p", "c_void_p", "c_void_p", "c_void_p"]),
    "ttr_sparse_group_workspace_bytes": ("c_long", ["c_long", "c_long"]),
    "ttr_sparse_group": ("c_int", ["c_long", "c_long", "c_void_p", "c_void_p", "c_void_p", "c_void_p", "c_long", "c_void_p"]),
    "ttr_sparse_gram_parts": ("c_long", ["c_int", "c_long", "c_long", "c_long"]),
    "ttr_sparse_gram_workspace_bytes": ("c_long", ["c_int", "c_long", "c_long", "c_long"]),
    "ttr_sparse_gram": ("c_int", ["c_int"] + ["c_long"] * 4 + ["c_void_p"] * 6 + ["c_long", "c_void_p", "c_long", "c_void_p", "c_long", "c_void_p"]),
    "ttr_sparse_project": ("c_int", ["c_int"] + ["c_long"] * 5 + ["c_void_p"] * 3 + ["c_long", "c_void_p", "c_long", "c_long", "c_void_p", "c_long", "c_void_p"]),
}


def test_entries_are_declared_in_the_header():
    for name, (res, args) in SPARSE_SIGNATURES.items():
        got = _hip._SIGNATURES[name]
        assert (got[0].__name__, [a.__name__ for a in got[1]]) == (res, args), name
    assert _hip.ABI_VERSION >= 15


@pytest.fixture(scope="module")
def cabi():
    """The cross-compiled library, loaded without a device: every call below returns from its argument checks."""
    import __graft_entry__ as g

    g.build()
    L = ctypes.CDLL(g.LIB)
    for name in SPARSE_SIGNATURES:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _hip._SIGNATURES[name]
    L.ttr_last_error.restype = ctypes.c_char_p
    return L


def test_sparse_entries_argument_envelope(cabi):
    OK, INVALID, UNSUPPORTED, WORKSPACE = _hip.OK, _hip.E_INVALID, _hip.E_UNSUPPORTED, _hip.E_WORKSPACE
    p = ctypes.c_void_p(64)  # never dereferenced: the calls below stop at their argument checks

    def gram(dt, r, I, nb, C, ptr=None, ldv=None, ldg=None, wsb=1 << 40):
        return cabi.ttr_sparse_gram(dt, r, I, nb, C, ptr, ptr, ptr, ptr, ptr, ptr, ldv or r, ptr, ldg or r * I, ptr, wsb, None)

    def project(dt, r, I, q, nb, C, ptr=None):
        return cabi.ttr_sparse_project(dt, r, I, q, nb, C, ptr, ptr, ptr, r, ptr, q, 1, ptr, q, None)

    assert cabi.ttr_sparse_keys(4, 3, None, 3, 1, None, None, None, None) == INVALID and b"NULL" in cabi.ttr_last_error()
    assert cabi.ttr_sparse_keys(4, 3, None, 3, 1, None, None, p, None) == INVALID and b"NULL" in cabi.ttr_last_error()
    assert cabi.ttr_sparse_keys(-1, 3, p, 3, 1, p, p, p, None) == INVALID and cabi.ttr_sparse_keys(4, 0, p, 3, 1, p, p, p, None) == INVALID
    assert cabi.ttr_sparse_levels(4, 3, None, 3, 1, None, None, None, None) == INVALID and b"NULL" in cabi.ttr_last_error()
    assert cabi.ttr_sparse_levels(0, 3, None, 3, 1, None, None, None, None) == OK
    assert cabi.ttr_sparse_levels(4, 0, p, 3, 1, p, p, p, None) == INVALID
    assert cabi.ttr_sparse_keys(1 << 31, 3, p, 3, 1, p, p, p, None) == UNSUPPORTED
    assert cabi.ttr_sparse_levels(1 << 31, 3, p, 3, 1, p, p, p, None) == UNSUPPORTED
    assert cabi.ttr_sparse_group_workspace_bytes(5000, 3) == 2 * 3 * 4 and cabi.ttr_sparse_group_workspace_bytes(0, 7) == 7 * 4
    assert cabi.ttr_sparse_group_workspace_bytes(10, 4097) == UNSUPPORTED and cabi.ttr_sparse_group_workspace_bytes(10, 0) == INVALID
    assert cabi.ttr_sparse_group(10, 3, None, None, None, None, 1 << 20, None) == INVALID and b"NULL" in cabi.ttr_last_error()
    assert cabi.ttr_sparse_group(10, 3, p, p, p, p, 11, None) == WORKSPACE
    assert cabi.ttr_sparse_group(10, 4097, p, p, p, p, 1 << 20, None) == UNSUPPORTED
    for dt, lim in ((_hip.F32, 4096), (_hip.F64, 2048)):
        assert cabi.ttr_eigh_max_n(dt) == lim
        assert gram(dt, 3, 5, 10, 4) == INVALID and b"NULL" in cabi.ttr_last_error()
        assert gram(dt, lim // 64 + 1, 64, 10, 4) == UNSUPPORTED and b"above" in cabi.ttr_last_error()
        assert gram(dt, 1, lim + 1, 10, 4) == UNSUPPORTED and gram(dt, lim, 1, 10, 4) == INVALID  # r I = limit: on to the pointers
        assert gram(dt, 0, 5, 10, 4) == INVALID and gram(dt, 3, 0, 10, 4) == INVALID and gram(dt, 3, 5, -1, 0) == INVALID
        assert gram(dt, 3, 5, 10, 11, p) == INVALID  # more columns than blocks
        assert gram(dt, 3, 5, 10, 4, p, ldv=2) == INVALID and gram(dt, 3, 5, 10, 4, p, ldg=14) == INVALID
        assert gram(dt, 3, 5, 10, 4, p, wsb=15 * 15 * (4 if dt == _hip.F32 else 8) - 1) == WORKSPACE
        assert gram(dt, 3, 5, 1 << 31, 4) == UNSUPPORTED
        assert cabi.ttr_sparse_gram_workspace_bytes(dt, 3, 5, 10) == 15 * 15 * (4 if dt == _hip.F32 else 8)
        assert cabi.ttr_sparse_gram_parts(dt, 3, 5, 10) == 1 and cabi.ttr_sparse_gram_parts(dt, 3, 1, 5000) == 3
        assert cabi.ttr_sparse_gram_parts(dt, lim + 1, 1, 10) == UNSUPPORTED
        assert project(dt, 3, 5, 2, 10, 4) == INVALID and b"NULL" in cabi.ttr_last_error()
        assert project(dt, 3, 5, 2, 10, 0) == OK
        assert project(dt, 3, 5, 16, 10, 4) == UNSUPPORTED  # q above r I
        assert project(dt, lim // 64 + 1, 64, 2, 10, 4) == UNSUPPORTED
        assert project(dt, 3, 5, 0, 10, 4) == INVALID and project(dt, 3, 5, 2, 3, 4) == INVALID
    assert gram(2, 3, 5, 10, 4) == INVALID and project(2, 3, 5, 2, 10, 4) == INVALID
    assert cabi.ttr_sparse_gram_parts(2, 3, 5, 10) == INVALID
