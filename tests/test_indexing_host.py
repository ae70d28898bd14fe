"""NumPy-style indexing of Tensor on the host mirror (tensor.py:1019-1434), replayed against tests/golden/indexing_f64.npz
(recorded from the reference by tools/gen_indexing_golden.py): values, returned core shapes and return types, plus the
reference's error cases."""
import json
import os

import numpy as np
import pytest
import torch

import tntorch_amd as tn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "indexing_f64.npz")


def decode(k):
    if isinstance(k, int):
        return k
    (tag, v), = k.items()
    if tag == "tuple":
        return tuple(decode(x) for x in v)
    if tag == "list":
        return [decode(x) for x in v]
    if tag == "ndarray":
        return np.array(v)
    if tag == "slice":
        return slice(*v)
    if tag == "none":
        return None
    return Ellipsis


def golden_cases():
    g = np.load(GOLDEN)
    meta = json.loads(bytes(g["meta"]).decode())
    for ci, m in enumerate(meta):
        cores = [torch.from_numpy(g[f"c{ci}_core{n}"]) for n in range(m["ncores"])]
        Us = [torch.from_numpy(g[f"c{ci}_U{n}"]) if m["tucker"][n] else None for n in range(m["ncores"])]
        keys = [(decode(e["key"]), e, g[f"c{ci}_k{ki}"]) for ki, e in enumerate(m["keys"])]
        yield m["name"], cores, Us, m["batch"], keys


def replay(device, dtype=torch.float64, tol=1e-12):
    """Every golden key through Tensor.__getitem__ with the cores on `device`; returns the number of keys checked."""
    checked = 0
    for name, cores, Us, batch, keys in golden_cases():
        t = tn.Tensor([c.to(device, dtype) for c in cores], Us=[None if U is None else U.to(device, dtype) for U in Us],
                      batch=batch)
        for key, e, want in keys:
            r = t[key]
            where = f"{name} {key!r}"
            if e["type"] == "scalar":
                assert isinstance(r, torch.Tensor) and not isinstance(r, tn.Tensor), where
                got = r.detach().cpu().double().numpy()
            else:
                assert isinstance(r, tn.Tensor), where
                assert r.batch == e["batch"], where
                assert [list(c.shape) for c in r.cores] == e["core_shapes"], where
                assert [None if U is None else list(U.shape) for U in r.Us] == e["U_shapes"], where
                assert all(c.device == t.cores[0].device for c in r.cores), where
                got = r.torch().cpu().double().numpy()
            assert got.shape == want.shape, where
            err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
            assert err <= tol, f"{where}: {err:.3e}"
            checked += 1
    return checked


def test_golden_replay_host():
    assert replay("cpu") == 88


def _tt(shape=(6, 7, 8, 9), r=3, seed=0, batch=False):
    g = torch.Generator().manual_seed(seed)
    ranks = [1] + [r] * (len(shape) - 1) + [1]
    lead = [4] if batch else []
    return tn.Tensor([torch.randn(lead + [ranks[n], s, ranks[n + 1]], generator=g, dtype=torch.float64)
                      for n, s in enumerate(shape)], batch=batch)


def test_errors_as_reference():
    t = _tt()
    with pytest.raises(IndexError):
        t[6]
    with pytest.raises(IndexError):
        t[0, 7]
    with pytest.raises(IndexError):
        t[-7]
    with pytest.raises(IndexError):
        t[[0, 6]]
    with pytest.raises(IndexError, match="Too many index entries"):
        t[0, 0, 0, 0, 0]
    with pytest.raises(IndexError, match="Only one ellipsis"):
        t[..., 0, ...]
    with pytest.raises(IndexError, match="contiguously"):
        t[[0], :, [0]]
    with pytest.raises(IndexError, match="contiguously"):
        t[[0], 0, [1]]
    with pytest.raises(ValueError, match="same length"):
        t[[0, 1], [0]]
    b = _tt(batch=True)
    with pytest.raises(ValueError, match="Cannot change batch dimension"):
        b[None, ...]
    with pytest.raises(ValueError, match="Advanced indexing is prohibited for batch dimension"):
        b[[0], [0]]
    with pytest.raises(IndexError):
        b[4]


def test_negative_indices():
    t = _tt()
    x = t.torch()
    assert torch.allclose(t[-1, 2, -3, 0], x[-1, 2, -3, 0], rtol=1e-13, atol=0)
    got = t[[-1, 0, -6], [3, -7, 6]]
    assert torch.allclose(got.torch(), x[[-1, 0, -6], [3, -7, 6]], rtol=1e-13, atol=1e-15)
    assert torch.allclose(t[:, -2].torch(), x[:, -2], rtol=1e-13, atol=1e-15)


def test_index_matrix_and_tensor_keys():
    t = _tt()
    x = t.torch()
    g = torch.Generator().manual_seed(1)
    P = torch.stack([torch.randint(0, s, (50,), generator=g) for s in t.shape], 1)
    for key in (P, P.numpy(), P.int()):
        r = t[key]
        assert [tuple(c.shape) for c in r.cores] == [(1, 50, 1)]
        assert torch.allclose(r.torch(), x[tuple(P.T)], rtol=1e-12, atol=1e-14)


def test_iteration_stops():
    t = _tt((3, 4, 5))
    items = [x for x in t]
    assert len(items) == 3
    assert all(torch.allclose(a.torch(), t.torch()[i], rtol=1e-13, atol=1e-15) for i, a in enumerate(items))


def test_input_cores_unchanged():
    t = _tt()
    t.Us[1] = torch.randn(5, 7, dtype=torch.float64)
    before = [c.clone() for c in t.cores] + [t.Us[1].clone()]
    for key in [(0, [1, 2], [3, 4]), (slice(None), 1), (1, 2, 3, 4), (None, ..., 2), ([0, 1, 2],)]:
        t[key]
    after = list(t.cores) + [t.Us[1]]
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_out_of_scope():
    t = _tt()
    with pytest.raises(NotImplementedError):
        t[t]  # mask Tensor keys need tn.accepted_inputs (automata)
    with pytest.raises(NotImplementedError):
        t[0] = 1.0
    cp = tn.Tensor([torch.randn(6, 2, dtype=torch.float64), torch.randn(7, 2, dtype=torch.float64)])
    with pytest.raises(NotImplementedError):
        cp[0, 0]
