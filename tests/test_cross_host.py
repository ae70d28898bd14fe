"""TT-cross on CPU tensors: maxvol and tn.cross replayed against tests/golden/{maxvol,cross}_f64.npz (recorded from the
unmodified reference by tools/gen_cross_golden.py), restatements of the reference's cross / ops tests, meshgrid, and the
keyword contract of tn.cross."""
import logging
import os

import numpy as np
import pytest
import torch

import tntorch_amd as tn
from tools.gen_cross_golden import MAXVOL_CASES, c_rows, cross_cases, maxvol_input

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture
def f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def replay_maxvol(device, ctol):
    """Every golden maxvol case on `device`: index exact, C to `ctol` (absolute; |C| <= 1.05 after the swaps)."""
    g = np.load(os.path.join(GOLDEN, "maxvol_f64.npz"))
    for k, (N, r, it) in enumerate(MAXVOL_CASES):
        A = torch.as_tensor(maxvol_input(k, N, r)).to(device)
        index, C = tn.maxvol(A, max_iters=it)
        assert index.dtype == torch.int64 and tuple(C.shape) == ((N, N) if N <= r else (N, r))
        np.testing.assert_array_equal(index.cpu().numpy(), g[f"m{k}_index"], err_msg=f"case {k}: {(N, r, it)}")
        rows = c_rows(N)
        np.testing.assert_allclose(C.cpu().numpy()[rows], g[f"m{k}_C"], rtol=0, atol=ctol, err_msg=f"case {k}: {(N, r, it)}")
    return len(MAXVOL_CASES)


def run_case(name, case, device):
    """tn.cross on one golden case, seeded as the generator was (its NumPy seed gives initial right sets without repeated rows); returns (tensor, info, next torch draws, next numpy draws)."""
    g = np.load(os.path.join(GOLDEN, "cross_f64.npz"))
    kw = {k: v for k, v in case.items() if k != "tensors_cores"}
    if "tensors_cores" in case:
        kw["tensors"] = [tn.Tensor([torch.as_tensor(g[f"{name}_in{a}{n}"]).to(device) for n in range(len(cs))])
                         for a, cs in zip("ab", case["tensors_cores"])]
    else:
        kw["domain"] = [d.to(device) for d in kw["domain"]]
    torch.manual_seed(11)
    np.random.seed(int(g[f"{name}_np_seed"]))
    t, info = tn.cross(**kw, verbose=False, return_info=True, suppress_warnings=True)
    return t, info, torch.randn(4).numpy(), np.random.rand(4)


def replay_cross(device, core_rtol):
    g = np.load(os.path.join(GOLDEN, "cross_f64.npz"))
    cases = cross_cases()
    for name, case in cases.items():
        t, info, nt, nn = run_case(name, case, device)
        N = t.dim()
        np.testing.assert_array_equal(np.asarray(info["Rs"]), g[f"{name}_Rs"], err_msg=name)
        for n in range(N):
            np.testing.assert_array_equal(info["lsets"][n], g[f"{name}_lset{n}"], err_msg=f"{name} lset {n}")
            np.testing.assert_array_equal(info["rsets"][n], g[f"{name}_rset{n}"], err_msg=f"{name} rset {n}")
        for n in range(N):
            ref = g[f"{name}_core{n}"]
            c = t.cores[n].detach().cpu().numpy()
            assert c.shape == ref.shape, (name, n)
            assert np.linalg.norm(c - ref) <= core_rtol * np.linalg.norm(ref), (name, n, np.linalg.norm(c - ref) / np.linalg.norm(ref))
        assert info["nsamples"] == int(g[f"{name}_nsamples"]), name
        np.testing.assert_array_equal(nt, g[f"{name}_next_torch"], err_msg=name)
        np.testing.assert_array_equal(nn, g[f"{name}_next_np"], err_msg=name)
        yield name, info, g[f"{name}_val_epss"]


def test_maxvol_golden():
    assert replay_maxvol("cpu", 1e-12) == len(MAXVOL_CASES)


def test_cross_golden(f64):
    seen = 0
    for name, info, val_epss in replay_cross("cpu", 1e-10):
        # same number of sweeps; the values agree to round-off (the validation points are evaluated in another summation order)
        np.testing.assert_allclose(np.array([float(v) for v in info["val_epss"]]), val_epss, rtol=1e-9, atol=1e-13, err_msg=name)
        seen += 1
    assert seen == 5


def test_maxvol_contract():
    A = torch.randn(3, 50, 6, dtype=torch.float64)
    idx, C = tn.maxvol(A)
    assert idx.shape == (3, 6) and C.shape == (3, 50, 6)
    for b in range(3):
        i1, C1 = tn.maxvol(A[b])
        assert torch.equal(i1, idx[b]) and torch.allclose(C1, C[b])
        np.testing.assert_allclose(C[b][idx[b]], np.eye(6), atol=1e-12)
        np.testing.assert_allclose(C[b], A[b] @ torch.linalg.inv(A[b][idx[b]]), atol=1e-12)
        assert C[b].abs().max() <= 1.05 + 1e-12
    i, C = tn.maxvol(torch.randn(4, 7))
    assert torch.equal(i, torch.arange(4)) and torch.equal(C, torch.eye(4))
    # tol below 1 counts as 1; max_iters=0 keeps the LU rows
    i0, _ = tn.maxvol(A[0], max_iters=0)
    lu_rows = torch.linalg.lu_factor(A[0])[1]
    assert i0.shape == (6,) and len(set(i0.tolist())) == 6 and lu_rows.shape == (6,)
    iA, _ = tn.maxvol(A[0], tol=0.5)
    iB, _ = tn.maxvol(A[0], tol=1.0)
    assert torch.equal(iA, iB)


# ------------------------------------------------------------------ the reference's test_cross.py / test_ops.py, restated
def check(t, full, tol):
    assert torch.norm(t.torch() - full) / torch.norm(full) < tol


def test_cross_domain(f64):
    domain = [torch.linspace(-1, 1, 12)] * 4
    X = torch.meshgrid(*domain, indexing="ij")
    f = lambda x, y, z, w: torch.cos(x + y) * torch.exp(z) + w ** 2
    t = tn.cross(function=f, domain=domain, verbose=False)
    check(t, f(*X), 1e-6)
    g = lambda M: torch.sum(M ** 2, dim=1)
    t = tn.cross(function=g, domain=domain, function_arg="matrix", verbose=False)
    check(t, sum(x ** 2 for x in X), 1e-6)


def test_cross_tensors(f64):
    t = tn.rand([10] * 4, ranks_tt=3) + 1.0
    check(tn.cross(function=lambda x: x ** 2, tensors=t, verbose=False), t.torch() ** 2, 1e-6)
    t2 = tn.rand([10] * 4, ranks_tt=2)
    check(tn.cross(function=lambda x, y: x * y + 2 * x, tensors=[t, t2], verbose=False), t.torch() * t2.torch() + 2 * t.torch(), 1e-6)


UNARY = {"abs": lambda x: x + 2, "acos": lambda x: x / 3, "asin": lambda x: x / 3, "cos": None, "cosh": None, "erf": None,
         "erfinv": lambda x: x / 3, "exp": None, "log": lambda x: x + 2, "log10": lambda x: x + 2, "log2": lambda x: x + 2,
         "reciprocal": lambda x: x + 2, "rsqrt": lambda x: x + 2, "sigmoid": None, "sin": None, "sinh": None,
         "sqrt": lambda x: x + 2, "tan": lambda x: x / 3, "tanh": None}


def test_ops(f64):
    torch.manual_seed(1)
    x = torch.linspace(-1, 1, 16)
    for name, shift in UNARY.items():
        base = tn.meshgrid([x] * 3)
        xs = base[0] + base[1] * 0.5 + base[2] * 0.25  # values in [-1.75, 1.75]
        t = tn.Tensor([c.clone() for c in xs.cores])
        arg = t.torch() if shift is None else shift(t.torch())
        if shift is not None:
            t = tn.cross(lambda v: shift(v), tensors=t, verbose=False)
        check(getattr(tn, name)(t), getattr(torch, name)(arg), 1e-5)
    a, b = tn.meshgrid([x + 2, x + 3])
    for name, fn in {"add": torch.add, "atan2": torch.atan2, "mul": torch.mul, "div": torch.div, "pow": torch.pow}.items():
        check(getattr(tn, name)(a, b), fn(a.torch(), b.torch()), 1e-5)


def test_meshgrid(f64):
    ts = tn.meshgrid(3, torch.tensor([1.0, 5.0]), np.array([2.0, 4.0, 6.0, 8.0]))
    assert len(ts) == 3 and all(t.shape == torch.Size([3, 2, 4]) for t in ts)
    grids = torch.meshgrid(torch.arange(3.0), torch.tensor([1.0, 5.0]), torch.tensor([2.0, 4.0, 6.0, 8.0]), indexing="ij")
    for t, d in zip(ts, grids):
        assert torch.equal(t.torch(), d) and t.cores[0].dtype == torch.float64
    ts2 = tn.meshgrid([torch.linspace(0, 1, 5)] * 2)
    assert len(ts2) == 2 and ts2[1].ranks_tt.tolist() == [1, 1, 1]
    assert tn.meshgrid([4, 4], batch=True)[0].batch


def test_cross_keywords(f64, caplog):
    domain = [torch.linspace(0, 1, 8)] * 3
    f = lambda x, y, z: 1 / (1 + x + y + z)
    t, info = tn.cross(f, domain=domain, ranks_tt=3, max_iter=2, val_size=50, return_info=True, record_samples=True,
                       verbose=False, eps=1e-30, suppress_warnings=True)
    for k in ("nsamples", "eval_time", "val_epss", "min", "argmin", "lsets", "rsets", "Rs", "left_locals", "total_time", "val_eps",
              "sample_positions", "sample_values"):
        assert k in info, k
    assert info["sample_positions"].shape == (info["nsamples"], 3) and info["sample_values"].shape == (info["nsamples"],)
    X = torch.meshgrid(*domain, indexing="ij")
    pos = info["sample_positions"]
    assert torch.allclose(info["sample_values"], f(pos[:, 0], pos[:, 1], pos[:, 2]))
    assert len(info["val_epss"]) == 2 and len(info["left_locals"]) == 2
    assert all(isinstance(s, np.ndarray) for s in info["lsets"] + info["rsets"] + info["left_locals"])
    check(t, f(*X), 1e-3)
    with caplog.at_level(logging.WARNING):
        tn.cross(f, domain=domain, ranks_tt=1, max_iter=1, verbose=False)
    assert any("larger than" in r.message for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        tn.cross(f, domain=domain, ranks_tt=1, max_iter=1, verbose=False, suppress_warnings=True)
    assert not caplog.records
    # function_arg='matrix' sees [P, N]; detach_evaluations detaches the result
    seen = []
    tn.cross(lambda M: seen.append(M.shape) or M.sum(dim=1), domain=domain, function_arg="matrix", ranks_tt=2, max_iter=1,
             verbose=False, suppress_warnings=True)
    assert all(len(s) == 2 and s[1] == 3 for s in seen)
    w = torch.tensor(2.0, requires_grad=True)
    t = tn.cross(lambda x, y, z: w * x, domain=domain, ranks_tt=1, max_iter=1, verbose=False, detach_evaluations=True)
    assert not t.cores[0].requires_grad


def test_cross_errors(f64):
    t = tn.rand([4] * 3, ranks_tt=2, batch=True)
    with pytest.raises(ValueError, match="Batched"):
        tn.cross(lambda x: x, tensors=t, verbose=False)
    with pytest.raises(ValueError, match="Invalid return value"):
        tn.cross(lambda x, y: torch.log(x - 0.5), domain=[torch.linspace(0, 1, 5)] * 2, verbose=False)


def test_cross_cp_host(f64):
    """CP factors on the host follow the reference's CP branch."""
    g = torch.Generator().manual_seed(3)
    U = [torch.rand(6, 2, generator=g) + 0.5 for _ in range(3)]
    t = tn.Tensor(U)
    full = torch.einsum("ir,jr,kr->ijk", *U)
    check(tn.cross(lambda x: torch.sqrt(x), tensors=t, verbose=False), torch.sqrt(full), 1e-6)
