"""The Boolean layer on CPU tensors: automata, logic, ``tn.mask``, the operators ``~ & | ^`` and ``tn.partialset`` against data recorded
from the unmodified reference (tests/golden/automata_f64.npz) and against dense Boolean arithmetic.  Integer-exact throughout:
the random trains of the mask and partialset cases have integer cores and steps that are powers of two."""
import os
import re

import numpy as np
import pytest
import torch

import automata_cases as ac
import tntorch_amd as tn
from tntorch_amd import _hostops

F64 = torch.float64


def dense(t):
    return t.torch().double().numpy()


# ---------------------------------------------------------------------------------------------- constructors
@pytest.mark.parametrize("name", sorted(ac.CTORS))
def test_constructor_cores_equal_the_reference(name):
    t, gold = ac.build(name), ac.golden_cores(name)
    assert len(t.cores) == len(gold)
    for c, g in zip(t.cores, gold):
        assert c.dtype == torch.float32 and c.device.type == "cpu" and torch.equal(c, g)
    t64 = ac.build(name, dtype=F64, device="cpu")
    assert all(c.dtype == F64 and torch.equal(c, g.double()) for c, g in zip(t64.cores, gold))


@pytest.mark.parametrize("name", ac.DENSE)
def test_formula_values_equal_the_reference(name):
    assert np.array_equal(dense(ac.dense_formula(name)), ac.fixture()["dense_" + name])
    assert ac.dense_formula(name, dtype=F64).cores[0].dtype == F64


def test_only_equals_the_reference():
    x, y, z, w = tn.symbols(4)
    assert np.array_equal(dense(tn.only(x)), ac.fixture()["dense_only_x"])
    assert np.array_equal(dense(tn.only(x | z)), ac.fixture()["dense_only_xz"])
    assert float(tn.only(x).torch().sum()) == 1.0


def test_true_false_symbols():
    assert np.array_equal(dense(tn.true(3)), np.ones((2, 2, 2))) and np.array_equal(dense(tn.false(3)), np.zeros((2, 2, 2)))
    s = tn.symbols(3, dtype=F64)
    assert len(s) == 3 and all(np.array_equal(dense(s[n]), dense(tn.presence(3, n))) for n in range(3))
    assert s[0].cores[0].dtype == F64


# ---------------------------------------------------------------------------------------------- operators and predicates
def test_operators_against_dense_boolean_arithmetic():
    x, y, z, w = tn.symbols(4)
    a, b = (x & ~y) | z, tn.weight_mask(4, [1, 2]) ^ w
    A, B = dense(a).astype(bool), dense(b).astype(bool)
    assert np.array_equal(dense(~a), (~A).astype(float))
    assert np.array_equal(dense(a & b), (A & B).astype(float))
    assert np.array_equal(dense(a | b), (A | B).astype(float))
    assert np.array_equal(dense(a ^ b), (A ^ B).astype(float))
    X, Y, Z = (np.indices((2, 2, 2, 2))[n].astype(bool) for n in range(3))
    assert np.array_equal(A, (X & ~Y) | Z)
    assert "__eq__" not in tn.Tensor.__dict__ and tn.Tensor.__hash__ is object.__hash__   # hashing is unchanged


def test_relevant_symbols():
    x, y, z, w = tn.symbols(4)
    assert tn.relevant_symbols(x & ~y) == [0, 1] and tn.irrelevant_symbols(x & ~y) == [2, 3]
    assert tn.relevant_symbols(tn.true(4)) == [] and tn.relevant_symbols((x & y) | (x & ~y)) == [0]


def test_implies_equiv_and_predicates():
    x, y, z = tn.symbols(3)
    assert tn.implies(x & y, x) and not tn.implies(x, x & y)
    assert tn.equiv(x | y, ~(~x & ~y)) and not tn.equiv(x | y, x ^ y)
    assert tn.equiv(tn.one(3), (x & ~y & ~z) | (~x & y & ~z) | (~x & ~y & z))
    assert tn.is_tautology(x | ~x) and not tn.is_tautology(x)
    assert tn.is_contradiction(x & ~x) and not tn.is_contradiction(x)
    assert tn.is_satisfiable(x & y & z) and not tn.is_satisfiable(x & ~x)


# ---------------------------------------------------------------------------------------------- accepted_inputs
@pytest.mark.parametrize("name", ["wm52", "wm4", "w3"])
def test_accepted_inputs_equal_the_reference(name):
    X = tn.accepted_inputs(ac.build(name))
    assert X.dtype == torch.int64 and torch.equal(X, torch.from_numpy(ac.fixture()["acc_" + name]))
    assert torch.equal(tn.accepted_inputs(ac.build(name, dtype=F64)), X)


def test_accepted_inputs_multiplicities_zero_and_one_mode():
    X = tn.accepted_inputs(tn.weight(3))
    assert X.shape == (12, 3) and torch.equal(X, ac.dense_accepted(dense(tn.weight(3))))   # weights above 1 repeat their string
    Z = tn.accepted_inputs(tn.false(3))
    assert Z.shape == (0, 3) and Z.dtype == torch.int64 and tuple(ac.fixture()["acc_zero"].shape) == (0, 3)
    assert torch.equal(tn.accepted_inputs(tn.weight_mask(1, 1)), torch.from_numpy(ac.fixture()["acc_n1"]))


def test_accepted_inputs_against_combinations():
    X = tn.accepted_inputs(tn.weight_mask(12, 6))
    assert X.shape == (924, 12) and torch.equal(X, ac.combinations_matrix(12, 6))


def test_accepted_inputs_contracts_tucker_factors_and_sums_boundary_ranks():
    m = tn.weight_mask(3, 1, dtype=F64)
    U = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=F64)   # mode 1 gets a third symbol: the sum of the two
    t = tn.Tensor(m.cores, Us=[None, U, None])
    assert torch.equal(tn.accepted_inputs(t), ac.dense_accepted(dense(t)))
    two = tn.Tensor([torch.cat([c, c], dim=0) if n == 0 else c for n, c in enumerate(m.cores)])   # boundary rank 2: twice the mask
    assert torch.equal(tn.accepted_inputs(two), ac.dense_accepted(2 * dense(m)))


@pytest.mark.parametrize("scale", [0.4, 0.5, -1.0, 1.5])
def test_accepted_inputs_refuses_what_is_not_a_count(scale):
    with pytest.raises(ValueError):
        tn.accepted_inputs(tn.weight_mask(5, 2) * scale)


def test_accepted_inputs_refuses_a_negative_child_count():
    x, y = tn.symbols(2)
    t = x - (x & y) * 2 + y * 2    # values 0, 2, 1, 1: fine
    assert tn.accepted_inputs(t).tolist() == [[0, 1], [0, 1], [1, 0], [1, 1]]
    with pytest.raises(ValueError):
        tn.accepted_inputs((~x & ~y) * 2 - (~x & y) + (x & y))   # values 2, -1, 0, 1: the prefix x = 0 counts 1 = 2 - 1


def test_documented_raises():
    with pytest.raises(NotImplementedError):
        tn.length(3)
    with pytest.raises(NotImplementedError):
        tn.automata.length(3)
    with pytest.raises(ValueError):
        tn.weight_mask(4, -1)
    with pytest.raises(ValueError):
        tn.weight_mask(4, [2, -1])
    with pytest.raises(ValueError):
        tn.weight_mask(4, 1, nsymbols=[2, 2, 2])
    with pytest.raises(ValueError):
        tn.weight_one_hot(4, nsymbols=[2, 2, 2, 2, 2])
    batched = tn.Tensor([torch.ones(2, 1, 2, 1), torch.ones(2, 1, 2, 1)], batch=True)
    with pytest.raises(ValueError):
        tn.accepted_inputs(batched)
    with pytest.raises(NotImplementedError):
        tn.accepted_inputs(tn.Tensor([torch.ones(2, 3), torch.ones(2, 3)]))   # CP cores
    with pytest.raises(ValueError):
        tn.accepted_inputs(torch.ones(2, 2))
    t = tn.rand([3, 3], ranks_tt=2)
    with pytest.raises(ValueError):
        tn.partialset(batched)
    with pytest.raises(ValueError):
        tn.partialset(tn.rand([3, 1, 3], ranks_tt=2))          # a mode of size 1
    with pytest.raises(ValueError):
        tn.partialset(t, 3)                                      # three differences of a mode of size 3
    with pytest.raises(ValueError):
        tn.partialset(t, 1, bounds=[[0, 1]])
    with pytest.raises(ValueError):
        tn.mask(batched, batched)
    with pytest.raises(NotImplementedError):
        t[t]   # mask keys stay out of scope


# ---------------------------------------------------------------------------------------------- the mirror of the kernels
@pytest.mark.parametrize("P, r, I, rn", [(1, 1, 1, 1), (5, 3, 2, 4), (65, 17, 3, 2), (257, 2, 5, 17)])
def test_mirror_level_against_brute_force(P, r, I, rn):
    L, core, fiber = ac.kernel_inputs(P, r, I, rn, F64, zero_rows=[0] if P > 1 else None)
    out = ac.level(_hostops, L, core, fiber, 3, 1, False)
    C = torch.einsum("pa,aib->pi", L, core).long()
    assert torch.equal(out["C"], C) and int(out["flag"]) == 0
    pairs = [(p, i) for p in range(P) for i in range(I) if C[p, i] > 0]
    assert out["idx"].tolist() == [p * I + i for p, i in pairs]
    assert torch.equal(out["Lnew"], torch.stack([L[p] @ core[:, i, :] for p, i in pairs]) if pairs else torch.zeros(0, rn, dtype=F64))
    assert out["cntnew"].tolist() == [int(C[p, i]) for p, i in pairs]
    assert out["offnew"].tolist() == (torch.cumsum(out["cntnew"], 0) - out["cntnew"]).tolist()
    col = [i for p, i in pairs for _ in range(int(C[p, i]))]
    assert out["Xs"][:, 1].tolist() == col and bool((out["Xs"][:, [0, 2]] == -5).all())
    last = ac.level(_hostops, L, core, fiber, 3, 1, True)
    assert last["Lnew"] is None and torch.equal(last["Xs"], out["Xs"]) and torch.equal(last["offnew"], out["offnew"])


def test_mirror_flags():
    L, core, fiber = ac.kernel_inputs(4, 3, 2, 2, F64)
    C = _hostops.accept_count(L, fiber)
    cnt = C.sum(1)
    off = torch.cumsum(cnt, 0) - cnt
    childoff = off[:, None] + torch.cumsum(C, 1) - C
    idx = torch.nonzero(C.reshape(-1) > 0).reshape(-1)

    def run(C=C, cnt=cnt, idx=idx):
        flag = torch.zeros(1, dtype=torch.int32)
        _hostops.accept_expand(L, core, C, childoff, cnt, idx, torch.zeros((int(cnt.sum()), 1), dtype=torch.int64), 0, flag, False)
        return int(flag)

    Cneg = C.clone()
    Cneg[0, 0], Cneg[0, 1] = -1, C[0].sum() + 1
    assert run() == 0
    assert run(C=Cneg) == _hostops.ACCEPT_NEGATIVE
    assert run(cnt=cnt + 1) == _hostops.ACCEPT_SUM_MISMATCH
    assert run(idx=torch.cat([idx, torch.tensor([8])])) == _hostops.ACCEPT_BAD_INDEX
    assert _hostops.accept_count(torch.full((1, 1), 1e300, dtype=F64), torch.full((1, 1), 1e10, dtype=F64)).tolist() == [[2 ** 53]]


# ---------------------------------------------------------------------------------------------- mask
def _golden_train(name, Us=None):
    return tn.Tensor(ac.golden_cores(name), Us=Us)


def test_mask_with_idxs_clamping_equals_the_reference():
    z = ac.fixture()
    t = _golden_train("mask_t")
    t.idxs = [torch.from_numpy(z["mask_idx{}".format(n)]) for n in range(3)]
    m = _golden_train("mask_m")
    out = tn.mask(t, m.clone())
    assert out.cores[0].dtype == F64
    # the entries: t[i, j, k] * m[min(idx_0[i], 1), min(idx_1[j], 1), min(idx_2[k], 1)]; integer cores: exact
    assert np.array_equal(dense(out), z["mask_out"]) and np.abs(z["mask_out"]).max() > 0
    sel = np.ix_(*[np.minimum(z["mask_idx{}".format(n)], 1) for n in range(3)])
    assert np.array_equal(dense(out), dense(t) * dense(m)[sel])
    lists = tn.Tensor(t.cores, idxs=[z["mask_idx{}".format(n)].tolist() for n in range(3)])   # idxs as lists
    assert np.array_equal(dense(tn.mask(lists, m)), dense(out))


def test_mask_selects_on_the_tucker_factor():
    x, y = tn.symbols(2, dtype=F64)
    U = torch.tensor([[1.0, 0.0], [0.0, 1.0]], dtype=F64)
    m = tn.Tensor((x | y).cores, Us=[U, None])
    g = torch.Generator().manual_seed(3)
    t = tn.Tensor([torch.randint(1, 4, (1, 4, 2), generator=g).double(), torch.randint(1, 4, (2, 3, 1), generator=g).double()])
    out = dense(tn.mask(t, m))
    keep = dense(x | y)[np.ix_([0, 1, 1, 1], [0, 1, 1])]
    assert np.array_equal(out, dense(t) * keep)


# ---------------------------------------------------------------------------------------------- partialset
def test_partialset_order_1_equals_the_reference():
    z = ac.fixture()
    t = _golden_train("pset_t")
    x = tn.symbols(3)[0]
    p = tn.partialset(t, 1, mask=x, bounds=z["pset_bounds"].tolist())
    assert p.shape == z["pset_out"].shape and all(np.array_equal(np.asarray(p.idxs[n]), z["pset_idx{}".format(n)]) for n in range(3))
    assert np.array_equal(dense(p), z["pset_out"]) and np.abs(z["pset_out"]).max() > 0   # integer cores, steps 0.5, 2, 0.5: exact


def _dense_partialset(D, orders, bounds=None, modes_allowed=None):
    """All mixed forward differences of the dense array D, stacked per mode as partialset does, zero where the total order is not
    in ``orders`` (or a differentiated mode is not in ``modes_allowed``)."""
    N, mo = D.ndim, max(orders)
    steps = [1.0 if bounds is None else (bounds[n][1] - bounds[n][0]) / (D.shape[n] - 1) for n in range(N)]
    out = D
    for n in range(N):
        stack = [out]
        for o in range(mo):
            stack.append(np.diff(stack[-1], axis=n) / steps[n])
        out = np.concatenate(stack, axis=n)
    ords = [np.concatenate([np.full(D.shape[n] - o, o) for o in range(mo + 1)]) for n in range(N)]
    total = sum(np.ix_(*ords))
    keep = np.isin(total, orders)
    if modes_allowed is not None:
        for n in range(N):
            if n not in modes_allowed:
                shape = [1] * N
                shape[n] = -1
                keep = keep & (ords[n].reshape(shape) == 0)
    return out, keep


@pytest.mark.parametrize("order", [2, [1, 2]])
def test_partialset_higher_orders_against_dense_differences(order):
    g = torch.Generator().manual_seed(5)
    t = tn.Tensor([torch.randint(0, 4, s, generator=g).double() for s in ((1, 8, 3), (3, 7, 3), (3, 6, 1))])   # integers: exact
    orders = order if isinstance(order, list) else [order]
    truth, keep = _dense_partialset(dense(t), orders)
    p = tn.partialset(t, order)
    assert p.shape == truth.shape == (8 + 7 + 6, 7 + 6 + 5, 6 + 5 + 4)
    got = dense(p)
    assert np.array_equal(got[~keep], np.zeros(int((~keep).sum())))                 # outside the mask: exact zeros
    assert np.array_equal(got[keep], truth[keep]) and np.abs(truth[keep]).max() > 0
    assert [int(i.max()) for i in p.idxs] == [2, 2, 2] and p.idxs[0].tolist() == [0] * 8 + [1] * 7 + [2] * 6
    # with bounds and a mask: the same step for both orders, only modes 1 and 2 differentiated
    x, y, z = tn.symbols(3)
    bounds = [[0, 14], [-3, 3], [0, 2.5]]   # steps 2, 1 and 0.5
    truth, keep = _dense_partialset(dense(t), orders, bounds, modes_allowed=[1, 2])
    got = dense(tn.partialset(t, order, mask=tn.only(y | z) | tn.only(y) | tn.only(z), bounds=bounds))
    assert np.array_equal(got[~keep], np.zeros(int((~keep).sum())))
    assert np.array_equal(got[keep], truth[keep])


# ---------------------------------------------------------------------------------------------- exports and documents
def test_exports_and_documents():
    from tntorch_amd import _hip

    assert tn.automata.__all__ == ["weight_mask", "weight_one_hot", "weight", "length", "accepted_inputs"]
    for name in tn.automata.__all__:
        assert getattr(tn, name) is getattr(tn.automata, name)
    for name in ("true", "false", "all", "none", "any", "one", "symbols", "relevant_symbols", "irrelevant_symbols", "only", "presence",
                 "absence", "is_tautology", "is_contradiction", "is_satisfiable", "implies", "equiv"):
        assert name in tn.logic.__all__ and getattr(tn, name) is getattr(tn.logic, name)
    assert "mask" in tn.tools.__all__ and tn.mask is tn.tools.mask
    assert "partialset" in tn.derivatives.__all__ and tn.partialset is tn.derivatives.partialset
    assert not hasattr(tn, "sum")
    for name in ("ttr_accept_count", "ttr_accept_expand", "ttr_accept_max_rank"):
        assert name in _hip.EXPORTED_SYMBOLS
    assert (_hip.ACCEPT_NEGATIVE, _hip.ACCEPT_SUM_MISMATCH, _hip.ACCEPT_BAD_INDEX) == (
        _hostops.ACCEPT_NEGATIVE, _hostops.ACCEPT_SUM_MISMATCH, _hostops.ACCEPT_BAD_INDEX)
    assert "ttr_accept.hip" in open(os.path.join(ac.ROOT, "tntorch_amd", "csrc", "Makefile")).read()
    design = open(os.path.join(ac.ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 18\.", design, flags=re.M) and "ttr_accept_expand" in design
    readme = open(os.path.join(ac.ROOT, "README.md")).read()
    assert "tn.accepted_inputs" in readme and "partialset" in readme and "stays out: it needs" not in readme
