"""``tntorch_amd/anova.py`` on CPU tensors (the host mirror) against tests/golden/anova_f64.npz: the reference's results and a
dense brute-force ANOVA (tools/gen_anova_golden.py)."""
import numpy as np
import pytest
import torch

import anova_cases as ac
import tntorch_amd as tn
from tntorch_amd import _hostops

F64 = torch.float64


@pytest.mark.parametrize("q", sorted(ac.CASES))
def test_golden_fp64(q):
    """Every case of the fixture within 1e-10 (absolute; the indices lie in [0, N]) of the brute-force truth."""
    r = ac.CASES[q](tn, F64, "cpu")
    err = ac.abs_err(r, q)
    print(q, "abs. error", err, "reference's", float(np.abs(ac.fixture()["ref_" + q] - ac.truth(q)).max()))
    assert err < 1e-10, (q, err)


def test_result_types():
    t, w = ac.train("t", F64), ac.marginals(F64)
    s = tn.sobol(t, ac.train("mask_x0", F64), w)
    assert isinstance(s, torch.Tensor) and s.dim() == 0 and s.dtype == F64
    v = tn.sobol(t, ac.train("mask_one_hot", F64), w)
    assert isinstance(v, tn.Tensor) and v.dim() == 1 and tuple(v.shape) == (5,)
    d = tn.dimension_distribution(t, marginals=w)
    assert isinstance(d, torch.Tensor) and tuple(d.shape) == (4,)
    s32 = tn.sobol(ac.train("t", torch.float32), ac.train("mask_x0", torch.float32), ac.marginals(torch.float32))
    assert s32.dtype == torch.float32
    assert abs(float(s32) - float(ac.truth("sobol_x0"))) < 1e-4


def test_package_masks_match_the_stored_ones():
    """The masks a user builds with this package give what the stored cores of the reference's masks give."""
    t, w = ac.train("t", F64), ac.marginals(F64)
    x = tn.symbols(4, dtype=F64)
    built = {"only_x0": tn.only(x[0]), "x0": x[0], "x0_not_x2": x[0] & ~x[2], "weight": tn.weight(4, dtype=F64),
             "one_hot": tn.weight_one_hot(4, 5, dtype=F64), "true": tn.true(4, dtype=F64)}
    for name, m in built.items():
        assert ac.abs_err(tn.sobol(t, m, w), "sobol_" + name) < 1e-10, name


def test_leading_ranks_are_summed_away():
    """A train whose first core has leading rank 2 is the sum of its two rows, as ``tn.dot`` reads it."""
    t = ac.train("t", F64)
    g = torch.Generator().manual_seed(5)
    extra = torch.rand(1, 3, 3, generator=g, dtype=F64)
    two = tn.Tensor([torch.cat([t.cores[0], extra])] + [c.clone() for c in t.cores[1:]])
    one = tn.Tensor([t.cores[0] + extra] + [c.clone() for c in t.cores[1:]])
    m, w = ac.train("mask_x0_not_x2", F64), ac.marginals(F64)
    assert abs(float(tn.sobol(two, m, w)) - float(tn.sobol(one, m, w))) < 1e-12


@pytest.mark.parametrize("name", ["t", "k"])
def test_anova_decomposition_round_trip(name):
    t = ac.train(name, F64)
    w = ac.marginals(F64, prefix="marg" if name == "t" else "kmarg")
    for marg in (None, w):
        a = tn.anova_decomposition(t, marg)
        for n, I in enumerate(t.shape):
            cols = I if t.Us[n] is None else t.Us[n].shape[1]
            assert tuple(a.Us[n].shape) == (I + 1, cols)
            assert list(a.idxs[n]) == [0] + [1] * I
            assert a.cores[n] is not t.cores[n] and torch.equal(a.cores[n], t.cores[n])
        assert tuple(a.shape) == tuple(I + 1 for I in t.shape)
        back = tn.undo_anova_decomposition(a)
        full = t.torch()
        assert float((back.torch() - full).abs().max()) <= 1e-12 * float(full.abs().max())
    # slice 0 of every mode is the mean under the marginals
    ws = [m / m.sum() for m in w]
    mean = t.torch()
    for n in range(t.dim() - 1, -1, -1):
        mean = torch.tensordot(mean, ws[n], dims=([n], [0]))
    assert abs(float(tn.anova_decomposition(t, w)[(0,) * t.dim()]) - float(mean)) < 1e-12 * abs(float(mean))


def test_truncate_anova():
    """``only(x1)`` does not accept the empty tuple, so the reference's ``truncate_anova(t, only(x1))`` is the first-order term of
    x1 WITHOUT the mean (the fixture's generator asserts it, 1e-15); the mean plus that term is the mask ``only(x1) | none(4)``.
    Both are compared with the brute-force terms."""
    t = ac.train("t", F64)
    x = tn.symbols(4, dtype=F64)
    one = tn.truncate_anova(t, tn.only(x[1]))
    assert one.dim() == 1 and tuple(one.shape) == (4,)
    assert ac.rel_err(one, "truncate_only_x1") < 1e-12
    keep = tn.truncate_anova(t, tn.only(x[1]), keepdim=True)
    assert tuple(keep.shape) == tuple(t.shape)
    assert ac.rel_err(keep, "truncate_only_x1_keepdim") < 1e-12
    assert ac.rel_err(tn.truncate_anova(t, tn.only(x[1]), marginals=ac.marginals(F64)), "truncate_only_x1_marg") < 1e-12
    # the mean plus the first-order term: the mask has to accept the empty tuple too
    both = tn.truncate_anova(t, tn.only(x[1]) | tn.none(4, dtype=F64))
    assert both.dim() == 1 and ac.rel_err(both, "truncate_only_x1_or_none") < 1e-12
    assert ac.rel_err(tn.truncate_anova(t, tn.only(x[1]) | tn.none(4, dtype=F64), marginals=ac.marginals(F64)),
                      "truncate_only_x1_or_none_marg") < 1e-12


def test_refusals():
    t, m, w = ac.train("t", F64), ac.train("mask_x0", F64), ac.marginals(F64)
    batched = tn.Tensor([c[None].clone() for c in t.cores], batch=True)
    cp = tn.Tensor([torch.rand(I, 2, dtype=F64) for I in t.shape])
    calls = {
        "sobol": lambda x, **kw: tn.sobol(x, m, **kw),
        "mean_dimension": lambda x, **kw: tn.mean_dimension(x, **kw),
        "dimension_distribution": lambda x, **kw: tn.dimension_distribution(x, **kw),
        "anova_decomposition": lambda x, **kw: tn.anova_decomposition(x, **kw),
        "truncate_anova": lambda x, **kw: tn.truncate_anova(x, m, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError):
            call(batched)
        with pytest.raises(NotImplementedError):
            call(cp)
        with pytest.raises(ValueError):
            call(t.torch())                         # not a Tensor
        with pytest.raises(ValueError):
            call(t, marginals=w[:3])                # wrong length
        with pytest.raises(ValueError):
            call(t, marginals=[w[1], w[1], w[2], w[3]])   # 4 entries for a mode of 3
    with pytest.raises(ValueError):
        tn.undo_anova_decomposition(t.torch())
    with pytest.raises(ValueError):
        tn.undo_anova_decomposition(batched)
    short = ac.train("kmask_x0", F64)               # a mask over 2 variables
    for call in (lambda: tn.sobol(t, short), lambda: tn.mean_dimension(t, mask=short), lambda: tn.dimension_distribution(t, mask=short),
                 lambda: tn.truncate_anova(t, short)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        tn.sobol(t, m.torch())
    with pytest.raises(ValueError):
        tn.dimension_distribution(t, order=0)


def test_marginals_are_not_modified():
    t, m = ac.train("t", F64), ac.train("mask_weight", F64)
    w = ac.marginals(F64)
    before = [x.clone() for x in w]
    tn.sobol(t, m, w)
    tn.mean_dimension(t, marginals=w)
    tn.dimension_distribution(t, marginals=w)
    tn.anova_decomposition(t, w)
    tn.truncate_anova(t, ac.train("mask_only_x0", F64), marginals=w)
    for a, b in zip(w, before):
        assert torch.equal(a, b) and a.dtype == b.dtype


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("given", [True, False], ids=["w_mu", "null"])
@pytest.mark.parametrize("shape", ac.SANDWICH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_mode_sandwich(shape, given, dtype):
    """The host mirror against the fp64 einsum: 5e-6 (fp32) / 1e-12 (fp64) of the reference's largest entry."""
    Z, A, w, mu = (x.to(dtype) for x in ac.sandwich_inputs(shape))
    Q = _hostops.mode_sandwich(Z, A, w if given else None, mu if given else None)
    ref = ac.sandwich_reference(shape, given)
    assert Q.dtype == dtype and tuple(Q.shape) == tuple(ref.shape)
    err = float((Q.double() - ref).abs().max() / ref.abs().max())
    print(shape, given, dtype, "rel. error", err)
    assert err < (5e-6 if dtype == torch.float32 else 1e-12)
