"""``tntorch_amd.patch(tntorch)`` on a class shaped like the reference's own: the bodies of the reference's
tests/test_round.py:7-68 run through the patched methods.  The patched object is a minimal stand-in with the reference's
attributes (tensor.py:107-209) whose own methods refuse to run, so every call the bodies make lands in this package: CPU cores
on the host mirror, device cores on the HIP kernels.  What the reference itself answers (its unpatched round_tt, its reduce
tree) comes from tests/golden/patch_reference_f64.npz, recorded by oracle/gen_golden.py."""
import types

import numpy as np
import pytest
import torch

import oracle
import tntorch_amd as tna
from parity import load_case


class _RefLike:
    """The attributes / construction the reference's Tensor exposes on this path (tensor.py:107-209), plus the helpers the
    reference's tests use around the patched methods (``clone``, ``dim``, ``ranks_tt``, ``torch``, ``+``, scalar ``/``)."""

    def __init__(self, cores, Us=None, idxs=None, batch=False):
        self.cores = list(cores)
        self.Us = [None] * len(cores) if Us is None else list(Us)
        self.idxs = idxs
        self.batch = batch

    @classmethod
    def _of(cls, t):
        return cls(t.cores, t.Us, t.idxs, t.batch)

    def _ours(self):
        return tna.Tensor(list(self.cores), Us=list(self.Us), idxs=self.idxs, batch=self.batch)

    def clone(self):
        return _RefLike([c.clone() for c in self.cores], [None if U is None else U.clone() for U in self.Us], self.idxs, self.batch)

    def dim(self):
        return len(self.cores)

    @property
    def ranks_tt(self):
        return self._ours().ranks_tt

    def torch(self):
        return self._ours().torch()

    def __add__(self, other):
        return _RefLike._of(self._ours() + other._ours())

    def __truediv__(self, s):
        return _RefLike._of(self._ours() / s)

    # unpatched placeholders (the reference's own methods would sit here)
    def round_tt(self, *a, **k):
        raise AssertionError("unpatched")

    orthogonalize = left_orthogonalize = right_orthogonalize = round_tucker = round = factor_orthogonalize = round_tt


def _unpatched_truncated_svd(*a, **k):
    raise AssertionError("unpatched")


def _stand_in_module():
    """The names of the reference module the test bodies reach: ``Tensor`` and ``truncated_svd`` (what ``patch`` rebinds),
    ``rand``, ``relative_error`` and the free ``round_tt`` (round.py:7-19: clone, then the method)."""

    def rand(shape, ranks_tt=None, ranks_tucker=None):
        if ranks_tt is None and ranks_tucker is None:
            ranks_tucker = [None] * len(shape)  # the reference's default: full TT ranks (create.py:243-272)
        return _RefLike._of(tna.rand(shape, ranks_tt=ranks_tt, ranks_tucker=ranks_tucker))

    def relative_error(gt, approx):
        a, b = gt.torch(), approx.torch()
        return (a - b).norm() / a.norm()

    def round_tt(t, *a, **k):
        t = t.clone()
        t.round_tt(*a, **k)
        return t

    return types.SimpleNamespace(Tensor=_RefLike, truncated_svd=_unpatched_truncated_svd, rand=rand,
                                 relative_error=relative_error, round_tt=round_tt)


@pytest.fixture()
def ref_tn():
    tn = _stand_in_module()
    saved = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # tests/test_round.py:4
    undo = tna.patch(tn)
    yield tn
    undo()
    torch.set_default_dtype(saved)


def test_patch_installs_and_uninstalls(ref_tn):
    tn = ref_tn
    assert hasattr(tn.Tensor.round_tt, "_tntorch_amd_original") and tn.truncated_svd is tna.truncated_svd
    first = tn.Tensor.round_tt
    undo2 = tna.patch(tn)  # idempotent: an already patched module is left alone and the SAME undo comes back
    assert tn.Tensor.round_tt is first
    undo2()
    assert not hasattr(tn.Tensor.round_tt, "_tntorch_amd_original") and tn.truncated_svd is not tna.truncated_svd
    undo2()  # a second undo is a no-op
    assert not hasattr(tn.Tensor.round_tt, "_tntorch_amd_original")
    undo3 = tna.patch(tn)  # (the fixture's undo is the first one: a no-op by now, so restore here)
    assert hasattr(tn.Tensor.round_tt, "_tntorch_amd_original")
    undo3()
    tna.patch(tn)  # leave the module patched for the fixture's teardown ... which holds the FIRST undo (no-op): undo below
    tna._patch._ACTIVE[id(tn)][1]()


def test_reference_orthogonalization_body(ref_tn):
    """tests/test_round.py:7-19 through the patched methods (20 random trains instead of 100)."""
    tn = ref_tn
    np.random.seed(0)
    torch.manual_seed(0)
    for _ in range(20):
        gt = tn.rand(np.random.randint(1, 8, np.random.randint(2, 6)))
        t = gt.clone()
        held = list(t.cores)
        snap = [c.clone() for c in held]
        assert tn.relative_error(gt, t) <= 1e-7
        t.left_orthogonalize(0)
        assert tn.relative_error(gt, t) <= 1e-7
        t.right_orthogonalize(t.dim() - 1)
        assert tn.relative_error(gt, t) <= 1e-7
        t.orthogonalize(np.random.randint(t.dim()))
        assert tn.relative_error(gt, t) <= 1e-7
        assert all(torch.equal(a, b) for a, b in zip(held, snap))  # rebinding: the old core tensors were never written


@pytest.mark.parametrize("alg", ["svd", "eig"])
def test_reference_truncated_svd_body(ref_tn, alg):
    """tests/test_round.py:22-39: batch == loop."""
    tn = ref_tn
    torch.manual_seed(1)
    gt = torch.rand((2, 32, 32))
    u, v = tn.truncated_svd(gt, batch=True, algorithm=alg)
    for i in range(len(gt)):
        u1, v1 = tn.truncated_svd(gt[i], batch=False, algorithm=alg)
        assert torch.allclose(u1, u[i]) and torch.allclose(v1, v[i])


@pytest.mark.parametrize("alg,tol", [("svd", 1e-4), ("eig", 1e-7)])
def test_reference_round_tt_body(ref_tn, alg, tol):
    """tests/test_round.py:41-59 (10 trains instead of 100)."""
    tn = ref_tn
    np.random.seed(2)
    torch.manual_seed(2)
    for _ in range(10):
        gt = tn.rand(np.random.randint(1, 8, np.random.randint(8, 10)), ranks_tt=np.random.randint(1, 10))
        gt.round_tt(1e-8, algorithm=alg)
        t = gt + gt
        t.round_tt(1e-8, algorithm=alg)
        assert tn.relative_error(gt, t / 2) <= tol
        if alg == "svd":
            assert max(gt.ranks_tt) == max(t.ranks_tt)
        t2 = tn.round_tt(gt + gt, eps=1e-8, algorithm=alg)  # free function: clone + patched method (round.py:7-19)
        assert tn.relative_error(gt, t2 / 2) <= tol


def test_reference_round_tucker_body(ref_tn):
    """tests/test_round.py:62-68 (5 tensors instead of 100)."""
    tn = ref_tn
    np.random.seed(3)
    torch.manual_seed(3)
    for _ in range(5):
        eps = np.random.rand() ** 2
        gt = tn.rand([32] * 4, ranks_tt=8, ranks_tucker=8)
        t = gt.clone()
        t.round_tucker(eps=eps)
        assert tn.relative_error(gt, t) <= eps


def test_patched_result_equals_unpatched(ref_tn):
    """Same input through the patched class and through the reference's own method (its output recorded): identical ranks,
    same tensor."""
    tn = ref_tn
    g = load_case("patch_reference_f64")
    a = tn.Tensor(g["unpatched_inp"])
    a.round_tt(eps=1e-8)                                        # patched (host mirror)
    b = g["unpatched_out"]                                      # the reference's own method
    assert list(a.ranks_tt) == oracle.tt_ranks(b)
    ref = oracle.tt_to_dense(b)
    assert (a.torch() - ref).norm() / ref.norm() < 1e-12


# ------------------------------------------------------------------ device cores under the stand-in class
@pytest.mark.gpu
def test_patch_on_device_cores():
    mod = types.SimpleNamespace(Tensor=_RefLike, truncated_svd=None)
    undo = tna.patch(mod)
    try:
        torch.manual_seed(5)
        g = oracle.tt_randn([8, 9, 7, 8, 6], 5, dtype=torch.float64)
        inp = oracle.tt_add(g, g)
        t = _RefLike([c.cuda() for c in inp])
        held = list(t.cores)
        snap = [c.clone() for c in held]
        t.round_tt(eps=1e-8)
        assert [c.shape[-1] for c in t.cores] == [5, 5, 5, 5, 1] and all(c.is_cuda for c in t.cores)
        ref = oracle.round_tt(inp, eps=1e-8)
        a = oracle.tt_to_dense([c.cpu() for c in t.cores])
        b = oracle.tt_to_dense(ref)
        assert (a - b).norm() / b.norm() < 1e-10
        assert all(torch.equal(x, y) for x, y in zip(held, snap))
        t2 = _RefLike([c.cuda() for c in inp])
        t2.orthogonalize(2)
        a2 = oracle.tt_to_dense([c.cpu() for c in t2.cores])
        assert (a2 - oracle.tt_to_dense(inp)).norm() / a2.norm() < 1e-12
        M = torch.rand(40, 90, dtype=torch.float64).cuda()
        L, R = mod.truncated_svd(M, eps=1e-3)
        assert ((L @ R) - M).norm() / M.norm() <= 1e-3
    finally:
        undo()
    with pytest.raises(AssertionError):
        _RefLike([torch.zeros(1, 2, 1)]).round_tt()


def test_reduce_tree_matches_reference_order():
    """tools.reduce (own implementation) builds the same tree and hands the operands over in the same order as
    tools.py:460-512: checked with a non-commutative combiner on 1..9 tensors against the reference's recorded results."""
    g = load_case("patch_reference_f64")
    for count in range(1, 10):
        cores = [g[f"reduce{count}_t{j}"] for j in range(count)]

        def comb(a, b):
            return a + b * 2.0  # order-sensitive: every tree shape / operand order gives different weights

        ref = g[f"reduce{count}_dense"]
        ours = tna.reduce((tna.Tensor([c.clone() for c in cs]) for cs in cores), comb, eps=1e-12)  # a generator works too
        assert (ours.torch() - ref).norm() / ref.norm() < 1e-10, count
    with pytest.raises(ValueError):
        tna.reduce([], comb)
