"""``tn.tt_apply`` / ``tn.tt_matmul`` / ``tn.tt_transpose`` on device tensors (a real MI355X) against fp64 CPU contractions that
are independent of the package, within the derived chain bound of algebra_cases; rounding, one explicit Euler step, and the
grad-mode refusals.  Results live on the device in the input dtype."""
import pytest
import torch

import algebra_cases as ac
import matrix_cases as mc
import tntorch_amd as tn

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
DTYPES = [F32, F64]


def _dev(cores):
    return [c.to(DEV) for c in cores]


def _matrix(G, idims, odims):
    return tn.TTMatrix(_dev(G), None, idims, odims)


def _on_device(t, dt):
    cores = t.cores
    assert all(c.is_cuda and c.dtype == dt for c in cores)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ac.CASES)
def test_products_against_the_truth(name, dt):
    G, T, U, idims, odims = ac.case(name, dt)
    M = _matrix(G, idims, odims)
    y = tn.tt_apply(M, tn.Tensor(_dev(T)))
    _on_device(y, dt)
    assert isinstance(y, tn.Tensor) and tuple(y.shape) == tuple(odims)
    assert y.ranks_tt.tolist() == [1] + [int(a.shape[-1]) * int(g.shape[-1]) for a, g in zip(T, G)]
    y64, bound = ac.apply_truth_and_bound(G, T, dt)
    mc.assert_within(y.torch().reshape(-1), y64, bound, "tt_apply {} {}".format(name, dt))

    z = tn.tt_apply(M, tn.Tensor(_dev(U)), transpose=True)
    _on_device(z, dt)
    assert tuple(z.shape) == tuple(idims)
    z64, bound = ac.apply_truth_and_bound(G, U, dt, transpose=True)
    mc.assert_within(z.torch().reshape(-1), z64, bound, "tt_apply transpose {} {}".format(name, dt))

    P = tn.tt_matmul(M, tn.tt_transpose(M))
    _on_device(P, dt)
    assert isinstance(P, tn.TTMatrix) and P.input_dims.tolist() == list(idims) and P.output_dims.tolist() == list(idims)
    p64, bound = ac.matmul_truth_and_bound(G, ac.transposed(G), dt)
    mc.assert_within(P.torch(), p64, bound, "tt_matmul {} {}".format(name, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ac.CASES)
def test_agrees_with_tt_multiply(name, dt):
    """Both are within their derived bounds of the same truth (test_algebra_host.py: the sum of the bounds)."""
    G, T, _, idims, odims = ac.case(name, dt)
    M, t = _matrix(G, idims, odims), tn.Tensor(_dev(T))
    got = tn.tt_apply(M, t).torch().reshape(-1)
    x = t.torch().reshape(1, -1)
    want = tn.tt_multiply(M, x)[0]
    assert got.is_cuda and want.is_cuda
    _, b1 = ac.apply_truth_and_bound(G, T, dt)
    _, b2 = mc.tt_truth_and_bound(G, x, dt)
    mc.assert_within(got, want.double().cpu(), b1 + b2[0] + b1, "tt_apply against tt_multiply {} {}".format(name, dt))


def test_identity_operator_returns_the_cores_bit_for_bit():
    dims = [4, 3, 5]
    T = ac.train_cores(dims, [3, 2], F32)
    eye = tn.TTMatrix([torch.eye(n, dtype=F32, device=DEV).reshape(1, n, n, 1) for n in dims], None, dims, dims)
    for transpose in (False, True):
        out = tn.tt_apply(eye, tn.Tensor(_dev(T)), transpose=transpose)
        for a, b in zip(out.cores, T):
            assert torch.equal(a.cpu(), b)


def test_rounded_eps_fp64():
    G, T, _, idims, odims = ac.case("three", F64)
    M = _matrix(G, idims, odims)
    y64, _ = ac.apply_truth_and_bound(G, T, F64)
    out = tn.tt_apply(M, tn.Tensor(_dev(T)), eps=1e-6)
    _on_device(out, F64)
    err = ac.rel_err(out.torch().reshape(-1).cpu().numpy(), y64.numpy())
    print("tt_apply eps = 1e-6 fp64: relative error", err, "ranks", out.ranks_tt.tolist())
    assert err <= 1e-6 + 1e-12
    p64, _ = ac.matmul_truth_and_bound(G, ac.transposed(G), F64)
    P = tn.tt_matmul(M, tn.tt_transpose(M), eps=1e-6)
    _on_device(P, F64)
    err = ac.rel_err(P.torch().cpu().numpy(), p64.numpy())
    print("tt_matmul eps = 1e-6 fp64: relative error", err, "ranks", [c.shape[-1] for c in P.cores])
    assert err <= 1e-6 + 1e-12 and P.cores[0].shape[-1] <= 16 and all(c.dim() == 4 for c in P.cores)


def test_rounded_rmax_fp32():
    """M @ vec(u) has product ranks [21, 10]; rmax = 4 truncates.  Bound: twice the error that round_tt of the host mirror's
    exact train gives on the CPU in the same dtype (rank-rule noise can pick a neighbouring subspace), as for convolve; both
    figures are printed."""
    G, _, U, idims, odims = ac.case("three", F32)
    z64, _ = ac.apply_truth_and_bound(G, U, F32, transpose=True)
    host = tn.tt_apply(tn.TTMatrix(list(G), None, idims, odims), tn.Tensor(U), transpose=True)
    host.round_tt(eps=0, rmax=4)
    bound = 2 * ac.rel_err(host.torch().reshape(-1).numpy(), z64.numpy())
    out = tn.tt_apply(_matrix(G, idims, odims), tn.Tensor(_dev(U)), transpose=True, rmax=4)
    _on_device(out, F32)
    assert out.ranks_tt.tolist() == [1, 4, 4, 1]
    err = ac.rel_err(out.torch().reshape(-1).cpu().numpy(), z64.numpy())
    print("rmax = 4 fp32: relative error", err, "bound (2 x the CPU's)", bound)
    assert 0 < bound and err <= bound


def test_one_euler_step():
    """u <- round(u + 0.1 tt_apply(A, u), eps = 1e-6) in fp64 against the dense computation: round_tt's bound on the relative error, plus
    1e-12 for the exact part."""
    dims = [4, 3, 5]
    g = torch.Generator().manual_seed(21)
    G = [torch.randn((r0, n, n, r1), dtype=F64, generator=g) for (r0, n, r1) in zip([1, 3, 2], dims, [3, 2, 1])]
    T = ac.train_cores(dims, [3, 2], F64, seed=22)
    A, u = _matrix(G, dims, dims), tn.Tensor(_dev(T))
    step = u + 0.1 * tn.tt_apply(A, u)
    step.round_tt(eps=1e-6)
    _on_device(step, F64)
    v = ac.train_dense(T)
    want = v + 0.1 * (v @ mc.tt_dense(G))
    err = ac.rel_err(step.torch().reshape(-1).cpu().numpy(), want.numpy())
    print("one Euler step: relative error", err, "ranks", step.ranks_tt.tolist())
    assert err <= 1e-6 + 1e-12
    assert max(step.ranks_tt.tolist()) <= 5     # the unfoldings of a 4 x 3 x 5 tensor


def test_grad_mode_refusals_and_the_ways_around_them():
    G, T, _, idims, odims = ac.case("three", F64)
    y64, bound = ac.apply_truth_and_bound(G, T, F64)
    Gd, Td = _dev(G), _dev(T)
    Gg = [Gd[0], Gd[1].clone().requires_grad_(True), Gd[2]]
    Tg = [Td[0], Td[1], Td[2].clone().requires_grad_(True)]
    M, Mg = tn.TTMatrix(Gd, None, idims, odims), tn.TTMatrix(Gg, None, idims, odims)
    t, tg = tn.Tensor(Td), tn.Tensor(Tg)
    msg = "not differentiable on the device.*detach the cores or use CPU tensors"
    with pytest.raises(NotImplementedError, match=msg):
        tn.tt_apply(Mg, t)
    with pytest.raises(NotImplementedError, match=msg):
        tn.tt_apply(M, tg)
    with pytest.raises(NotImplementedError, match=msg):
        tn.tt_apply(Mg, tn.Tensor(_dev(ac.case("three", F64)[2])), transpose=True)
    with pytest.raises(NotImplementedError, match=msg):
        tn.tt_matmul(Mg, tn.tt_transpose(M))
    with pytest.raises(NotImplementedError, match=msg):
        tn.tt_matmul(M, tn.tt_transpose(Mg))
    with torch.no_grad():
        y = tn.tt_apply(Mg, tg)
        P = tn.tt_matmul(Mg, tn.tt_transpose(Mg))
    assert not any(c.requires_grad for c in y.cores) and not any(c.requires_grad for c in P.cores)
    mc.assert_within(y.torch().reshape(-1), y64, bound, "under no_grad")
    detached = tn.tt_apply(tn.TTMatrix([c.detach() for c in Gg], None, idims, odims), tn.Tensor([c.detach() for c in Tg]))
    for a, b in zip(detached.cores, y.cores):
        assert torch.equal(a, b)
    assert Gg[1].requires_grad and Tg[2].requires_grad      # the operands are as they were


def test_refuses_different_devices_and_dtypes():
    G, T, _, idims, odims = ac.case("three", F64)
    M = _matrix(G, idims, odims)
    with pytest.raises(ValueError, match="same device"):
        tn.tt_apply(M, tn.Tensor(T))
    with pytest.raises(ValueError, match="same device"):
        tn.tt_matmul(M, tn.tt_transpose(tn.TTMatrix(list(G), None, idims, odims)))
    with pytest.raises(ValueError, match="same dtype"):
        tn.tt_apply(M, tn.Tensor(_dev([c.float() for c in T])))
