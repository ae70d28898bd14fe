"""The moment family on device tensors (a real MI355X): the fixture values of tests/golden/moments_f32.npz under the bounds of
tests/test_moments_host.py (tests/moments_cases.py), in fp32 and fp64; device against CPU; and one call whose approximate path
meets a bond rank above 64 (the blocked QR of the rounding)."""
import pytest
import torch

import moments_cases as mc
import tntorch_amd as tn

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _on_device(v, dt):
    assert isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 and v.dtype == dt


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("q", sorted(mc.EXACT))
def test_exact_values(q, dt):
    v = mc.EXACT[q](tn, dt, DEV)
    _on_device(v, dt)
    mc.check_exact(q, v, dt)


@pytest.mark.parametrize("q", sorted(mc.APPROX))
def test_approximate_values_fp32(q):
    v = mc.APPROX[q](tn, torch.float32, DEV)
    _on_device(v, torch.float32)
    mc.check_approx(q, v)


@pytest.mark.parametrize("q", sorted(mc.TIGHT))
def test_eig_fp64_tight(q):
    v = mc.TIGHT[q](tn, torch.float64, DEV)
    _on_device(v, torch.float64)
    mc.check_tight(q, v)


@pytest.mark.parametrize("q", ["hsum_exact_M4", "rawm_k3", "varm"])
def test_device_and_cpu_agree_exact(q):
    for dt, bound in ((torch.float32, 1e-5), (torch.float64, 1e-12)):
        d, c = float(mc.EXACT[q](tn, dt, DEV)), float(mc.EXACT[q](tn, dt, "cpu"))
        print(q, dt, d, c)
        assert abs(d - c) < 2 * bound * abs(mc.truth(q))   # each side within `bound` of the truth


@pytest.mark.parametrize("q", ["hsum_eig_M3", "hsum_svd_M3", "rawm_k4", "norm_k3"])
def test_device_and_cpu_agree_approximate(q):
    d, c = float(mc.APPROX[q](tn, torch.float32, DEV)), float(mc.APPROX[q](tn, torch.float32, "cpu"))
    print(q, d, c)
    assert abs(d - c) <= 2 * mc.approx_bound(q)
    if q in mc.TIGHT:
        d, c = float(mc.TIGHT[q](tn, torch.float64, DEV)), float(mc.TIGHT[q](tn, torch.float64, "cpu"))
        assert abs(d - c) < 2e-9 * abs(mc.truth(q))


def test_one_mode_boundary_ranks_and_identities_on_device():
    v = mc.train("v", torch.float64, DEV)
    for alg, eps in (("exact", None), ("eig", 1e-12), ("svd", 1e-12)):
        out = tn.hadamard_sum([v, v, v], algorithm=alg, eps=eps)
        _on_device(out, torch.float64)
        assert abs(float(out) - mc.truth("v_hsum_exact_M3")) < 1e-12 * mc.truth("v_hsum_exact_M3")
    g = torch.Generator().manual_seed(2)
    t = tn.Tensor([torch.rand(2, 4, 3, generator=g, dtype=torch.float64).cuda(), torch.rand(3, 5, 2, generator=g, dtype=torch.float64).cuda(),
                   torch.rand(2, 3, 3, generator=g, dtype=torch.float64).cuda()])
    u = tn.Tensor([torch.rand(1, 4, 2, generator=g, dtype=torch.float64).cuda(), torch.rand(2, 5, 2, generator=g, dtype=torch.float64).cuda(),
                   torch.rand(2, 3, 2, generator=g, dtype=torch.float64).cuda()])
    ref = float(tn.dot(t, u))
    for alg, eps in (("exact", None), ("eig", 1e-13)):
        assert abs(float(tn.hadamard_sum([t, u], algorithm=alg, eps=eps)) - ref) < 1e-10 * abs(ref), alg
    a = mc.train("a", torch.float64, DEV)
    n2 = float(tn.normsq(a))
    assert abs(float(tn.raw_moment(a, 2, algorithm="exact")) * float(a.numel()) - n2) < 1e-12 * n2
    assert abs(float(a.std()) ** 2 - float(a.var())) < 1e-12 * float(a.var())


def test_bond_rank_above_64_inside_the_approximate_path():
    """A 3-mode 9 x 9 x 9 train of rank 9 with M = 3: the products of the second and third mode have bonds of up to
    9 * 9 = 81 > 64 before their rounding (asserted on the ranks the rounding is given).  fp32 bound against the dense truth."""
    from tntorch_amd import _hipops

    g = torch.Generator().manual_seed(9)
    cores = [torch.rand(1, 9, 9, generator=g), torch.rand(9, 9, 9, generator=g), torch.rand(9, 9, 1, generator=g)]
    d = torch.einsum("aib,bjc,ckd->ijk", *[c.double() for c in cores])
    truth = float((d**3).sum())
    t = tn.Tensor([c.cuda() for c in cores])
    seen = []
    real = _hipops.round_tt

    def spy(c, *args, **kw):
        seen.append(max(max(x.shape[1], x.shape[3]) for x in c))
        return real(c, *args, **kw)

    _hipops.round_tt = spy
    try:
        v = tn.hadamard_sum([t, t, t], algorithm="eig", eps=1e-6)
    finally:
        _hipops.round_tt = real
    _on_device(v, torch.float32)
    assert max(seen) > 64, seen
    err = abs(float(v) - truth) / truth
    print("bonds seen", seen, "value", float(v), "truth", truth, "rel. error", err)
    assert err < 1e-5, err
