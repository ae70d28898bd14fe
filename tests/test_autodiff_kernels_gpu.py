"""ttr_gather_grad alone, against an fp64 sum on the CPU of the same dtype-rounded inputs.

Shapes (r0, r1): boundary cores, both sides of a 16-wide MFMA tile, both sides of the kernel's 64 x 64 workgroup tile, and the rank
limit.  Every case runs slices with 0, 1, 2 and 3 tasks whose lengths are 0, 1, 3, 4, 5, S - 1, S, S + 1 and 2 S + 1 for the shape's
own staging depth S (the rule is restated in ``stage_rows`` below and compared with the library's), over a shuffled permutation with
samples that belong to no task, and row strides above r0 / r1.

Tolerance per element: n eps sum_p |L[p, a]| |R[p, b]| with n the slice's sample count and eps = 2^-23 / 2^-52: twice the classical
bound gamma_n of a sum of n products in any order, the factor 2 covering the reference's own fp64 rounding.  Nothing is measured.

Bitwise: empty slices and empty tasks are exact zeros, strided and contiguous operands and two calls give equal bits, and the canary
elements around dG and the workspace stay untouched."""
import pytest
import torch

from tntorch_amd import _hip, _hipops, _hostops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
EPS = {torch.float64: 2.0 ** -52, torch.float32: 2.0 ** -23}
F64 = torch.float64
SHAPES = [(1, 1), (1, 16), (1, 17), (17, 1), (4, 4), (5, 33), (31, 33), (64, 64), (65, 16), (63, 65), (80, 80), (512, 2), (2, 512)]


def stage_width(r):
    """Staged row width of a tile side: the live columns (at most 64) rounded up to 16, made 16 mod 32."""
    return min(64, -(-r // 16) * 16) | 16


def stage_rows(r0, r1, dtype):
    """Samples per staging pass: what fits in 48 KiB next to one int64 id per sample, at most 256, a multiple of 4."""
    es = 4 if dtype == torch.float32 else 8
    return min(256, (48 * 1024) // ((stage_width(r0) + stage_width(r1)) * es + 8)) & ~3


def layout(S):
    """(task lengths per slice): slice 0 has no task, slice 3 one empty task, slices 2, 4 three tasks, slice 5 two."""
    return [[], [S + 1], [3, 0, 2 * S + 1], [0], [1, 4, 5], [S - 1, S]]


def build_case(r0, r1, dtype, seed):
    S = stage_rows(r0, r1, dtype)
    g = torch.Generator().manual_seed(seed)
    slices = layout(S)
    lens = [n for sl in slices for n in sl]
    P = sum(lens) + 5  # five samples belong to no task
    Lw = torch.randn(P, r0 + 3, generator=g, dtype=F64).to(dtype)
    Rw = torch.randn(P, r1 + 2, generator=g, dtype=F64).to(dtype)
    perm = torch.randperm(P, generator=g)
    te = torch.tensor(lens).cumsum(0)
    tb = te - torch.tensor(lens)
    toff = torch.tensor([0] + [len(sl) for sl in slices]).cumsum(0)
    return S, slices, Lw, Rw, perm, tb, te, toff


def reference(L, R, perm, tb, te, toff):
    """(dG, bound / (n eps)) in fp64: per slice, the sum over the samples of its tasks."""
    I = toff.shape[0] - 1
    L, R = L.double(), R.double()
    ref = torch.zeros(L.shape[1], I, R.shape[1], dtype=F64)
    mag = torch.zeros_like(ref)
    count = []
    for i in range(I):
        q = torch.cat([perm[int(tb[t]):int(te[t])] for t in range(int(toff[i]), int(toff[i + 1]))] + [perm[:0]])
        ref[:, i, :] = L[q].T @ R[q]
        mag[:, i, :] = L[q].abs().T @ R[q].abs()
        count.append(len(q))
    return ref, mag, count


def test_stage_rule_matches_the_library():
    for dtype in DTYPES:
        for r0, r1 in SHAPES + [(512, 512), (16, 16), (32, 48)]:
            S = stage_rows(r0, r1, dtype)
            assert S >= 4 and S % 4 == 0 and S == _hip.gather_grad_stage_rows(dtype, r0, r1), (r0, r1, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r0,r1", SHAPES)
def test_gather_grad_task_edges_strides_canaries(r0, r1, dtype):
    S, slices, Lw, Rw, perm, tb, te, toff = build_case(r0, r1, dtype, 1000 * r0 + r1)
    I, T = len(slices), int(toff[-1])
    L, R = Lw[:, 2:2 + r0], Rw[:, 1:1 + r1]
    Ld, Rd = Lw.to(DEV)[:, 2:2 + r0], Rw.to(DEV)[:, 1:1 + r1]
    assert Ld.stride(0) == r0 + 3 and Rd.stride(0) == r1 + 2
    args = (perm.to(DEV), tb.to(DEV), te.to(DEV), toff.to(DEV))
    n, pad = r0 * I * r1, 64
    wsb = int(_hip.lib().ttr_gather_grad_workspace_bytes(_hip.dtype_code(dtype), T, r0, r1))
    assert wsb == T * r0 * r1 * Ld.element_size()
    buf = torch.full((n + 2 * pad,), 777.0, dtype=dtype, device=DEV)
    wbuf = torch.full((wsb + 512,), 0xAB, dtype=torch.uint8, device=DEV)
    out = _hip.gather_grad(Ld, Rd, *args, out=buf[pad:pad + n].view(r0, I, r1), workspace=wbuf[256:256 + wsb])
    assert bool((buf[:pad] == 777.0).all()) and bool((buf[pad + n:] == 777.0).all())  # canaries around dG
    assert bool((wbuf[:256] == 0xAB).all()) and bool((wbuf[256 + wsb:] == 0xAB).all())  # and around the workspace
    again = _hip.gather_grad(Ld, Rd, *args)
    contig = _hip.gather_grad(Ld.contiguous(), Rd.contiguous(), *args)
    assert torch.equal(out, again) and torch.equal(out, contig)  # two calls; row strides ldl > r0, ldr > r1
    got = out.cpu().double()
    ref, mag, count = reference(L, R, perm, tb, te, toff)
    assert count[0] == 0 and count[3] == 0 and not got[:, 0, :].any() and not got[:, 3, :].any()  # exact zeros
    for i in range(I):
        bound = count[i] * EPS[dtype] * mag[:, i, :]
        err = (got[:, i, :] - ref[:, i, :]).abs()
        assert bool((err <= bound).all()), (i, count[i], S, float((err / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_grad_plan_from_an_index_column(dtype):
    """The plan of a random index column with a tiny task size (slices in 1 .. 4 tasks, one slice empty): device kernel against the
    host mirror in fp64."""
    g = torch.Generator().manual_seed(5)
    P, I, r0, r1 = 301, 7, 9, 20
    col = torch.randint(0, I - 1, (P,), generator=g)  # slice I - 1 stays empty
    col[:150] = 2  # one long slice
    v = torch.remainder(col, I)
    perm = torch.sort(v, stable=True).indices
    counts = torch.bincount(v, minlength=I).tolist()
    L = torch.randn(P, r0, generator=g, dtype=F64).to(dtype)
    R = torch.randn(P, r1, generator=g, dtype=F64).to(dtype)
    plan_h = _hostops.GradPlan(counts, "cpu", task_samples=40)
    plan_d = _hipops.GradPlan(counts, DEV, task_samples=40)
    assert plan_d.ntasks == plan_h.ntasks and max(int(x) for x in plan_h.toff[1:] - plan_h.toff[:-1]) >= 3
    got = _hipops.gather_grad(L.to(DEV), R.to(DEV), perm.to(DEV), plan_d).cpu().double()
    ref = _hostops.gather_grad(L.double(), R.double(), perm, plan_h)
    mag = _hostops.gather_grad(L.double().abs(), R.double().abs(), perm, plan_h)
    n = torch.tensor(counts, dtype=F64)[None, :, None]
    assert not got[:, I - 1, :].any()
    assert bool(((got - ref).abs() <= n * EPS[dtype] * mag).all())


def test_gather_grad_refusals_and_empty_input():
    dtype = torch.float32
    one = torch.zeros(1, dtype=torch.int64, device=DEV)
    toff = torch.tensor([0, 1], device=DEV)
    with pytest.raises(NotImplementedError):  # TTR_E_UNSUPPORTED
        _hip.gather_grad(torch.zeros(1, 513, device=DEV), torch.zeros(1, 2, device=DEV), one, one, one + 1, toff)
    with pytest.raises(NotImplementedError):
        _hip.gather_grad(torch.zeros(1, 2, device=DEV), torch.zeros(1, 513, device=DEV), one, one, one + 1, toff)
    out = torch.full((3, 4, 5), float("nan"), dtype=dtype, device=DEV)  # P == 0: zeros
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    _hip.gather_grad(torch.zeros(0, 3, device=DEV), torch.zeros(0, 5, device=DEV), empty, empty, empty,
                     torch.zeros(5, dtype=torch.int64, device=DEV), out=out)
    assert not out.any() and not out.isnan().any()
    out.fill_(float("nan"))  # P == 0 with (empty) tasks
    z4 = torch.zeros(4, dtype=torch.int64, device=DEV)
    _hip.gather_grad(torch.zeros(0, 3, device=DEV), torch.zeros(0, 5, device=DEV), empty, z4, z4,
                     torch.arange(5, device=DEV), out=out)
    assert not out.any() and not out.isnan().any()
