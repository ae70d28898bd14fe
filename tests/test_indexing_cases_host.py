"""The references of tests/indexing_cases.py against brute-force loops, on the CPU: chain_reference against a loop over points
and k and against the host mirror, the magnitude bound of the integer cores for every case family of the GPU file, the
counts of counts_column, and the derived error bound on a host fp32 chain."""
import pytest
import torch

import indexing_cases as ic
from tntorch_amd import _hostops

SMALL = [  # ranks, sizes, B, P: batch > 1, r_a and r_b > 1, one mode, a mode of size 1
    ([2, 3, 4, 3], [4, 5, 3], 3, 11),
    ([1, 2, 1], [3, 2], 2, 7),
    ([3, 2], [6], 2, 9),
    ([2, 2, 3, 2, 2], [2, 1, 4, 3], 1, 5),
]


@pytest.mark.parametrize("ranks,sizes,B,P", SMALL)
def test_chain_reference_against_loops(ranks, sizes, B, P):
    cores = ic.gauss_cores(ranks, sizes, B, 7, torch.float64)
    cols = ic.random_cols(sizes, P, 8)
    assert any(bool((c < 0).any()) for c in cols)
    ref, scale = ic.chain_reference(cores, cols)
    assert ref.shape == scale.shape == (B, ranks[0], P, ranks[-1]) and ref.dtype == torch.float64
    brute = ic.brute_chain(cores, cols)
    assert float((ref - brute).abs().max()) <= 1e-13 * float(scale.max())
    host = _hostops.gather_chain(cores, cols)
    assert float((ref - host).abs().max()) <= 1e-13 * float(scale.max())
    assert torch.equal(scale, ic.chain_reference([c.abs() for c in cores], cols)[0])
    assert bool((ref.abs() <= scale * (1 + 1e-12)).all())
    # int32 columns and the wrapped columns give the same reference
    assert torch.equal(ref, ic.chain_reference(cores, [c.to(torch.int32) for c in cols])[0])
    assert torch.equal(ref, ic.chain_reference(cores, [ic.wrapped(c, I) for c, I in zip(cols, sizes)])[0])


def test_chain_reference_on_integer_cores_is_exact():
    cores = ic.int_cores([2, 3, 4, 3], [4, 5, 3], 3, 5)
    cols = ic.random_cols([4, 5, 3], 11, 6)
    ref, _ = ic.chain_reference(cores, cols)
    assert torch.equal(ref, ic.brute_chain(cores, cols)) and torch.equal(ref, ref.round())


def test_reference_refuses_out_of_range():
    cores = ic.int_cores([1, 2, 1], [3, 4], 1, 1)
    for bad in (4, -5):
        with pytest.raises(IndexError):
            ic.chain_reference(cores, [torch.tensor([0, 1]), torch.tensor([0, bad])])


@pytest.mark.parametrize("name", list(ic.INT_CASES))
def test_int_cores_stay_below_the_bound(name):
    ranks, sizes, B = ic.INT_CASES[name]
    bound = ic.int_bound(ranks)
    assert bound <= 2 ** 20 < ic.INT_LIMIT
    cores = ic.case_cores(name)
    assert [tuple(c.shape) for c in cores] == [(B, ranks[n], sizes[n], ranks[n + 1]) for n in range(len(sizes))]
    for c in cores:
        assert torch.equal(c, c.round()) and float(c.abs().max()) <= 2
    P = 3 if B > 1000 else 200
    ref, scale = ic.chain_reference(cores, ic.random_cols(sizes, P, 9))
    # the chain over |G| bounds every partial sum of every output
    assert float(scale.max()) <= bound and float(ref.abs().max()) <= bound
    assert torch.equal(ref, ref.round()) and torch.equal(ref.float().double(), ref)


def test_int_bound_is_the_stated_product():
    assert ic.int_bound([2, 3, 3, 2]) == 2 ** 3 * 9
    assert ic.int_bound([512, 33, 3, 2]) == 2 ** 3 * 99  # the leading rank does not enter
    assert ic.int_bound([4, 64]) == 2
    with pytest.raises(AssertionError):
        ic.int_cores([1, 512, 512, 1], [2, 2, 2], 1, 0)  # 2^3 * 2^18 = 2^21


@pytest.mark.parametrize("counts", list(ic.TILE_EDGE_COUNTS.values()) + [(0, 0, 3), (5,)])
def test_counts_column(counts):
    a, b = ic.counts_column(counts, 1), ic.counts_column(counts, 2)
    assert a.dtype == torch.int64 and a.shape == (sum(counts),)
    assert torch.bincount(a, minlength=len(counts)).tolist() == list(counts)
    assert torch.bincount(b, minlength=len(counts)).tolist() == list(counts)
    assert sum(counts) < 20 or not torch.equal(a, b)  # shuffled by the seed
    assert sum(counts) < 20 or not torch.equal(a, a.sort().values)


def test_tile_edge_counts_fall_on_the_edges():
    """Every family holds an empty group, a group that fills its tiles exactly, and one that is a row over or under."""
    for ra, counts in ic.TILE_EDGE_COUNTS.items():
        rows = [c * ra for c in counts]
        assert 0 in rows
        assert any(r and r % ic.TILE_ROWS == 0 for r in rows)
        assert any(r % ic.TILE_ROWS in (1, 2, 3) for r in rows) and any(r % ic.TILE_ROWS in (61, 62, 63) for r in rows), ra


def test_one_mode_big_passes_the_grid():
    P, ra, rn, _, _ = ic.ONE_MODE_BIG
    assert P * ra * rn > ic.GATHER_GRID * ic.THREADS


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_error_bound_holds_for_a_host_chain(dtype):
    """The derived bound on a chain evaluated in ``dtype`` on the CPU (any summation order): a sanity check of the bound's form."""
    ranks, sizes = ic.lead_ranks(3, gauss=True), [3, 3, 3]
    cores = ic.gauss_cores(ranks, sizes, 2, 11, dtype)
    cols = ic.random_cols(sizes, 37, 12)
    ref, scale = ic.chain_reference(cores, cols)
    got = _hostops.gather_chain(cores, [ic.wrapped(c, 3) for c in cols])
    assert got.dtype == dtype
    assert bool(((got.double() - ref).abs() <= ic.error_bound(ranks, dtype, scale)).all())
    assert float(ic.error_bound([4, 9], dtype, scale).abs().max()) == 0.0
