"""The cases of tests/golden/sample_f64.npz (tools/gen_sample_golden.py) and the checks the host and the GPU tests of ``tn.sample``
share.  A case is a random fp64 train drawn by the reference after ``torch.manual_seed(11)``; the fixture holds its cores as the
reference drew them (``<case>_core<n>``) and the reference's ``tn.sample(t, P=4096, seed=5)`` as uint8 (``<case>_X``).

``valid`` is the per-decision check that makes a comparison independent of rounding: a computed index is right when the
threshold lies, within the rounding of the computation, between the exact running sums on either side of it (DESIGN section 23
derives the bound)."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_GOLDEN, SEED_GOLDEN, SEED_CORES = 4096, 5, 11
CASES = {
    "pos": ("rand", [8, 7, 6, 5], 4),
    "signed": ("randn", [8, 7, 6, 5], 4),
    "long": ("rand", [3] * 12, 3),
    "wide": ("rand", [64, 33, 17], 6),
}
MAX_UNEXPLAINED_SHARE = 0.01   # rows that may differ from the golden rows (and must then pass ``valid``): a condition, not a tolerance

_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "sample_f64.npz")) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


def build(name, tn):
    """The train of a case as the package ``tn`` draws it (the recording tool calls this with the reference)."""
    kind, shape, r = CASES[name]
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(SEED_CORES)
        return getattr(tn, kind)(shape, ranks_tt=r)
    finally:
        torch.set_default_dtype(old)


def cores(name, dtype=torch.float64, device="cpu"):
    """The cores of a case from the fixture (not redrawn)."""
    z = fixture()
    return [torch.from_numpy(z[f"{name}_core{n}"]).to(dtype).to(device) for n in range(len(CASES[name][1]))]


def golden(name):
    return torch.from_numpy(fixture()[f"{name}_X"].astype(np.int64))


def thresholds(P, N, seed=SEED_GOLDEN):
    """The reference's stream: ``rng.random(P)`` once per mode, in mode order, as an fp64 [P, N] tensor."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([rng.random(P) for _ in range(N)], axis=1))


def valid(cores, X, U, dtype):
    """bool [P]: every decision of every sample is right up to the rounding of a computation in ``dtype``.

    In fp64 on the CPU, from the cores as given and along the prefix X itself holds: q_i = |L . fiber_i|, its running sums c_i and
    T.  A decision x passes when  c_{x-1} - d <= u T < c_x + d  and  q_x > 0,  with
        d = 2 n eps(dtype) sum_i S_i + 2 I 2^-53 T,
        n = (r_0 + .. + r_{mu+1}) + sum_{k > mu} (I_k + r_{k+1}) + N + 2,
    S_i the same quantity as q_i computed from the absolute values of the cores and of the right vector.  (The issue proposed
    n = r_0 + .. + r_{mu+1} + 2 and no factors of 2; the derivation of DESIGN section 23 also counts the terms of the right
    vector, which the sweep computes in the dtype as well, one rounding per mode for the rescalings, and that the comparison
    c_x > u T has a rounded quantity on either side.)"""
    cs = [c.detach().double().cpu() for c in cores]
    X, U = X.detach().cpu(), U.detach().double().cpu()
    N, P = len(cs), X.shape[0]
    eps = torch.finfo(dtype).eps
    right, aright = [None] * (N + 1), [None] * (N + 1)
    right[N] = aright[N] = torch.ones(cs[-1].shape[2], dtype=torch.float64)
    for mu in reversed(range(N)):
        right[mu] = cs[mu].sum(dim=1) @ right[mu + 1]
        aright[mu] = cs[mu].abs().sum(dim=1) @ aright[mu + 1]
    L = torch.ones((P, cs[0].shape[0]), dtype=torch.float64)
    aL = L.clone()
    ok = torch.ones(P, dtype=torch.bool)
    n_left = cs[0].shape[0]
    for mu in range(N):
        G = cs[mu]
        r, I, rn = G.shape
        n_left += rn
        n_right = sum(cs[k].shape[1] + cs[k].shape[2] for k in range(mu + 1, N))
        n = n_left + n_right + N + 2
        q = (L @ torch.einsum("aib,b->ai", G, right[mu + 1])).abs()
        S = aL @ torch.einsum("aib,b->ai", G.abs(), aright[mu + 1])
        c = torch.cumsum(q, dim=1)
        T = c[:, -1]
        d = 2 * n * eps * S.sum(dim=1) + 2 * I * 2.0 ** -53 * T
        x = X[:, mu]
        inside = (x >= 0) & (x < I)
        xc = x.clamp(0, I - 1)
        cx = c.gather(1, xc[:, None])[:, 0]
        cprev = torch.where(xc > 0, c.gather(1, (xc - 1).clamp_min(0)[:, None])[:, 0], torch.zeros_like(cx))
        qx = q.gather(1, xc[:, None])[:, 0]
        uT = U[:, mu] * T
        ok &= inside & (cprev - d <= uT) & (uT < cx + d) & (qx > 0)
        Gx = G[:, xc, :]
        L = torch.einsum("pa,apb->pb", L, Gx)
        aL = torch.einsum("pa,apb->pb", aL, Gx.abs())
    return ok


def explained(X, X_ref, cores, U, dtype):
    """Assert that the rows of X that differ from X_ref pass ``valid`` and number at most 1 % of P; returns their number."""
    X, X_ref = X.detach().cpu(), X_ref.detach().cpu()
    assert X.shape == X_ref.shape and X.dtype == X_ref.dtype == torch.int64
    differ = (X != X_ref).any(dim=1)
    nd = int(differ.sum())
    if nd:
        ok = valid(cores, X, U, dtype)
        assert bool(ok[differ].all()), "{} differing rows are not explained by rounding".format(int((differ & ~ok).sum()))
    assert nd <= MAX_UNEXPLAINED_SHARE * X.shape[0], "{} of {} rows differ".format(nd, X.shape[0])
    return nd
