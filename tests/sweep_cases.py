"""What the tests of the sweep kernels (ttr_sweep.hip: ttr_rowgram, ttr_rotgram, ttr_project / ttr_project_flat, ttr_colgram,
ttr_colproject) share: graded and random operands, the fp64 truths of every result, and ENTRY-WISE error bounds that are derived
here, not measured.  Importable without a GPU.

Operands.  graded(R, n, decay) = Q diag(2^(-decay j)) P^T rounded to the working precision; V1 = the eigenvectors of the Gram
matrix FORMED IN THE WORKING PRECISION (solved in fp64, descending, rounded): what pass 1 of the two-pass truncation hands to
pass 2.  V2 and sigma come from the rotated Gram matrix in the same way.  The decays keep sigma_min^2 above 2^-100, and with the
item scales 2^+-20 every product stays a normal fp32 number.

Truths are fp64 products of the ROUNDED operands:  W = V1^T M,  G = W W^T,  U = V1 V2[:, :ro] (a pass-through item: V1[:, :ro];
without V1: V2[:, :ro]),  right = U^T M [/ sigma],  left = U [sigma].  A `rows32` item counts rows 32.. of M as zero.  The tall
("col") kernels compute the transposes: ttr_colgram(M) is the row Gram matrix of M^T, ttr_colproject's left is right^T and its
right is left^T.

Bounds.  u = 2^-24 / 2^-53, gamma_k = k u / (1 - k u): a sum of k products in the working precision, in ANY order, is within
gamma_k sum |a||b| of the exact one (Higham, Accuracy and Stability, section 3.1).
  rotation      What = fl(V1^T M) = W + dW, |dW| <= E = gamma_R |V1|^T |M|                    (R products per entry)
  rotgram       Ghat = fl(What What^T): |What What^T - W W^T| <= A E^T + E A^T + E E^T with A = |W|, and the Gram sum itself
                (n products, the 4-wave reduction, the sum of the nparts partials) adds gamma_(n+4+nparts) (A+E)(A+E)^T
  rowgram       gamma_(n+4+nparts) |M||M|^T
  U             E_U = gamma_R |V1||V2| + u |U|   (R products, one rounding on the way to memory); 0 where U is a copy
  right         Uhat^T M computed with R products: E_U^T |M| + gamma_R (|U| + E_U)^T |M|, divided by |sigma|, + 2 u |right| for
                the reciprocal and the product with it.  Where the kernels' rule makes 1 / sigma = 0 (|sigma| below the smallest
                normal) the entries must be exact zeros: truth 0, bound 0.
  left          E_U |sigma| + u |left|
Every bound is taken with the project's usual factor 2 to spare (higher-order terms, the error of the fp64 truth) and gets
R n tiny(dtype) on top, so that a flushed subnormal is not a failure.  The point of the entry-wise form: an entry of G that
belongs to two small rotated rows gets a bound of its own size.  V1^T (M M^T) V1 -- one pass instead of two -- errs there by
gamma sigma_1^2 and is refused by two orders of magnitude (test_sweep_cases_host.py), while `max |err| / max |G|` passes it.
"""
import functools

import torch

DTYPES = [torch.float32, torch.float64]
SPARE = 2.0

# (R, n, decay): sigma_j = 2^(-decay j)
GRADED = [(64, 100, 0.5), (64, 1000, 0.5), (37, 65, 1.0)]
ITEM_SCALES = (1.0, 2.0 ** 20, 2.0 ** -20)   # one item each: B = 3

GRAM_R = (1, 15, 16, 17, 32, 33, 48, 63, 64)
GRAM_N = (1, 15, 16, 17, 48, 49, 65)
PROJECT_RO_64 = (1, 15, 16, 17, 31, 32, 33, 63, 64)
PROJECT_SMALL_R = (1, 17, 32, 33)
PROJECT_N = (1, 2, 31, 32, 33, 65)
PROJECT_SPLIT_N = ((543, 2), (1000, 4))      # (n, parts at B = 2)
COL_N = (1, 15, 16, 17, 33, 63, 64)
COL_ROWS = (1, 15, 17, 65, 257)
COL_SPLIT_ROWS = ((1000, 3), (1030, 4))      # (rows, parts at B = 2)
NPARTS_N, NPARTS = 100, (1, 3, 7, 9)         # 7 chunks of 16 columns


def unit(dt):
    return 2.0 ** -24 if dt == torch.float32 else 2.0 ** -53


def tiny(dt):
    return torch.finfo(dt).tiny


def dt_name(dt):
    return "f32" if dt == torch.float32 else "f64"


def gamma(k, dt):
    ku = k * unit(dt)
    assert ku < 0.01
    return ku / (1.0 - ku)


# ------------------------------------------------------------------ the kernels' host arithmetic, mirrored
def split_range(chunks, nparts, part):
    per = (chunks + nparts - 1) // nparts
    c0 = part * per
    return c0, min(c0 + per, chunks)


def pick_split(n, batch):
    """Parts of ttr_project (and of ttr_sweep_gram_parts): 32-column chunks, >= 8 per part, aiming at 2048 workgroups, <= 64."""
    chunks = (n + 31) // 32
    want = (2048 + batch - 1) // batch
    return max(1, min(want, max(chunks // 8, 1), 64))


def col_split(rows, batch):
    """Parts of ttr_colgram / ttr_colproject: 16-row chunks, >= 16 per part, aiming at 4096 workgroups."""
    chunks = (rows + 15) // 16
    want = (4096 + batch - 1) // batch
    return max(1, min(want, max(chunks // 16, 1), 4096))


# ------------------------------------------------------------------ operands
def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * p for k, p in zip(key, (7919, 104729, 1299709, 15485863))) % (2 ** 31))


def graded(R, n, decay, dt, seed=0):
    """M [R, n] = Q diag(2^(-decay j)) P^T rounded to dt."""
    assert 2.0 * decay * (R - 1) < 100, "sigma_min^2 below 2^-100"
    g = _gen(R, n, seed, 1)
    Q = torch.linalg.qr(torch.randn(R, R, generator=g, dtype=torch.float64))[0]
    P = torch.linalg.qr(torch.randn(max(n, R), R, generator=g, dtype=torch.float64))[0][:n]
    s = 2.0 ** (-decay * torch.arange(R, dtype=torch.float64))
    return ((Q * s) @ P.T).to(dt)


def randn(shape, dt, seed=0):
    return torch.randn(shape, generator=_gen(*shape[-2:], seed, 2), dtype=torch.float64).to(dt)


def orthogonal(B, R, dt, seed=0):
    """[B, R, R] random orthogonal matrices rounded to dt."""
    return torch.linalg.qr(torch.randn(B, R, R, generator=_gen(B, R, seed, 3), dtype=torch.float64))[0].to(dt)


def eig_desc(G):
    """(eigenvalues, eigenvectors) of the symmetric G (any dtype), solved in fp64, in descending order."""
    w, V = torch.linalg.eigh(G.double())
    return w.flip(-1), V.flip(-1)


def pass1_vectors(M):
    """V1 (and sigma1) of M [..., R, n]: from the Gram matrix formed in M's dtype -- what pass 1 hands over."""
    w, V = eig_desc(M @ M.transpose(-1, -2))
    return V.to(M.dtype), w.clamp_min(0).sqrt().to(M.dtype)


def pass2_vectors(M, V1):
    """V2 and sigma: from the Gram matrix of the rows rotated in M's dtype."""
    W = V1.transpose(-1, -2) @ M
    w, V = eig_desc(W @ W.transpose(-1, -2))
    return V.to(M.dtype), w.clamp_min(0).sqrt().to(M.dtype)


@functools.lru_cache(maxsize=None)
def graded_batch(R, n, decay, dt):
    """(M [3, R, n], V1, V2 [3, R, R], sigma, sigma1 [3, R]): three different graded matrices scaled by 1, 2^20 and 2^-20.
    Read-only: shared by the tests."""
    M = torch.stack([graded(R, n, decay, dt, seed=b) * s for b, s in enumerate(ITEM_SCALES)])
    V1, sigma1 = pass1_vectors(M)
    V2, sigma = pass2_vectors(M, V1)
    return M, V1, V2, sigma, sigma1


@functools.lru_cache(maxsize=None)
def random_batch(B, R, n, dt, seed=0):
    """(M [B, R, n] randn, V1, V2 random orthogonal, sigma, sigma1 in [0.5, 1.5)) -- read-only."""
    g = _gen(B, R, n, seed)
    M = randn((B, R, n), dt, seed)
    V1, V2 = orthogonal(B, R, dt, seed + 1), orthogonal(B, R, dt, seed + 2)
    sigma = (torch.rand(B, R, generator=g, dtype=torch.float64) + 0.5).to(dt)
    sigma1 = (torch.rand(B, R, generator=g, dtype=torch.float64) + 0.5).to(dt)
    return M, V1, V2, sigma, sigma1


# ------------------------------------------------------------------ truths and bounds (batched: leading dimension B)
def _flags(f, B):
    if f is None:
        return torch.zeros(B, dtype=torch.bool)
    return torch.as_tensor(f).cpu().bool().reshape(B)


def effective(M, rows32=None):
    """M in fp64 with rows 32.. of the flagged items as the zeros they stand for (whatever memory holds there)."""
    Md = M.detach().cpu().double().clone()
    f = _flags(rows32, Md.shape[0])
    if Md.shape[1] > 32 and bool(f.any()):
        Md[f, 32:] = 0.0
    return Md


def gram_truth_and_bound(M, V1, dt, nparts=1, rows32=None):
    """(G, bound) [B, R, R] of ttr_rowgram (V1 None) / ttr_rotgram, summed over the parts."""
    Md = effective(M, rows32)
    B, R, n = Md.shape
    gs = gamma(n + 4 + nparts, dt)
    floor = R * n * tiny(dt)
    if V1 is None:
        A = Md.abs()
        return Md @ Md.transpose(1, 2), SPARE * gs * (A @ A.transpose(1, 2)) + floor
    Vd = V1.detach().cpu().double()
    W = Vd.transpose(1, 2) @ Md
    E = gamma(R, dt) * (Vd.abs().transpose(1, 2) @ Md.abs())
    A = W.abs()
    AE = A + E
    bound = A @ E.transpose(1, 2) + E @ A.transpose(1, 2) + E @ E.transpose(1, 2) + gs * (AE @ AE.transpose(1, 2))
    return W @ W.transpose(1, 2), SPARE * bound + floor


def part_columns(n, nparts, part, chunk=16):
    """Columns [c0, c1) of `part`: the kernels split the ceil(n / chunk) chunks by split_range."""
    c0, c1 = split_range((n + chunk - 1) // chunk, nparts, part)
    return min(c0 * chunk, n), min(c1 * chunk, n)


def part_truths_and_bounds(M, V1, dt, nparts, rows32=None):
    """(G, bound) [B, nparts, R, R]: every part is the Gram matrix of its own column range; a part without a chunk is exactly
    zero (bound 0)."""
    B, R, n = M.shape
    G = torch.zeros(B, nparts, R, R, dtype=torch.float64)
    bound = torch.zeros_like(G)
    for q in range(nparts):
        c0, c1 = part_columns(n, nparts, q)
        if c1 > c0:
            G[:, q], bound[:, q] = gram_truth_and_bound(M[:, :, c0:c1], V1, dt, 1, rows32)
    return G, bound


def u_truth(V1, V2, ro, dt, flat=None):
    """(U, E_U) [B, R, ro] in fp64: U = V1 V2[:, :ro]; V1[:, :ro] for a pass-through item; V2[:, :ro] without V1 (E_U = 0 for both)."""
    V2d = V2.detach().cpu().double()
    B = V2d.shape[0]
    if V1 is None:
        U = V2d[:, :, :ro].clone()
        return U, torch.zeros_like(U)
    V1d = V1.detach().cpu().double()
    V2c = torch.nan_to_num(V2d[:, :, :ro], nan=0.0)
    U = V1d @ V2c
    EU = gamma(V1d.shape[1], dt) * (V1d.abs() @ V2c.abs()) + unit(dt) * U.abs()
    f = _flags(flat, B)
    U[f] = V1d[f][:, :, :ro]
    EU[f] = 0.0
    return U, EU


def project_truth_and_bounds(M, V1, V2, sigma, ro, scale_right, dt, rows32=None, flat=None, sigma1=None):
    """(right [B, ro, n], right bound, left [B, R, ro], left bound) of ttr_project / ttr_project_flat.  `sigma` None: no
    scaling.  Pass-through items (flat, only with V1) take their scales from sigma1."""
    Md = effective(M, rows32)
    B, R, n = Md.shape
    u = unit(dt)
    if V1 is None:
        flat = None
    U, EU = u_truth(V1, V2, ro, dt, flat)
    aM = Md.abs()
    right = U.transpose(1, 2) @ Md
    rb = EU.transpose(1, 2) @ aM + gamma(R, dt) * ((U.abs() + EU).transpose(1, 2) @ aM)
    left = U.clone()
    lb = EU.clone()
    floor = R * n * tiny(dt)
    if scale_right and sigma is not None:
        sg = sigma.detach().cpu().double()[:, :ro].clone()
        f = _flags(flat, B)
        if bool(f.any()):
            sg[f] = sigma1.detach().cpu().double()[f][:, :ro]
        dead = sg.abs() < tiny(dt)                       # the kernels' rule: 1 / sigma counts as 0
        inv = torch.where(dead, torch.zeros_like(sg), 1.0 / torch.where(dead, torch.ones_like(sg), sg))
        right = right * inv[:, :, None]
        rb = rb * inv.abs()[:, :, None] + 2 * u * right.abs()
        rb = SPARE * rb + ((~dead).double() * floor)[:, :, None]
        left = U * sg[:, None, :]
        lb = SPARE * (EU * sg.abs()[:, None, :] + u * left.abs()) + floor
    else:
        rb = SPARE * rb + floor
        lb = SPARE * lb + floor
    return right, rb, left, lb


def colgram_truth_and_bound(M, V1, dt, nparts=1):
    """ttr_colgram of the tall M [B, rows, n]: the row formulas on M^T."""
    return gram_truth_and_bound(M.transpose(1, 2), V1, dt, nparts)


def colproject_truth_and_bounds(M, V1, V2, sigma, ro, left_ortho, dt):
    """(left [B, rows, ro], left bound, right [B, ro, n], right bound) of ttr_colproject: the transposes of the row results."""
    r, rb, l, lb = project_truth_and_bounds(M.transpose(1, 2), V1, V2, sigma, ro, left_ortho, dt)
    return r.transpose(1, 2), rb.transpose(1, 2), l.transpose(1, 2), lb.transpose(1, 2)


def ratio(got, truth, bound):
    """max |got - truth| / bound (inf for a NaN or an error at a zero bound)."""
    err = (got.detach().cpu().double() - truth).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.nan_to_num(r, nan=float("inf"))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------ emulations in the working precision (torch, any device)
def emulate_gram(M, V1=None):
    """The faithful algorithm: rotate, then Gram, every product in M's dtype."""
    W = M if V1 is None else V1.transpose(1, 2) @ M
    return W @ W.transpose(1, 2)


def emulate_shortcut(M, V1):
    """One pass: V1^T (M M^T) V1 in M's dtype -- what ttr_rotgram exists to avoid."""
    return V1.transpose(1, 2) @ (M @ M.transpose(1, 2)) @ V1


def emulate_project(M, V1, V2, sigma, ro, scale_right, swap=None, sigma_roll=0):
    """right, left as the kernels form them, in M's dtype.  swap = (i, j): U with columns i and j exchanged; sigma_roll: sigma
    taken from the item that many places on (both: deliberate damage for the host tests)."""
    U = V2[:, :, :ro] if V1 is None else V1 @ V2[:, :, :ro]
    if swap is not None:
        U = U.clone()
        U[:, :, list(swap)] = U[:, :, list(swap[::-1])]
    right = U.transpose(1, 2) @ M
    left = U
    if scale_right:
        sg = torch.roll(sigma, sigma_roll, 0)[:, :ro]
        right = right * (1.0 / sg)[:, :, None]
        left = U * sg[:, None, :]
    return right, left


# ------------------------------------------------------------------ ttr_spectrum_flat, ttr_carry_rows32: the header's rules
def spectrum_flat_rule(sigma, keep, thr):
    """flat[b] = sigma[b][keep - 1] >= thr sigma[b][0] > 0, in fp64 (batch mode: no tolerance)."""
    s = sigma.detach().cpu().double()
    return ((s[:, 0] > 0) & (s[:, keep - 1] >= thr * s[:, 0])).to(torch.int32)


def carry_rows32_rule(Rm, c, dt):
    """flag[b] = rows 32.. of the 64-row Rm[b] hold at most (c eps)^2 of its squared Frobenius norm, in fp64."""
    x = Rm.detach().cpu().double()
    low = (x[:, 32:] ** 2).sum(dim=(1, 2))
    ce = c * torch.finfo(dt).eps
    return (low <= ce * ce * (x ** 2).sum(dim=(1, 2))).to(torch.int32)
