"""Tensors of shape 2^N read as Boolean formulas of N symbols: 1 where the formula holds, 0 elsewhere.

Mirror of ``tntorch/logic.py`` with the reference's semantics; the connectives are the operators ``~ & | ^`` of ``Tensor``
(``1 - a``, ``a * b``, ``a + b - a * b``, ``a + b - 2 a * b``).

Unlike the reference: the constructors take ``dtype`` and ``device`` (default: fp32 on the CPU, what the reference builds), and
``is_satisfiable`` sums through the chain of right environments (there is no ``tn.sum`` here).
"""

import numpy as np
import torch

from .tensor import Tensor

__all__ = ["true", "false", "all", "none", "any", "one", "symbols", "relevant_symbols", "irrelevant_symbols", "only", "presence",
           "absence", "is_tautology", "is_contradiction", "is_satisfiable", "implies", "equiv"]


def _literals(N, which, value, dtype, device):
    """Rank-1 cores of ones with entry ``value`` of every mode in ``which`` set to zero."""
    cores = [torch.ones([1, 2, 1], dtype=dtype, device=device) for n in range(N)]
    for w in np.atleast_1d(which):
        cores[int(w)][0, value, 0] = 0
    return Tensor(cores)


def true(N, dtype=None, device=None):
    """A formula of N symbols that is always true (logic.py:7-16)."""
    return Tensor([torch.ones([1, 2, 1], dtype=dtype, device=device) for n in range(N)])


def false(N, dtype=None, device=None):
    """A formula of N symbols that is always false (logic.py:19-28)."""
    return Tensor([torch.zeros([1, 2, 1], dtype=dtype, device=device) for n in range(N)])


def all(N, which=None, dtype=None, device=None):
    """Satisfied iff all symbols (or those in ``which``) are true (logic.py:31-50)."""
    return _literals(N, range(N) if which is None else which, 0, dtype, device)


def none(N, which=None, dtype=None, device=None):
    """Satisfied iff all symbols (or those in ``which``) are false (logic.py:53-72)."""
    return _literals(N, range(N) if which is None else which, 1, dtype, device)


def any(N, which=None, dtype=None, device=None):
    """Satisfied iff at least one symbol (of those in ``which``) is true (logic.py:75-85)."""
    return ~none(N, which, dtype=dtype, device=device)


def one(N, which=None, dtype=None, device=None):
    """Satisfied iff one and only one input is true, the n-ary exclusive or (logic.py:88-103; with ``which``: and it is one of
    those)."""
    from .automata import weight_mask

    m = weight_mask(N, 1, dtype=dtype, device=device)
    return m if which is None else m & any(N, which, dtype=dtype, device=device)


def symbols(N, dtype=None, device=None):
    """The N Boolean symbols, each an N-dimensional tensor (logic.py:106-115)."""
    return [presence(N, n, dtype=dtype, device=device) for n in range(N)]


def relevant_symbols(t):
    """The variables whose value affects the formula's output in at least one case (logic.py:118-134): those along which the
    difference of the two slices is not zero."""
    from .metrics import norm

    t2 = Tensor([torch.cat((c[:, 1:2, :] - c[:, 0:1, :], c), dim=1) for c in t.decompress_tucker_factors().cores])
    N = t.dim()
    return [n for n in range(N) if float(norm(t2[[slice(1, 3)] * n + [0] + [slice(1, 3)] * (N - n - 1)])) > 1e-10]


def irrelevant_symbols(t):
    """The variables whose value never affects the formula's output (logic.py:137-147)."""
    rel = relevant_symbols(t)
    return [n for n in range(t.dim()) if n not in rel]


def only(t):
    """Forces all irrelevant symbols to be zero (logic.py:150-165): with ``x, y = tn.symbols(2)``, ``x`` holds in two cases and
    ``tn.only(x)`` in one (x true, y false)."""
    from .tools import mask

    c0 = t.cores[0]
    return mask(t, absence(t.dim(), irrelevant_symbols(t), dtype=c0.dtype, device=c0.device))


def presence(N, which, dtype=None, device=None):
    """True iff all symbols in ``which`` are present (logic.py:168-182)."""
    return _literals(N, which, 0, dtype, device)


def absence(N, which, dtype=None, device=None):
    """True iff all symbols in ``which`` are absent (logic.py:185-199)."""
    return _literals(N, which, 1, dtype, device)


def is_tautology(t):
    """True iff the formula is always satisfied (logic.py:202-211)."""
    from .metrics import norm

    return bool(norm(~t) <= 1e-6)


def is_contradiction(t):
    """True iff the formula is never satisfied (logic.py:214-223)."""
    from .metrics import norm

    return bool(norm(t) <= 1e-6)


def is_satisfiable(t):
    """True iff the formula can be satisfied (logic.py:226-235): its sum is at least 1e-6."""
    from .automata import _total

    return bool(_total(t, "is_satisfiable") >= 1e-6)


def implies(t1, t2):
    """True iff ``t1`` implies ``t2``, i.e. is a sufficient condition (logic.py:238-248)."""
    return bool(is_contradiction(t1 & ~t2))


def equiv(t1, t2):
    """True iff the two formulas are logically equivalent (logic.py:251-261)."""
    return implies(t1, t2) & implies(t2, t1)
