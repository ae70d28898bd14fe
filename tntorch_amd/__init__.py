"""tntorch_amd -- MI355X-native TT orthogonalisation / rounding behind tntorch's API.

``import tntorch_amd as tn`` exposes the names of the reference (``tntorch/__init__.py:1-14``)
that sit on the TT decomposition / rounding hot path: ``tn.Tensor``, ``tn.round_tt``,
``tn.round``, ``tn.truncated_svd``, the unfoldings, plus the small helpers the reference's
tests use around them (``rand``/``randn``, ``dot``/``norm``/``relative_error``), and TT-cross (``tn.cross``, ``tn.maxvol``,
``tn.meshgrid`` and the element-wise functions of ``ops``: ``tn.exp``, ``tn.cos``, ...), and TT completion from samples
(``tn.als_completion``), sparse TT-SVD (``tn.sparse_tt_svd``), sparse polynomial-chaos regression of scattered float samples
(``tn.PCEInterpolator``, ``tn.gram_schmidt``, ``tn.features2indices``, ...), the moment family (``tn.hadamard_sum``, ``tn.raw_moment``,
``tn.normalized_moment``, ``tn.var``, ``tn.std``) and the differential operators of ``derivatives.py`` (``tn.partial``,
``tn.gradient``, ``tn.divergence``, ``tn.curl``, ``tn.laplacian``, ``tn.dgsm``, ``tn.active_subspace``) and the exact
convolution of two trains (``tn.convolve``), and the Boolean layer: ``tn.automata`` (``tn.weight_mask``, ``tn.accepted_inputs``,
...), ``tn.logic`` (``tn.symbols``, ``tn.only``, ``tn.implies``, ...), ``tn.mask`` and ``tn.partialset``, and the array tools of
``tools.py`` and ``ops.py``: ``tn.squeeze``, ``tn.unsqueeze``, ``tn.unbind``, ``tn.cat``, ``tn.transpose``, ``tn.flip``, ``tn.pad``,
``tn.ttm``, ``tn.generate_basis`` and ``tn.cumsum`` (marginalising a mode is ``tn.squeeze(tn.ttm(t, weights, dim))``; there is no
``tn.sum`` / ``tn.mean``), and the variance-based sensitivity analysis of ``anova.py``: ``tn.anova_decomposition``,
``tn.undo_anova_decomposition``, ``tn.truncate_anova``, ``tn.sobol``, ``tn.mean_dimension`` and ``tn.dimension_distribution``,
and drawing index vectors from a train read as an unnormalised mass function: ``tn.sample``, and the matrix formats of
``matrix.py`` with their products with a batch of vectors: ``tn.TTMatrix``, ``tn.CPMatrix``, ``tn.tt_multiply``, ``tn.cp_multiply``, and a batch of rows of a TT-matrix
(``tn.tt_lookup``: the embedding table; ``tn.tt_embedding`` / ``tn.tt_embedding_bag``: the same table, trainable on the device), and the products that stay in TT format (``tn.tt_apply``: a TT-matrix applied to a
train, ``tn.tt_matmul``, ``tn.tt_transpose``), and the solver that inverts them: ``tn.tt_solve``, fixed-rank ALS for ``A x = b``
with a symmetric positive definite ``TTMatrix`` and a train ``b`` (the three-layer environment fused into one kernel), and
``tn.tt_amen_solve``, the same system at ranks that adapt while the sweeps run (AMEn; the local CG steps are three fused kernels), and the extreme
eigenpair of a symmetric ``TTMatrix``: ``tn.tt_eigsh``, fixed-rank ALS whose local LOBPCG steps are two fused kernels, and gradient-based fitting (``autodiff.py``):
``tn.optimize`` and ``tn.dof``, with ``t[X]`` at index arrays, ``Tensor.torch()``, ``tn.dist`` / ``tn.relative_error`` against a
dense tensor and ``tn.tt_multiply`` (in the cores and the tensor) differentiable on the device (hand-written backward passes; every other operation refuses device cores that require
grad).
"""

from .tools import *  # noqa: F401,F403
from .round import *  # noqa: F401,F403
from .tensor import *  # noqa: F401,F403
from .create import *  # noqa: F401,F403
from .metrics import *  # noqa: F401,F403
from .matrix import *  # noqa: F401,F403
from .lookup import *  # noqa: F401,F403
from .embedding import *  # noqa: F401,F403
from .ttalgebra import *  # noqa: F401,F403
from .ttsolve import *  # noqa: F401,F403
from .tteigs import *  # noqa: F401,F403
from .ttamen import *  # noqa: F401,F403
from .maxvol import *  # noqa: F401,F403
from .cross import *  # noqa: F401,F403
from .ops import *  # noqa: F401,F403
from .interpolation import *  # noqa: F401,F403
from .derivatives import *  # noqa: F401,F403
from .automata import *  # noqa: F401,F403
from .logic import *  # noqa: F401,F403
from .anova import *  # noqa: F401,F403
from .autodiff import *  # noqa: F401,F403
from . import autodiff, automata, embedding, logic, lookup, ttamen, tteigs, ttsolve  # noqa: F401
from . import dist_batch  # noqa: F401
from ._patch import patch  # noqa: F401

__version__ = "0.1.0"


def hip_available() -> bool:
    """True when the HIP kernel library has been built in-tree."""
    from . import _hip

    return _hip.available()
