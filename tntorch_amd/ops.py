"""``cumsum`` (ops.py:6-30) and the element-wise functions of tensor trains by cross-approximation (ops.py:53-348).

``cumsum`` is exact: the running sum of a mode is the running sum of its core (or Tucker factor) along the mode axis, one
``ttr_mode_scan`` launch per mode on device tensors.  ``cumprod`` (ops.py:33-45: ``exp(cumsum(log(t)))``, two cross-approximations)
stays out of scope.

Each element-wise function is one call to :func:`cross` with ``verbose=False``.  ``div`` and ``pow`` call cross with ``x / y`` and
``x ** y`` directly (the reference goes through ``t1 / t2`` and ``t1 ** t2``, tensor.py:775-795); the ``Tensor`` operators keep
their own behaviour.
"""

import torch

from .cross import cross

__all__ = ["cumsum", "abs", "acos", "asin", "cos", "cosh", "erf", "erfinv", "exp", "log", "log10", "log2", "reciprocal", "rsqrt", "sigmoid", "sin", "sinh", "sqrt", "tan", "tanh", "add", "atan2", "mul", "div", "pow"]


def cumsum(t, dim=None):
    """Computes the cumulative sum of a tensor along one or several dims, similarly to PyTorch's ``cumsum()`` (ops.py:6-30).  The
    Tucker factor is scanned where the mode has one, else the core.

    :param t: input :class:`Tensor`
    :param dim: an int or list of ints (default: all)

    :return: a :class:`Tensor` of the same shape, on ``t``'s device in its dtype

    Unlike the reference: the running sums are accumulated in fp64 and rounded once (for fp32 cores too); a ``dim`` out of range
    or repeated raises ValueError, batched tensors ValueError, CP cores NotImplementedError.  ``t`` is not modified.
    """
    from ._dispatch import ops_for
    from .tensor import Tensor
    from .tools import _array_dims, _check_array_tensor

    _check_array_tensor(t, "cumsum")
    dims = _array_dims(range(t.dim()) if dim is None else dim, t.dim(), "cumsum")
    cores, Us = [], []
    for n in range(t.dim()):
        core, U = t.cores[n], t.Us[n]
        if n not in dims:
            cores.append(core.clone())
            Us.append(None if U is None else U.clone())
        elif U is None:
            cores.append(ops_for(core).mode_scan(core.contiguous()))
            Us.append(None)
        else:
            cores.append(core.clone())
            Us.append(ops_for(U).mode_scan(U[None].contiguous())[0])
    return Tensor(cores, Us=Us, idxs=t._idxs)


def abs(t):
    """Element-wise ``torch.abs`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.abs(x), tensors=t, verbose=False)


def acos(t):
    """Element-wise ``torch.acos`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.acos(x), tensors=t, verbose=False)


def asin(t):
    """Element-wise ``torch.asin`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.asin(x), tensors=t, verbose=False)


def cos(t):
    """Element-wise ``torch.cos`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.cos(x), tensors=t, verbose=False)


def cosh(t):
    """Element-wise ``torch.cosh`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.cosh(x), tensors=t, verbose=False)


def erf(t):
    """Element-wise ``torch.erf`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.erf(x), tensors=t, verbose=False)


def erfinv(t):
    """Element-wise ``torch.erfinv`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.erfinv(x), tensors=t, verbose=False)


def exp(t):
    """Element-wise ``torch.exp`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.exp(x), tensors=t, verbose=False)


def log(t):
    """Element-wise ``torch.log`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.log(x), tensors=t, verbose=False)


def log10(t):
    """Element-wise ``torch.log10`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.log10(x), tensors=t, verbose=False)


def log2(t):
    """Element-wise ``torch.log2`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.log2(x), tensors=t, verbose=False)


def reciprocal(t):
    """Element-wise ``torch.reciprocal`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.reciprocal(x), tensors=t, verbose=False)


def rsqrt(t):
    """Element-wise ``torch.rsqrt`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.rsqrt(x), tensors=t, verbose=False)


def sigmoid(t):
    """Element-wise ``torch.sigmoid`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.sigmoid(x), tensors=t, verbose=False)


def sin(t):
    """Element-wise ``torch.sin`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.sin(x), tensors=t, verbose=False)


def sinh(t):
    """Element-wise ``torch.sinh`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.sinh(x), tensors=t, verbose=False)


def sqrt(t):
    """Element-wise ``torch.sqrt`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.sqrt(x), tensors=t, verbose=False)


def tan(t):
    """Element-wise ``torch.tan`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.tan(x), tensors=t, verbose=False)


def tanh(t):
    """Element-wise ``torch.tanh`` of a :class:`Tensor`, by cross-approximation."""
    return cross(lambda x: torch.tanh(x), tensors=t, verbose=False)


def add(t1, t2):
    """Element-wise ``x + y`` of two :class:`Tensor` of the same shape, by cross-approximation."""
    return cross(lambda x, y: x + y, tensors=[t1, t2], verbose=False)


def atan2(t1, t2):
    """Element-wise ``torch.atan2(x, y)`` of two :class:`Tensor` of the same shape, by cross-approximation."""
    return cross(lambda x, y: torch.atan2(x, y), tensors=[t1, t2], verbose=False)


def mul(t1, t2):
    """Element-wise ``x * y`` of two :class:`Tensor` of the same shape, by cross-approximation."""
    return cross(lambda x, y: x * y, tensors=[t1, t2], verbose=False)


def div(t1, t2):
    """Element-wise ``x / y`` of two :class:`Tensor` of the same shape, by cross-approximation."""
    return cross(lambda x, y: x / y, tensors=[t1, t2], verbose=False)


def pow(t1, t2):
    """Element-wise ``x ** y`` of two :class:`Tensor` of the same shape, by cross-approximation."""
    return cross(lambda x, y: x ** y, tensors=[t1, t2], verbose=False)
