"""Element-wise functions of tensor trains by cross-approximation (ops.py:53-348): each is one call to :func:`cross` with
``verbose=False``.  ``div`` and ``pow`` call cross with ``x / y`` and ``x ** y`` directly (the reference goes through
``t1 / t2`` and ``t1 ** t2``, tensor.py:775-795); the ``Tensor`` operators keep their own behaviour.  ``cumsum`` and ``cumprod``
are out of scope.
"""

import torch

from .cross import cross

__all__ = ["abs", "acos", "asin", "cos", "cosh", "erf", "erfinv", "exp", "log", "log10", "log2", "reciprocal", "rsqrt", "sigmoid", "sin", "sinh", "sqrt", "tan", "tanh", "add", "atan2", "mul", "div", "pow"]


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
