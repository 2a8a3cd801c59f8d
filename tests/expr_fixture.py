"""tests/golden/expr_vectors.npz (made by tests/golden/make_expr_vectors.py with mpmath, which no test imports) for the two compilations of the expression
evaluator: the host's (test_expr_host.py) and the device's (test_gpu_expr_device.py)."""
import os

import numpy as np

_G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expr_vectors.npz"))
TEXTS = [str(t) for t in _G["text"]]
SPECIAL_TEXTS = [str(t) for t in _G["special_text"]]
VARIABLES = "x,y,z"

# operations IEEE 754 rounds correctly (+ - * /, sqrt) and operations that are exact: both compilations must give the fixture's bits
EXACT = ["0.0027182818284590452", "x", "-x", "!x", "x+y", "x-y", "x*y", "x/y", "x%y", "x=y", "x!=y", "x<y", "x<=y", "x>y", "x>=y", "x&y", "x|y",
         "abs(x)", "ceil(x)", "floor(x)", "int(x)", "trunc(x)", "sqrt(x)", "max(x,y)", "min(x,y)", "if(x,y,z)"]
INEXACT = [t for t in TEXTS if t not in EXACT]
assert len(TEXTS) == 51 and len(EXACT) == 26 and set(EXACT) <= set(TEXTS)


def vectors(text):
    """(argument tuples padded to the three variables, correctly rounded values)"""
    k = TEXTS.index(text)
    a = _G["args_%02d" % k]
    return np.hstack([a, np.zeros((a.shape[0], 3 - a.shape[1]))]), _G["want_%02d" % k]


def special_vectors(text):
    """(argument tuples padded to the three variables, class per tuple: 0 finite, 1 NaN, 2 +inf, 3 -inf)"""
    k = SPECIAL_TEXTS.index(text)
    a = _G["special_args_%02d" % k]
    return np.hstack([a, np.zeros((a.shape[0], 3 - a.shape[1]))]), _G["special_class_%02d" % k]


def classes(v):
    v = np.asarray(v)
    return np.where(np.isnan(v), 1, np.where(np.isposinf(v), 2, np.where(np.isneginf(v), 3, 0)))


def same_bits(a, b):
    """equal as bit patterns, except that a zero equals a zero of the other sign"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | ((a == 0.0) & (b == 0.0))


def ulps(got, want):
    """|got - want| in units of the spacing of doubles at want (subnormal spacing below the normal range); inf where one side only is not finite"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(got - want) / np.spacing(np.abs(want))
    return np.where(np.isfinite(got) & np.isfinite(want), d, np.where(same_bits(got, want), 0.0, np.inf))
