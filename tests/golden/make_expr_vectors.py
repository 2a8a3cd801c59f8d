"""Generates tests/golden/expr_vectors.npz: for every operator and function of the run-time expression grammar (femus_amd/csrc/fh_expr.cpp) argument
tuples over its domain, edges included, and the value of the operation computed with mpmath at 60 digits and rounded once to double.  Both compilations
of the evaluator -- the host's against libm (tests/test_expr_host.py) and the device's against the device math library (tests/test_gpu_expr_device.py)
-- are pinned to this one table instead of to each other.  A second table holds special arguments (zeros, infinities, NaN, the largest and the smallest
magnitudes) with the CLASS numpy gives on the CPU (finite / NaN / +inf / -inf).

    python tests/golden/make_expr_vectors.py        (needs mpmath; the tests read the .npz only)

The semantics restated here are the parser library's (fparser): truth is |v| >= 0.5, = and != use the epsilon 1e-12, % is the truncated remainder (sign
of the dividend), int() rounds to the nearest integer with halves away from zero, a negative base takes integer exponents only.  No tuple lies within
1e-9 of a jump of a discontinuous operation unless it sits exactly ON the jump with exactly representable arguments (asserted below; the prescribed
= / != cases either side of the epsilon are the one exception, their differences are exact in double arithmetic).  Trigonometric arguments keep 1e-3 from
every pole.  The file is written with fixed zip timestamps: running this script again reproduces it byte for byte.  Numbers and expression strings only."""
import io
import os
import zipfile
from fractions import Fraction

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 60
N_RANDOM = 48
EPS = mp.mpf(1e-12)                         # FHX_EPS as the double the evaluator holds
TINY, HUGE = 5e-324, 1e308
rng = np.random.default_rng(20261017)


def to_double(v):
    """an mpf rounded ONCE to the nearest double (subnormals included; float(mpf) would round twice there)"""
    v = mp.mpf(v)
    if mp.isinf(v) or mp.isnan(v):
        return float(v)
    sign, man, exp, _ = v._mpf_
    q = Fraction(int(man)) * Fraction(2) ** int(exp)
    try:
        r = float(q)
    except OverflowError:
        r = float("inf")
    return -r if sign else r


def truth(v):
    return abs(v) >= mp.mpf(0.5)


def b2f(b):
    return mp.mpf(1 if b else 0)


def fmod(a, b):
    q = mp.floor(abs(a / b)) * mp.sign(a) * mp.sign(b)
    return a - q * b


def power(a, b):
    if a < 0:
        assert b == mp.floor(b)
        return (-1 if int(b) % 2 else 1) * mp.power(-a, b)
    return mp.power(a, b)


def fp_int(a):
    return mp.ceil(a - mp.mpf(0.5)) if a < 0 else mp.floor(a + mp.mpf(0.5))


def trunc(a):
    return mp.ceil(a) if a < 0 else mp.floor(a)


# ---- distance of a tuple to the nearest jump of its operation (None: the operation is continuous there) ----

def d_int(v):
    return abs(v - mp.nint(v))


JUMP = {
    "floor(x)": lambda x: d_int(x), "ceil(x)": lambda x: d_int(x), "trunc(x)": lambda x: d_int(x), "int(x)": lambda x: d_int(x + mp.mpf(0.5)),
    "x<y": lambda x, y: abs(x - y), "x<=y": lambda x, y: abs(x - y), "x>y": lambda x, y: abs(x - y), "x>=y": lambda x, y: abs(x - y),
    "x&y": lambda x, y: min(abs(abs(x) - 0.5), abs(abs(y) - 0.5)), "x|y": lambda x, y: min(abs(abs(x) - 0.5), abs(abs(y) - 0.5)),
    "!x": lambda x: abs(abs(x) - 0.5), "if(x,y,z)": lambda x, y, z: abs(abs(x) - 0.5), "x%y": lambda x, y: d_int(x / y) * abs(y),
}
POLE = {"tan(x)": mp.pi / 2, "sec(x)": mp.pi / 2, "cot(x)": 0, "csc(x)": 0}      # poles at shift + k pi


def pole_distance(text, x):
    return abs((x - POLE[text]) - mp.nint((x - POLE[text]) / mp.pi) * mp.pi)


def acceptable(text, args):
    a = [mp.mpf(float(v)) for v in args]
    if text in JUMP:
        d = JUMP[text](*a)
        if 0 < d < mp.mpf(1e-9):
            return False
    if text in POLE and pole_distance(text, a[0]) < mp.mpf(1e-3):
        return False
    return True


# ---- draws ----

def U(lo, hi, n=N_RANDOM, k=1):
    return rng.uniform(lo, hi, (n, k))


def LU(lo, hi, n=N_RANDOM, k=1, signed=False):
    v = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), (n, k))
    return v * rng.choice([-1.0, 1.0], (n, k)) if signed else v


def col(*vals):
    return np.array(vals, dtype=float).reshape(-1, 1)


def rows(*tuples):
    return np.array(tuples, dtype=float)


TRUTHS = [0.0, 0.49, 0.51, -0.49, -0.51, 0.5, -0.5, 1.0, -1.0, 3.7, 0.2]
TRIG_BIG = [1e5, 1e10, 1e15, -1e5, -1e10, -1e15]
ROUND_EDGES = col(-3, 0, 2, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, -7.5, 6.5, -0.25, -0.75, -41.3, 2.0 ** 53, -2.0 ** 53, 1e15, -1e15)
EQ_CASES = rows(*[(b, b + s * d) for b in (0.0, 1.0, 0.3, -2.5, 100.0) for d in (0.5e-12, 2e-12) for s in (1, -1)],
                *[(b, b) for b in (0.0, 1.0, 0.3, -2.5, 1e300)])
CMP_EQUAL = rows((0.3, 0.3), (1, 1), (-2.5, -2.5), (0, 0), (1e300, 1e300), (-1e-300, -1e-300))
ARITH_WIDE = np.hstack([LU(1e-150, 1e150, 16, 1, True), LU(1e-150, 1e150, 16, 1, True)])

# text -> (mpmath function of the arguments, argument tuples)
OPS = {
    # the 18 program words that are not function calls
    "0.0027182818284590452": (lambda x: mp.mpf("0.0027182818284590452"), U(-1, 1)),
    "x": (lambda x: x, np.vstack([U(-10, 10), col(0, TINY, -HUGE)])),
    "-x": (lambda x: -x, np.vstack([U(-10, 10), col(0, 1e300, -1e300, TINY)])),
    "!x": (lambda x: 1 - b2f(truth(x)), np.vstack([U(-2, 2), col(*TRUTHS)])),
    "x+y": (lambda x, y: x + y, np.vstack([U(-1e3, 1e3, k=2), ARITH_WIDE, rows((0.1, 0.2), (1, -1), (1e16, 1), (1e-310, 1e-310), (2.0 ** -1074, -2.0 ** -1073))])),
    "x-y": (lambda x, y: x - y, np.vstack([U(-1e3, 1e3, k=2), ARITH_WIDE, rows((0.3, 0.1), (1, 1), (1e16, 1), (1, 1 - 2.0 ** -53), (1e-310, 3e-310))])),
    "x*y": (lambda x, y: x * y, np.vstack([U(-1e3, 1e3, k=2), ARITH_WIDE, rows((0.1, 3), (1e-200, 1e-120), (-1e-200, 1.5e-123), (1e154, 1e154), (0, -5))])),
    "x/y": (lambda x, y: x / y, np.vstack([U(-1e3, 1e3, k=2), ARITH_WIDE, rows((1, 3), (2, 3), (1e-300, 1e10), (-1e-300, 3e22), (1e300, 1e-8), (0, 7), (1, 10))])),
    "x%y": (fmod, np.vstack([np.hstack([U(-20, 20, 64), U(0.1, 5, 64) * rng.choice([-1.0, 1.0], (64, 1))]),
                             rows((6, 2), (-7, 2), (7, -2), (-7, -2), (7, 2), (5.5, 0.5), (0.3, 0.7), (-0.3, 0.7), (0, 3), (1e6 + 0.25, 0.5), (-12.75, -0.25))])),
    "x^y": (power, np.vstack([np.hstack([LU(1e-3, 1e3), U(-5, 5)]), np.hstack([U(-10, -0.1), rng.integers(-5, 6, (N_RANDOM, 1)).astype(float)]),
                              rows((2, 10), (2, -1), (0, 2), (0, 0), (-8, 3), (-2, -2), (10, 300), (1.0000001, 1e8), (7, 0.5), (0.5, 1000))])),
    "x=y": (lambda x, y: b2f(abs(x - y) <= EPS), np.vstack([U(-5, 5, k=2), EQ_CASES])),
    "x!=y": (lambda x, y: b2f(abs(x - y) > EPS), np.vstack([U(-5, 5, k=2), EQ_CASES])),
    "x<y": (lambda x, y: b2f(x < y), np.vstack([U(-5, 5, k=2), CMP_EQUAL])),
    "x<=y": (lambda x, y: b2f(x <= y), np.vstack([U(-5, 5, k=2), CMP_EQUAL])),
    "x>y": (lambda x, y: b2f(x > y), np.vstack([U(-5, 5, k=2), CMP_EQUAL])),
    "x>=y": (lambda x, y: b2f(x >= y), np.vstack([U(-5, 5, k=2), CMP_EQUAL])),
    "x&y": (lambda x, y: b2f(truth(x) and truth(y)), rows(*[(a, b) for a in TRUTHS for b in TRUTHS])),
    "x|y": (lambda x, y: b2f(truth(x) or truth(y)), rows(*[(a, b) for a in TRUTHS for b in TRUTHS])),
    # the 33 functions
    "abs(x)": (abs, np.vstack([U(-10, 10), col(0, 1e300, -1e300, TINY, -TINY)])),
    "acos(x)": (mp.acos, np.vstack([U(-1, 1), col(-1, 1, 0, 1 - 1e-12, -1 + 1e-12, 0.5, 1e-10)])),
    "acosh(x)": (mp.acosh, np.vstack([1 + LU(1e-12, 1e6), col(1, 1 + 2.0 ** -52, 1e300, 2, 1 + 1e-8)])),
    "asin(x)": (mp.asin, np.vstack([U(-1, 1), col(-1, 1, 0, 1 - 1e-12, -1 + 1e-12, 0.5, 1e-10)])),
    "asinh(x)": (mp.asinh, np.vstack([LU(1e-10, 1e6, signed=True), col(0, 1e300, -1e300, 1, TINY)])),
    "atan(x)": (mp.atan, np.vstack([U(-10, 10, 24), LU(1e-8, 1e10, 24, signed=True), col(0, 1e300, -1e300, 1, -1, 200.0, -800.0, TINY)])),
    "atanh(x)": (mp.atanh, np.vstack([U(-1, 1), col(1 - 1e-12, -1 + 1e-12, 0, 1e-10, -1e-10, 0.5, 0.999)])),
    "cbrt(x)": (lambda x: mp.sign(x) * mp.cbrt(abs(x)), np.vstack([U(-100, 100, 24), LU(1e-300, 1e300, 24, signed=True), col(0, 8, -27, TINY, 1e300, 1e-300)])),
    "ceil(x)": (mp.ceil, np.vstack([U(-50, 50), ROUND_EDGES])),
    "cos(x)": (mp.cos, np.vstack([U(-10, 10), col(*TRIG_BIG), col(0, 1e-8, 1.5707963267948966, 3.141592653589793, 100.0)])),
    "cosh(x)": (mp.cosh, np.vstack([U(-20, 20), col(0, 700, -700, 1e-10, 710.0, 1)])),
    "cot(x)": (mp.cot, np.vstack([U(-10, 10), col(*TRIG_BIG), col(1.5707963267948966, 0.002, -0.002, 100.0)])),
    "csc(x)": (mp.csc, np.vstack([U(-10, 10), col(*TRIG_BIG), col(1.5707963267948966, 0.002, -0.002, 100.0)])),
    "exp(x)": (mp.exp, np.vstack([U(-20, 20, 40), U(-745, -709, 12), col(709.7, 700, 0, 1, -1, 1e-10, -708.4, -744.9, -745.1, -745.3, -746, -800, -1e4)])),
    "exp2(x)": (lambda x: mp.power(2, x), np.vstack([U(-30, 30, 40), U(-1074, -1022, 8), col(10, -10, 0, 0.5, 1023.5, -1060, -1074, -1074.9, -1075.5, -1080, -5000)])),
    "floor(x)": (mp.floor, np.vstack([U(-50, 50), ROUND_EDGES])),
    "int(x)": (fp_int, np.vstack([U(-50, 50), ROUND_EDGES])),
    "log(x)": (mp.log, np.vstack([LU(1e-300, 1e300), col(1e-300, 1, 1 + 2.0 ** -52, 1 - 2.0 ** -53, 0.999999, 1.000001, 2.718281828459045, TINY, 1e308)])),
    "log10(x)": (mp.log10, np.vstack([LU(1e-300, 1e300), col(1e-300, 1, 10, 1000, 1e-5, 1 + 2.0 ** -52, 0.999999, TINY, 1e308)])),
    "log2(x)": (lambda x: mp.log(x, 2), np.vstack([LU(1e-300, 1e300), col(1e-300, 1, 8, 0.25, 1 + 2.0 ** -52, 0.999999, 3, TINY, 1e308)])),
    "sec(x)": (mp.sec, np.vstack([U(-10, 10), col(*TRIG_BIG), col(0, 1e-8, 3.141592653589793, 1.5687963267948966, 100.0)])),
    "sin(x)": (mp.sin, np.vstack([U(-10, 10), col(*TRIG_BIG), col(0, 1e-8, 1.5707963267948966, 3.141592653589793, 100.0, TINY)])),
    "sinh(x)": (mp.sinh, np.vstack([U(-20, 20), col(0, 700, -700, 1e-10, -1e-10, 710.0, 1)])),
    "sqrt(x)": (mp.sqrt, np.vstack([LU(1e-300, 1e300), col(0, 4, 2, TINY, 1e308, 0.25, 1e-320)])),
    "tan(x)": (mp.tan, np.vstack([U(-10, 10), col(*TRIG_BIG), col(0, 1e-8, 0.7853981633974483, 1.5687963267948966, 100.0)])),
    "tanh(x)": (mp.tanh, np.vstack([U(-5, 5), col(0, 20, -20, 1e-10, -1e-10, 0.5, 400.0)])),
    "trunc(x)": (trunc, np.vstack([U(-50, 50), ROUND_EDGES])),
    "atan2(x,y)": (mp.atan2, np.vstack([U(-10, 10, k=2), rows((0, 1), (1, 0), (0, -1), (-1, 0), (1e-300, 1e300), (1, -1), (-1, -1), (1e300, 1e-300), (3, 1e-9))])),
    "hypot(x,y)": (mp.hypot, np.vstack([U(-10, 10, 32, 2), LU(1e-200, 1e200, 16, 2, True), rows((3, 4), (1e300, 1e300), (1e-300, 1e-300), (0, 0), (0, 5), (1, 1e-20), (TINY, TINY))])),
    "max(x,y)": (max, np.vstack([U(-10, 10, k=2), rows((0.3, 0.3), (0, -1), (-1e300, 1e300), (2, 2), (-TINY, TINY))])),
    "min(x,y)": (min, np.vstack([U(-10, 10, k=2), rows((0.3, 0.3), (0, -1), (-1e300, 1e300), (2, 2), (-TINY, TINY))])),
    "pow(x,y)": (power, np.vstack([np.hstack([LU(1e-3, 1e3), U(-5, 5)]), np.hstack([U(-10, -0.1), rng.integers(-5, 6, (N_RANDOM, 1)).astype(float)]),
                                   rows((2, 10), (2, -1), (0, 2), (0, 0), (-8, 3), (-2, -2), (10, 300), (1.0000001, 1e8), (1.5, 0.3), (0.5, 1000))])),
    "if(x,y,z)": (lambda x, y, z: y if truth(x) else z, np.vstack([U(-2, 2, k=3), np.hstack([col(*TRUTHS), U(-9, 9, len(TRUTHS), 2)])])),
}
assert len(OPS) == 18 + 33


def filtered(text, args):
    """tuples that keep their distance from jumps and poles; the random part must keep N_RANDOM of them"""
    keep = np.array([acceptable(text, a) for a in args])
    return args[keep]


# ---- special arguments: the class only, from numpy on the CPU ----

SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, HUGE, -HUGE, TINY, -TINY])
NP_UNARY = {
    "abs(x)": np.abs, "acos(x)": np.arccos, "acosh(x)": np.arccosh, "asin(x)": np.arcsin, "asinh(x)": np.arcsinh, "atan(x)": np.arctan, "atanh(x)": np.arctanh,
    "cbrt(x)": np.cbrt, "ceil(x)": np.ceil, "cos(x)": np.cos, "cosh(x)": np.cosh, "cot(x)": lambda x: 1.0 / np.tan(x), "csc(x)": lambda x: 1.0 / np.sin(x),
    "exp(x)": np.exp, "exp2(x)": np.exp2, "floor(x)": np.floor, "int(x)": lambda x: np.where(x < 0, np.ceil(x - 0.5), np.floor(x + 0.5)), "log(x)": np.log,
    "log10(x)": np.log10, "log2(x)": np.log2, "sec(x)": lambda x: 1.0 / np.cos(x), "sin(x)": np.sin, "sinh(x)": np.sinh, "sqrt(x)": np.sqrt, "tan(x)": np.tan,
    "tanh(x)": np.tanh, "trunc(x)": np.trunc,
}
NP_BINARY = {"x+y": np.add, "x-y": np.subtract, "x*y": np.multiply, "x/y": np.divide}
CLASS_FINITE, CLASS_NAN, CLASS_PINF, CLASS_NINF = 0, 1, 2, 3


def classes(v):
    return np.where(np.isnan(v), CLASS_NAN, np.where(np.isposinf(v), CLASS_PINF, np.where(np.isneginf(v), CLASS_NINF, CLASS_FINITE))).astype(np.int8)


def write_npz(path, arrays):
    """np.savez_compressed with the zip members' timestamps fixed, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    out = {"text": np.array(list(OPS))}
    for k, (text, (fn, args)) in enumerate(OPS.items()):
        a = filtered(text, np.asarray(args, dtype=float))
        assert a.shape[0] >= 48, (text, a.shape)
        want = np.array([to_double(fn(*[mp.mpf(float(v)) for v in t])) for t in a])
        assert not np.isnan(want).any(), text
        out["args_%02d" % k], out["want_%02d" % k] = a, want
    with np.errstate(all="ignore"):
        sp_text = list(NP_UNARY) + list(NP_BINARY)
        out["special_text"] = np.array(sp_text)
        pairs = np.array([(a, b) for a in SPECIAL for b in SPECIAL])
        for k, text in enumerate(sp_text):
            if text in NP_UNARY:
                a = SPECIAL.reshape(-1, 1)
                c = classes(NP_UNARY[text](SPECIAL))
            else:
                a = pairs
                c = classes(NP_BINARY[text](pairs[:, 0], pairs[:, 1]))
            out["special_args_%02d" % k], out["special_class_%02d" % k] = a, c
    path = os.path.join(HERE, "expr_vectors.npz")
    write_npz(path, out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
