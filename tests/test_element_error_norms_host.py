"""fh_elem_error_norms_host (capi.error_norms_host): the L2 norm and the H1 semi-norm of a discrete function minus a known one, on the host -- the A/B partner of
the device path (tests/test_gpu_element_error_norms.py) -- against the literal restatement of GetErrorNorm_L2_H1_with_analytical_sol and its variants in
tests/error_norm_reference.py, on the meshes of tests/amr_flag_cases.py.  No device."""
import functools

import numpy as np
import pytest

import amr_flag_cases as ac
import error_norm_reference as enr
from femus_amd import capi

# Largest ratios measured over all cases of test 1 on the machine this was written on: |l2_i - reference| / B_i = 3.8e-15 and |h1_i - reference| / B_i =
# 1.8e-15 (B_i: the element's integrand with every product and difference replaced by magnitudes).  They are 0 wherever the library's tables are the oracle's
# to the last bit: the two sides take the same sums in the same order, every product rounded on its own.  TOL = 16 times the larger.
TOL = 16 * 3.8e-15

# a cubic of the coordinates, outside every family's space; the texts are evaluated by the library's evaluator and, through poly(), by Python: the same operations
# in the same order
CUBIC = {2: ("1+x*x*x-2*x*y*y+0.5*x*y+y", ["3*x*x-2*y*y+0.5*y", "0.5*x-4*x*y+1"]),
         3: ("1+x*x*x-2*x*y*y+0.5*x*y+y+z*z*z-x*y*z", ["3*x*x-2*y*y+0.5*y-y*z", "0.5*x-4*x*y+1-x*z", "3*z*z-x*y"])}
# in the family's space on a simplex: linear, and quadratic for the other two
INSIDE = {2: {0: ("1+2*x-y", ["2", "0-1"]), 1: ("1+2*x-y+x*y-3*y*y+0.5*x*x", ["2+y+x", "x-1-6*y"])},
          3: {0: ("1+2*x-y+0.5*z", ["2", "0-1", "0.5"]), 1: ("1+2*x-y+0.5*z+x*y-3*y*y+0.5*x*x+z*x-z*z", ["2+y+x+z", "x-1-6*y", "0.5+x-2*z"])}}
for _d in INSIDE:
    INSIDE[_d][2] = INSIDE[_d][1]
MODES = (enr.QP, enr.DOFS, enr.VECTOR)


def poly(text):
    code = compile(text, "<exact>", "eval")

    def fn(x):
        return eval(code, {"x": x[0], "y": x[1], "z": x[2] if len(x) > 2 else 0.0})
    return fn


def callables(dim, table=None):
    ex, gr = (CUBIC if table is None else table)[dim]
    fns = [poly(t) for t in gr]
    return poly(ex), lambda x: [f(x) for f in fns]


def vectors(m, fe):
    """sol = lcg_fill; the second discrete function: half of it plus the bumped fill of the flag cases (exactly sol/2 far from the corner)"""
    sol, eps = ac.vectors(m, fe)
    return sol, 0.5 * sol + eps


def host(m, fe, mode, sol=None, other=None, table=None):
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    s, o = vectors(m, fe)
    s = s if sol is None else sol
    ex, gr = (CUBIC if table is None else table)[xs.shape[1]]
    if mode == enr.QP:
        return capi.error_norms_host(kind, ed, xs, fe, s, exact=ex, gradient=gr, order=m[3])
    if mode == enr.DOFS:
        return capi.error_norms_host(kind, ed, xs, fe, s, exact=ex, order=m[3])
    return capi.error_norms_host(kind, ed, xs, fe, s, against=o if other is None else other, order=m[3])


@functools.lru_cache(maxsize=None)
def reference(m, fe, mode):
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    s, o = vectors(m, fe)
    ex, gr = callables(xs.shape[1])
    return enr.error_norms(kind, ed, xs, fe, s, mode, ex, gr, o, m[3])


def ratios(got, want, B):
    """|got - want| / B per element; where B_i == 0 both sides must be exactly 0"""
    d = np.abs(got - want)
    assert not got[B == 0].any() and not want[B == 0].any()
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(B == 0, 0.0, d / B)


def check_totals(h, r):
    """all terms are non-negative: any two orders of summation agree within 2 N 2^-53 relative"""
    for key, n in (("l2", r["N_l2"]), ("h1", r["N_h1"])):
        assert abs(h[key] ** 2 - r[key] ** 2) <= 2 * n * 2.0 ** -53 * r[key] ** 2, key


CASES = [(m, fe, mode) for m in ac.MESHES for fe in m[4] for mode in MODES]


def case_id(c):
    return "%s-fe%d-%s" % (ac.mesh_id(c[0]), c[1], c[2])


# ---- 1. the host statement against the literal restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_host_statement_against_the_literal_restatement(case):
    """per element |l2_i - reference| <= TOL B_i and |h1_i - reference| <= TOL B_i (largest ratios measured over all 72 cases: 3.8e-15 and 1.8e-15; TOL = 16 times
    the larger); the squared totals within 2 N 2^-53 relative of the reference's running sums, N the number of (element, point, term) contributions"""
    m, fe, mode = case
    r = reference(m, fe, mode)
    h = host(m, fe, mode)
    r2, r1 = ratios(h["elem_l2"], r["elem_l2"], r["B_l2"]), ratios(h["elem_h1"], r["elem_h1"], r["B_h1"])
    print("largest |l2_i - ref| / B = %.3e, |h1_i - ref| / B = %.3e" % (r2.max(), r1.max()))
    assert TOL <= 1e-10
    assert r2.max() <= TOL and r1.max() <= TOL
    assert r["l2"] > 0 and r["h1"] > 0
    check_totals(h, r)


def poly_arrays(dim, table=None):
    """callables() on arrays of points [..., dim]"""
    ex, gr = (CUBIC if table is None else table)[dim]

    def at(text, x):
        return eval(text, {"x": x[..., 0], "y": x[..., 1], "z": x[..., 2] if dim > 2 else 0.0}) + 0.0 * x[..., 0]
    return lambda x: at(ex, x), lambda x: np.stack([at(t, x) for t in gr], axis=-1)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in (ac.MESHES[1], ac.MESHES[3], ac.MESHES[5], ac.MESHES[-1])], ids=case_id)
def test_the_bounds_in_array_operations_are_the_loops(case):
    """error_norm_reference.magnitude_bounds against the B_i and N of the literal loop: sums of the same non-negative magnitudes in another order, from a
    Jacobian inverted by another routine -- within 1e-12 relative, far above either's rounding and far below what would matter to a bound"""
    m, fe, mode = case
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    s, o = vectors(m, fe)
    r = reference(m, fe, mode)
    ex, gr = poly_arrays(xs.shape[1])
    b = enr.magnitude_bounds(kind, ed, xs, fe, s, mode, ex, gr, o, m[3])
    assert b["N_l2"] == r["N_l2"] and b["N_h1"] == r["N_h1"]
    assert np.allclose(b["B_l2"], r["B_l2"], rtol=1e-12, atol=0) and np.allclose(b["B_h1"], r["B_h1"], rtol=1e-12, atol=0)


# ---- 2. exact zeros --------------------------------------------------------------------------------------------------------------------------------------------------
SMALL = [ac.MESHES[1], ac.MESHES[3], ac.MESHES[6], ac.MESHES[-1]]


def nodal_values(text, xs, n):
    """the expression on the host at the first n nodes, at the point (x, 0 beyond dim, t = 0)"""
    pts = np.zeros((n, 4))
    pts[:, :xs.shape[1]] = xs[:n]
    e = capi.Expr(text, "x,y,z,t")
    try:
        return e(pts)
    finally:
        e.destroy()


@pytest.mark.parametrize("m", SMALL, ids=ac.mesh_id)
def test_exact_zeros(m):
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    for fe in m[4]:
        s, o = vectors(m, fe)
        h = host(m, fe, enr.VECTOR, other=s)
        assert h["l2"] == 0.0 and h["h1"] == 0.0 and not h["elem_l2"].any() and not h["elem_h1"].any()
        h = host(m, fe, enr.DOFS, sol=nodal_values(CUBIC[xs.shape[1]][0], xs, own[fe]))
        assert h["l2"] == 0.0 and h["h1"] == 0.0 and not h["elem_l2"].any() and not h["elem_h1"].any()


# ---- 3. a cross-check that needs no reference -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ac.MESHES, ids=ac.mesh_id)
def test_the_norm_of_one_is_the_volume_of_the_flags(m):
    """sol = 0 against exact = 1 with zero gradients: (0 - 1)(0 - 1) weight is the weight itself, so elem_l2 is bit for bit the vol of error_flag_host on a mesh
    whose elements are all of the mesh's level, and h1 is 0"""
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    dim = xs.shape[1]
    for fe in m[4]:
        h = capi.error_norms_host(kind, ed, xs, fe, np.zeros(own[fe]), exact="1", gradient=["0"] * dim, order=m[3])
        f = capi.error_flag_host(kind, ed, xs, np.zeros(kind.shape[0], dtype=np.int64), 0, fe, np.ones(own[fe]), np.ones(own[fe]), 0.5, "L2", 0.0, m[3])
        assert np.array_equal(h["elem_l2"].view(np.int64), f["vol"].view(np.int64)) and (f["vol"] > 0).all()
        assert h["h1"] == 0.0 and not h["elem_h1"].any()
        assert np.float64(h["l2"]).view(np.int64) == np.sqrt(np.float64(f["sums"][1])).view(np.int64)


# ---- 4. polynomial reproduction ----------------------------------------------------------------------------------------------------------------------------------------
AFFINE = [m for m in ac.MESHES if m[0] in ("tri2.neu", "cube_Tet.neu") and not m[1]]


@pytest.mark.parametrize("m", AFFINE, ids=ac.mesh_id)
def test_a_function_of_the_family_is_reproduced(m):
    """affine elements, exact in the family's space, sol its nodal values: u_h is exact, so l2_i and h1_i are rounding alone, within TOL B_i"""
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    dim = xs.shape[1]
    assert len(AFFINE) == 4
    for fe in m[4]:
        table = {dim: INSIDE[dim][fe]}
        s = nodal_values(table[dim][0], xs, own[fe])
        h = host(m, fe, enr.QP, sol=s, table=table)
        ex, gr = callables(dim, table)
        r = enr.error_norms(kind, ed, xs, fe, s, enr.QP, ex, gr, None, m[3])
        assert (r["B_l2"] > 0).all() and (r["B_h1"] > 0).all()
        print("fe %d: largest l2_i / B = %.3e, h1_i / B = %.3e" % (fe, (h["elem_l2"] / r["B_l2"]).max(), (h["elem_h1"] / r["B_h1"]).max()))
        assert (h["elem_l2"] <= TOL * r["B_l2"]).all() and (h["elem_h1"] <= TOL * r["B_h1"]).all()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
X5 = "x+y+z+t+s"
REFUSALS = [
    (dict(fe=3), "fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not 3"),
    (dict(fe=-1), "fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not -1"),
    (dict(order=7), "unsupported Gauss rule 7"),
    (dict(order="tenth"), "unsupported Gauss rule 'tenth'"),
    (dict(exact=None, gradient=None), "give exact and gradient, exact alone, or against"),
    (dict(exact=None), "mode 0 (qp) needs exact"),
    (dict(gradient=["x", None]), "mode 0 (qp) needs gradient[1]"),
    (dict(gradient=["x"]), "gradient has 1 components, the mesh has dimension 2"),
    (dict(against="sol"), "exact is not allowed in mode 2 (vector)"),
    (dict(exact=None, against="sol"), "gradient is not allowed in mode 2 (vector)"),
    (dict(exact="five"), "exact has 5 variables, at most 4 (x, y, z, t) are served"),
    (dict(gradient=["x", "five"]), "gradient[1] has 5 variables, at most 4 (x, y, z, t) are served"),
    (dict(short="sol"), "sol has 10 entries, the family has 11 dofs on this mesh"),
    (dict(short="against", exact=None, gradient=None, against="short"), "has 10 entries, the family has 11 dofs on this mesh"),
    (dict(sol=None), "sol is null"),
]
REFUSAL_IDS = [",".join("%s=%s" % kv for kv in c.items()) for c, _ in REFUSALS]


def refusal_arguments(change, n, vector):
    """the arguments of error_norms / error_norms_host for one line of REFUSALS; vector(array) makes what the callee takes as a vector"""
    a = dict(fe=2, order="seventh", exact="x*y", gradient=["y", "x"], against=None, sol="sol")
    a.update({k: v for k, v in change.items() if k != "short"})
    made = []

    def expr(t):
        if t == "five":
            made.append(capi.Expr(X5, "x,y,z,t,s"))
            return made[-1]
        return t
    a["exact"] = expr(a["exact"])
    if a["gradient"] is not None:
        a["gradient"] = [expr(t) for t in a["gradient"]]
    short = change.get("short")
    a["sol"] = None if a["sol"] is None else vector(np.ones(n - (1 if short == "sol" else 0)))
    if a["against"] is not None:
        a["against"] = vector(np.ones(n - (1 if short == "against" else 0)))
    return a, made


@pytest.mark.parametrize("change,message", REFUSALS, ids=REFUSAL_IDS)
def test_refusals(change, message):
    kind, ed, xs, own, lev, level = ac.mesh_of("tri2.neu", False, "read")
    assert own[2] == 11
    a, made = refusal_arguments(change, own[2], lambda v: v)
    try:
        with pytest.raises(capi.FemusHipError) as e:
            capi.error_norms_host(kind, ed, xs, a["fe"], a["sol"], a["exact"], a["gradient"], a["against"], a["order"])
        assert message in str(e.value)
    finally:
        for q in made:
            q.destroy()


def test_the_library_refuses_a_mode_out_of_range_and_what_a_mode_must_not_have():
    """what capi never sends: the C entry point alone"""
    import ctypes
    kind, ed, xs, own, lev, level = ac.mesh_of("tri2.neu", False, "read")
    L = capi.load_library()
    code = np.full(kind.shape[0], capi.GEOM["tri"], dtype=np.int32)
    ed32, sol, norms = np.ascontiguousarray(ed, dtype=np.int32), np.ones(own[2]), np.zeros(2)
    ex = capi.Expr("x", "x,y,z,t")
    grad = (ctypes.c_void_p * 2)(ex.h, ex.h)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(mode, exact, gradient, other):
        rc = L.fh_elem_error_norms_host(2, kind.shape[0], p(code), p(ed32), xs.shape[0], p(xs), 2, 4, p(sol), mode, exact, gradient, other, p(norms), None, None)
        return rc, L.fh_last_error().decode()
    try:
        for args, message in (((3, ex.h, grad, None), "mode must be 0 (qp), 1 (dofs) or 2 (vector), not 3"),
                              ((-1, ex.h, grad, None), "mode must be 0 (qp), 1 (dofs) or 2 (vector), not -1"),
                              ((1, ex.h, grad, None), "gradient is not allowed in mode 1 (dofs)"),
                              ((1, None, None, None), "mode 1 (dofs) needs exact"),
                              ((0, ex.h, None, None), "mode 0 (qp) needs gradient"),
                              ((0, ex.h, grad, p(sol)), "other is not allowed in mode 0 (qp)"),
                              ((2, None, None, None), "mode 2 (vector) needs other")):
            rc, text = call(*args)
            assert rc != 0 and message in text, (args[0], text)
        assert call(0, ex.h, grad, None)[0] == 0
    finally:
        ex.destroy()
