"""tests/system_reference.py, the yardstick of the system kernel, checked on the host before anything is measured with it:
(a) with one variable it is tests/quasilinear_reference.py, element by element, to 1e-14 of the largest entry;
(b) two different scalar forms side by side: the diagonal blocks are theirs, the off-diagonal blocks exactly 0;
(c) its Jacobian is the derivative of its residual: K delta against the five-point central difference of -RES along delta, in every family;
and the refusals capi.SystemForm makes before anything reaches the device."""
import numpy as np
import pytest

import quasilinear_reference as qr
import system_reference as sr
from test_gpu_generic_assembler import CASES, FES, curved, mesh

_MESH = {}


def setup(case):
    if case not in _MESH:
        kind, ed, xs, own = mesh(case, refinements=0)
        _MESH[case] = (kind, ed, curved(xs), own)
    return _MESH[case]


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("case", CASES)
def test_one_variable_is_the_scalar_restatement(case, name):
    kind, ed, xs, own = setup(case)
    dim = xs.shape[1]
    scalar = qr.with_source({"A": qr.form_a, "B": qr.form_b}[name](dim), dim)[1]
    form = sr.from_scalar([scalar])
    rng = np.random.default_rng(11)
    for fe in FES:
        for e in range(0, ed.shape[0], max(1, ed.shape[0] // 7)):
            s = kind[e]
            nc = sr.mixed_mesh.CLASSES[s][qr.FAM[fe]]
            x, u = xs[ed[e, :nc]], rng.uniform(-1, 1, nc)
            T = qr.tables(s, fe, "seventh")
            Kq, Fq = qr.element(x, u, *T, scalar)
            Ks, Fs = sr.elements(x[None], u[None, None], *T, form)
            assert np.abs(Ks[0, 0, :, 0, :] - Kq).max() <= 1e-14 * np.abs(Kq).max()
            assert np.abs(Fs[0, 0] - Fq).max() <= 1e-14 * max(np.abs(Fq).max(), np.abs(Kq).max())


@pytest.mark.parametrize("case", CASES)
def test_two_scalar_forms_side_by_side(case):
    kind, ed, xs, own = setup(case)
    dim = xs.shape[1]
    fe = "biquadratic"
    ndof = own[2]
    a, b = qr.with_source(qr.form_a(dim), dim)[1], qr.form_b(dim)[1]
    u = np.random.default_rng(11).uniform(-1, 1, (2, ndof))
    K, F = sr.assemble(kind, ed, xs, fe, sr.from_scalar([a, b]), u)
    for k, form in enumerate((a, b)):
        Kk, Fk = qr.assemble(kind, ed, xs, fe, form, u[k])
        blk = K[k * ndof:(k + 1) * ndof, k * ndof:(k + 1) * ndof]
        assert abs(blk - Kk).max() <= 1e-13 * abs(Kk).max()
        assert np.abs(F[k * ndof:(k + 1) * ndof] - Fk).max() <= 1e-13 * np.abs(Fk).max()
        off = K[k * ndof:(k + 1) * ndof, (1 - k) * ndof:(2 - k) * ndof]
        assert off.nnz == 0 or abs(off).max() == 0.0


# the step of the difference per form, as in tests/test_quasilinear_reference_host.py: 2^-3 where RES is a cubic in U (form S), 2^-10 for form R's sqrt
FORMS = {"S": (sr.form_s, 2.0 ** -3), "R": (sr.form_r, 2.0 ** -10)}
JACOBIAN_TOL = 4.4e-12     # the bound of tests/test_quasilinear_reference_host.py (its reasoning holds per variable: the same c and a per species)


@pytest.mark.parametrize("name", list(FORMS))
@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("case", CASES)
def test_the_jacobian_is_the_derivative_of_the_residual(case, fe, name):
    """K(U) delta = d(-RES)(U + t delta)/dt at t = 0 by (R(-2h) - 8 R(-h) + 8 R(h) - R(2h)) / 12h.  Form S makes RES a cubic in U (A_kk grad u_k, u0 u1 grad u0,
    u_d d_d u_k): at h = 2^-3 the formula has no truncation error.  Form R has sqrt(1 + u^2): h = 2^-10, as for the scalar form B."""
    kind, ed, xs, own = setup(case)
    make, h = FORMS[name]
    form = make(xs.shape[1])[1]
    n = form["m"] * own[qr.FAM[fe]]
    rng = np.random.default_rng(11)
    u, delta = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    K, _ = sr.assemble(kind, ed, xs, fe, form, u)
    R = {t: sr.assemble(kind, ed, xs, fe, form, u + t * h * delta)[1] for t in (-2, -1, 1, 2)}
    dR = (R[-2] - 8 * R[-1] + 8 * R[1] - R[2]) / (12 * h)
    Kd = K @ delta
    defect = np.abs(Kd + dR).max() / np.abs(Kd).max()
    print("%s %s form %s: |K delta + dRES| = %.3e of max |K delta|" % (case, fe, name, defect))
    assert defect <= JACOBIAN_TOL
    if name == "S":
        ndof = own[qr.FAM[fe]]
        assert abs(K - K.T).max() > 1e-3 * abs(K).max()
        assert abs(K[:ndof, ndof:2 * ndof] - K[ndof:2 * ndof, :ndof].T).max() > 1e-3 * abs(K).max()          # A_01 != A_10: the blocks are not mirrored


def test_system_form_refusals():
    from femus_amd import capi
    with pytest.raises(ValueError, match="5 variables"):
        capi.SystemForm(5)
    with pytest.raises(ValueError, match="0 variables"):
        capi.SystemForm(0)
    with pytest.raises(ValueError, match=r"f has 3 entries, 2 are expected"):
        capi.SystemForm(2, f=["1", "2", "3"])
    with pytest.raises(ValueError, match=r"A\[1\] has 1 entries, 2 are expected"):
        capi.SystemForm(2, A=[["1", None], ["1"]])
    with pytest.raises(ValueError, match=r"A\[0\] must be a list"):
        capi.SystemForm(2, A=["1", "1"])
    with pytest.raises(ValueError, match=r"c_g\[0\]\[0\] has 4 entries, at most 3"):
        capi.SystemForm(1, c_g=[[["u0"] * 4]])
    with pytest.raises(ValueError, match=r"A_u has 1 entries"):
        capi.SystemForm(2, A_u=[[[None, None], [None, None]]])
    wide = capi.Expr("u0+w", capi.SystemForm.variables(2) + ",w")
    try:
        with pytest.raises(ValueError, match=r"c\[1\] has 12 variables, at most 11"):
            capi.SystemForm(2, c=[None, wide])
        with pytest.raises(capi.FemusHipError):
            capi.SystemForm(2, c=["u2", None])                 # u2 is no variable of a system of two
    finally:
        wide.destroy()
    assert capi.SystemForm.variables(2) == "x,y,z,u0,u1,u0x,u0y,u0z,u1x,u1y,u1z"
    form = capi.SystemForm(**sr.form_s(3)[0])
    assert form.m == 3 and len(form.exprs) == 3 + 5 + 5 + 3 + 9 + 9
    form.destroy()
