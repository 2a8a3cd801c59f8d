"""tests/system_transient_reference.py, the yardstick of the theta-step of systems, checked on the host before anything is measured with it:
(a) with one variable and M = 1 it is tests/transient_reference.py;
(b) its Jacobian is the derivative of its residual: K delta against the five-point central difference of -RES along delta, for forms S and R, theta = 1 and
    0.5, a full non-symmetric M and an M with a zero row (step and bound of tests/test_system_reference_host.py: the mass term is linear in U and adds no
    truncation error);
(c) with a zero row of M and theta = 0.5, that row's block is the theta = 1 assembly's: the algebraic equation is taken at the new time;
and the refusals capi.TransientSystemForm makes before anything reaches the device."""
import numpy as np
import pytest

import quasilinear_reference as qr
import system_reference as sr
import system_transient_reference as st
import transient_reference as tr
from test_system_reference_host import FORMS as STEPS, JACOBIAN_TOL, setup

TIME, DT = 0.7, 0.05
PAIRS = [("tri", "biquadratic"), ("tet", "serendipity"), ("wedge", "linear"), ("mixed3d", "linear"), ("mixed2d", "biquadratic")]
TIMED = {"S": st.form_s, "R": st.form_r}


def mass_of(kind, m):
    """full: every entry in (0.5, 2), not symmetric; zero_row: the same with the last row 0 (an algebraic last equation)"""
    M = np.random.default_rng(7).uniform(0.5, 2.0, (m, m))
    if kind == "zero_row":
        M[m - 1] = 0.0
    return M


@pytest.mark.parametrize("theta", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("case,fe", [("tri", "biquadratic"), ("mixed3d", "serendipity")])
def test_one_variable_with_unit_mass_is_the_scalar_restatement(case, fe, name, theta):
    kind, ed, xs, own = setup(case)
    dim, ndof = xs.shape[1], own[qr.FAM[fe]]
    scalar = tr.timed({"A": qr.form_a, "B": qr.form_b}[name](dim), dim)[1]
    form = lambda t: sr.from_scalar([scalar(t)])
    u, uo = np.random.default_rng(11).uniform(-1, 1, ndof), np.random.default_rng(12).uniform(-1, 1, ndof)
    Kt, Ft = tr.assemble(kind, ed, xs, fe, scalar, u, uo, TIME, DT, theta)
    for M in (None, [[1.0]]):
        Ks, Fs = st.assemble(kind, ed, xs, fe, form, u, uo, TIME, DT, theta, M=M)
        assert abs(Ks - Kt).max() <= 1e-13 * abs(Kt).max()
        assert np.abs(Fs - Ft).max() <= 1e-13 * np.abs(Ft).max()


@pytest.mark.parametrize("mass", ["full", "zero_row"])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", ["S", "R"])
@pytest.mark.parametrize("case,fe", PAIRS)
def test_the_jacobian_is_the_derivative_of_the_residual(case, fe, name, theta, mass):
    """K_tr(U) delta = d(-RES_tr)(U + t delta)/dt at t = 0 by (R(-2h) - 8 R(-h) + 8 R(h) - R(2h)) / 12h, Uo fixed"""
    kind, ed, xs, own = setup(case)
    h = STEPS[name][1]
    form = TIMED[name](xs.shape[1])[1]
    m = form(TIME)["m"]
    n = m * own[qr.FAM[fe]]
    M = mass_of(mass, m)
    rng = np.random.default_rng(11)
    u, delta = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    uo = np.random.default_rng(12).uniform(-1, 1, n)
    Mass = tr.mass(kind, ed, xs, fe)
    at = lambda v: st.assemble(kind, ed, xs, fe, form, v, uo, TIME, DT, theta, M=M, Mass=Mass)
    K = at(u)[0]
    R = {t: at(u + t * h * delta)[1] for t in (-2, -1, 1, 2)}
    dR = (R[-2] - 8 * R[-1] + 8 * R[1] - R[2]) / (12 * h)
    Kd = K @ delta
    defect = np.abs(Kd + dR).max() / np.abs(Kd).max()
    print("%s %s form %s theta %g mass %s: |K delta + dRES| = %.3e of max |K delta|" % (case, fe, name, theta, mass, defect))
    assert defect <= JACOBIAN_TOL
    assert abs(K - K.T).max() > 1e-3 * abs(K).max()


@pytest.mark.parametrize("name", ["S", "R"])
@pytest.mark.parametrize("case,fe", [("tri", "biquadratic"), ("mixed3d", "linear")])
def test_an_algebraic_row_is_taken_at_the_new_time(case, fe, name):
    """M with a zero last row: at theta = 0.5 that row block of K and RES is bit for bit the one of theta = 1 -- dt (J, S)(U, time), nothing of the old state --
    while the other row blocks differ"""
    kind, ed, xs, own = setup(case)
    form = TIMED[name](xs.shape[1])[1]
    m, ndof = form(TIME)["m"], own[qr.FAM[fe]]
    M = mass_of("zero_row", m)
    assert list(st.thetas(M, 0.5)) == [0.5] * (m - 1) + [1.0] and list(st.thetas(M, 0.0)) == [0.0] * (m - 1) + [1.0]
    u, uo = np.random.default_rng(11).uniform(-1, 1, m * ndof), np.random.default_rng(12).uniform(-1, 1, m * ndof)
    K5, F5 = st.assemble(kind, ed, xs, fe, form, u, uo, TIME, DT, 0.5, M=M)
    K1, F1 = st.assemble(kind, ed, xs, fe, form, u, uo, TIME, DT, 1.0, M=M)
    Ks, Fs = sr.assemble(kind, ed, xs, fe, form(TIME), u)
    last, other = slice((m - 1) * ndof, m * ndof), slice(0, ndof)
    assert abs(K5[last] - K1[last]).max() == 0.0 and np.array_equal(F5[last], F1[last])
    assert abs(K5[last] - DT * Ks[last]).max() <= 1e-15 * abs(Ks).max() and np.abs(F5[last] - DT * Fs[last]).max() <= 1e-15 * np.abs(Fs).max()
    assert abs(K5[other] - K1[other]).max() > 1e-3 * abs(K1).max() and np.abs(F5[other] - F1[other]).max() > 1e-3 * np.abs(F1).max()


def test_transient_system_form_refusals():
    from femus_amd import capi
    assert capi.TransientSystemForm.variables(2) == "x,y,z,u0,u1,u0x,u0y,u0z,u1x,u1y,u1z,t"
    assert capi.SystemForm.variables(2) == "x,y,z,u0,u1,u0x,u0y,u0z,u1x,u1y,u1z"
    with pytest.raises(ValueError, match="TransientSystemForm: 5 variables"):
        capi.TransientSystemForm(5)
    with pytest.raises(ValueError, match="TransientSystemForm: 0 variables"):
        capi.TransientSystemForm(0)
    with pytest.raises(ValueError, match=r"f has 3 entries, 2 are expected"):
        capi.TransientSystemForm(2, f=["1", "2", "3"])
    with pytest.raises(ValueError, match=r"c_g\[0\]\[0\] has 4 entries, at most 3"):
        capi.TransientSystemForm(1, c_g=[[["u0"] * 4]])
    wide = capi.Expr("u0+t+w", capi.TransientSystemForm.variables(2) + ",w")
    timed = capi.Expr("u0*t", capi.TransientSystemForm.variables(2))
    try:
        with pytest.raises(ValueError, match=r"TransientSystemForm: the program c\[1\] has 13 variables, at most 12"):
            capi.TransientSystemForm(2, c=[None, wide])
        with pytest.raises(ValueError, match=r"SystemForm: the program c\[0\] has 12 variables, at most 11"):
            capi.SystemForm(2, c=[timed, None])                # the stationary form keeps its 3 + 4 m
        with pytest.raises(capi.FemusHipError):
            capi.TransientSystemForm(2, c=["u2", None])        # u2 is no variable of a system of two
        with pytest.raises(capi.FemusHipError):
            capi.SystemForm(2, f=["1+t", None])                # t is no variable of the stationary form
        form = capi.TransientSystemForm(2, c=[timed, None], f=["(1+x)*(1+t)", "t"])
        assert form.m == 2 and len(form.exprs) == 3 and isinstance(form, capi.SystemForm)
        form.destroy()
        assert timed.h is not None                             # the caller's Expr is left alone
    finally:
        wide.destroy()
        timed.destroy()
    form = capi.TransientSystemForm(**st.form_s(3)[0])
    assert form.m == 3 and len(form.exprs) == 3 + 5 + 5 + 3 + 9 + 9
    form.destroy()
    form = capi.TransientSystemForm(**st.form_r()[0])
    assert form.m == 4
    form.destroy()
