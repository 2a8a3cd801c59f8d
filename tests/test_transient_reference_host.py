"""tests/transient_reference.py, the yardstick of the transient kernel and driver, checked on the host before anything is measured with it:
(a) its Jacobian is the derivative of its residual in u: K_tr delta against the five-point central difference of -RES_tr along delta;
(b) on the linear heat equation its stepper is the matrix recursion (M + theta dt K)^-1 (M - (1 - theta) dt K);
(c) that stepping has the temporal orders of the theta-method against the semi-discrete exact solution."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import quasilinear_reference as qr
import transient_reference as tr
from test_gpu_generic_assembler import curved, mesh

TIME, DT = 0.7, 0.05
# the step of the difference: 2^-3 where RES is a cubic in u (form A), 2^-10 for the sqrt of form B, as tests/test_quasilinear_reference_host.py argues; the
# mass term is linear in u and adds no truncation error.  The bound is the one that file is asked: 1e-9 of max |K delta|
FORMS = {"A": (qr.form_a, 2.0 ** -3), "B": (qr.form_b, 2.0 ** -10)}


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", list(FORMS))
@pytest.mark.parametrize("case,fe", [("tri", "biquadratic"), ("mixed3d", "linear"), ("mixed2d", "serendipity")])
def test_the_jacobian_is_the_derivative_of_the_residual(case, fe, name, theta):
    kind, ed, xs, own = mesh(case, refinements=0)
    xs = curved(xs)
    dim, ndof = xs.shape[1], own[qr.FAM[fe]]
    make, h = FORMS[name]
    _, form = tr.timed(make(dim), dim)
    rng = np.random.default_rng(11)
    u, uo, delta = rng.uniform(-1, 1, ndof), rng.uniform(-1, 1, ndof), rng.uniform(-1, 1, ndof)
    M = tr.mass(kind, ed, xs, fe)
    K, _ = tr.assemble(kind, ed, xs, fe, form, u, uo, TIME, DT, theta, M=M)
    R = {t: tr.assemble(kind, ed, xs, fe, form, u + t * h * delta, uo, TIME, DT, theta, M=M)[1] for t in (-2, -1, 1, 2)}
    dR = (R[-2] - 8 * R[-1] + 8 * R[1] - R[2]) / (12 * h)
    Kd = K @ delta
    defect = np.abs(Kd + dR).max() / np.abs(Kd).max()
    print("%s %s form %s theta %g: |K delta + dRES| = %.3e of max |K delta|" % (case, fe, name, theta, defect))
    assert defect <= 1e-9
    if name == "A":
        assert abs(K - K.T).max() > 1e-3 * abs(K - M).max()


def host_heat(theta, nsteps):
    lv, free, M, K, u0 = tr.heat_system()
    s = tr.HostStepper(lv, "linear", lambda t: {}, dirichlet={f: None for f in (-2, -3, -4, -5)}, theta=theta)
    s.set_initial(u0)
    for _ in range(nsteps):
        s.step(tr.HEAT_T / nsteps, tol=1e-6)
        s.copy_solution_to_old()
    return s.u


@pytest.mark.parametrize("theta", [1.0, 0.5, 0.0])
def test_heat_steps_are_the_matrix_recursion(theta):
    lv, free, M, K, u0 = tr.heat_system()
    n, dt = 8, tr.HEAT_T / 8 * (0.1 if theta == 0.0 else 1.0)        # the explicit method inside its stability limit
    s = tr.HostStepper(lv, "linear", lambda t: {}, dirichlet={f: None for f in (-2, -3, -4, -5)}, theta=theta)
    s.set_initial(u0)
    Mf, Kf = M[free][:, free], K[free][:, free]
    lu = spla.splu(sp.csc_matrix(Mf + theta * dt * Kf))
    w = u0[free].copy()
    for _ in range(n):
        assert s.step(dt) <= 2                                         # a linear problem: the second iteration only sees ||EPS|| < 1e-12
        s.copy_solution_to_old()
        w = lu.solve((Mf - (1 - theta) * dt * Kf) @ w)
    d = np.abs(s.u[free] - w).max()
    print("theta %g: |stepper - recursion| = %.3e of %.3e" % (theta, d, np.abs(w).max()))
    assert d <= 1e-12 * np.abs(w).max()
    assert np.all(s.u[~free] == 0.0) and abs(s.time - n * dt) < 1e-15


@pytest.mark.parametrize("theta,p", [(1.0, 1), (0.5, 2)])
def test_temporal_orders_of_the_stepper(theta, p):
    """u_t = lap u on tri_box(4, 4), linear family, T = 0.1, against exp(-T M^-1 K) u0: steps 8, 16, 32, the last observed order within 0.15 of p"""
    lv, free, M, K, u0 = tr.heat_system()
    exact = tr.heat_exact(free, M, K, u0)
    err = [np.abs(host_heat(theta, n) - exact).max() for n in (8, 16, 32)]
    orders = tr.observed_orders(err)
    print("theta %g: errors %s, orders %s" % (theta, err, orders))
    assert err[0] > err[1] > err[2]
    assert abs(orders[-1] - p) <= 0.15
