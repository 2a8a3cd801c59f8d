"""femus_amd.transient.TransientQuasilinearElements: theta-steps on resident element meshes against the host stepper of tests/transient_reference.py (Newton on
the restatement's system with scipy's sparse LU), the temporal orders against the semi-discrete exact solution, a stationary solution as a fixed point, a flagged
top level, run() against its steps, and a second driver after destroy().  Everything on tri_box meshes of at most three levels from 2 x 2 (the heat problem: 4 x 4).

The stepping problem: form B, u_t - div((1 + u^2) grad u) + sqrt(1 + u^2) = exp(x) (1 + y) (1 + t) on (-1, 1)^2; on the left side (flag -5) u = 0.3 (1 - y^2) t,
which moves in time and vanishes at the corners it shares with the bottom and top sides (-2, -4: u = 0); on the right side (-3) the flux 0.5 (1 + y);
u(0) = 0.2 (1 - x^2) (1 - y^2)."""
import functools

import numpy as np
import pytest

import quasilinear_reference as qr
import transient_reference as tr
from femus_amd import mixed_mesh

pytestmark = pytest.mark.gpu
G_LEFT, FLUX_RIGHT, U0 = "0.3*(1-y*y)*t", "0.5*(1+y)", "0.2*(1-x*x)*(1-y*y)"
U0_HOT = "0.2*(1-x*x)+0.1"          # not zero on the sides whose Dirichlet value is 0 (flags given as None), nor on the left side at t = 0
DT, NSTEPS, TOL = 0.05, 4, 1e-9
FE = "biquadratic"


def level0():
    return mixed_mesh.tri_box(2, 2, (-1., -1.), (1., 1.))


@functools.lru_cache(maxsize=None)
def host_steps(theta, nlevels, start=U0):
    """(solution after NSTEPS steps, Newton iterations of every step) of the host stepper"""
    from femus_amd import capi
    lv = level0()
    for _ in range(1, nlevels):
        lv = mixed_mesh.refine(*lv[:4])
    g, q, u0 = capi.Expr(G_LEFT, "x,y,z,t"), capi.Expr(FLUX_RIGHT, "x,y,z,t"), capi.Expr(start, "x,y,z,t")
    s = tr.HostStepper(lv, FE, tr.timed(qr.form_b(2), 2)[1], dirichlet={-5: g, -2: None, -4: None}, flux={-3: q}, theta=theta)
    x4 = np.zeros((s.ndof, 4))
    x4[:, :2] = lv[2][:s.ndof]
    s.set_initial(u0(x4))
    counts = []
    for _ in range(NSTEPS):
        counts.append(s.step(DT, tol=TOL, max_newton=15))
        s.copy_solution_to_old()
    for e in (g, q, u0):
        e.destroy()
    s.u.setflags(write=False)
    return s.u, tuple(counts)


def stepping_driver(ctx, theta, nlevels, form, **kw):
    from femus_amd.transient import TransientQuasilinearElements
    return TransientQuasilinearElements(ctx, level0(), FE, nlevels, form, dirichlet={-5: G_LEFT, -2: None, -4: None}, flux={-3: FLUX_RIGHT}, theta=theta, **kw)


def timed_form():
    from femus_amd import capi
    return capi.TransientForm(**tr.timed(qr.form_b(2), 2)[0])


@pytest.mark.parametrize("nlevels", [2, 1])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_steps_against_the_host_stepper(ctx, theta, nlevels):
    """four steps: the solution within 1e-10 of the host stepper's largest entry (the project's bound for a driver against a host Newton with a direct solve),
    and the same number of Newton iterations in every step"""
    want, counts = host_steps(theta, nlevels)
    form = timed_form()
    d = stepping_driver(ctx, theta, nlevels, form)
    try:
        d.set_initial(U0)
        out = d.run(DT, NSTEPS, tol=TOL, max_newton=15, lin_maxit=30)
        u = d.solution()
        err = np.abs(u - want).max()
        print("theta %g, %d levels: |u - host stepper| = %.3e of %.3e, Newton iterations %s (host %s)"
              % (theta, nlevels, err, np.abs(want).max(), [len(o["newton_history"]) for o in out], list(counts)))
        assert all(o["converged"] for o in out)
        assert abs(d.time - NSTEPS * DT) < 1e-14 and abs(out[-1]["time"] - d.time) == 0.0
        assert err <= 1e-10 * np.abs(want).max()
        assert tuple(len(o["newton_history"]) for o in out) == counts
        if nlevels == 1:
            assert all(h[0] <= 1 for o in out for h in o["newton_history"])
    finally:
        d.destroy()
        form.destroy()


@pytest.mark.parametrize("as_array", [False, True])
def test_an_initial_state_that_is_not_zero_on_a_homogeneous_dirichlet_side(ctx, as_array):
    """a flag given as None is g = 0 at every step, as UpdateBdc sets it: the initial state (a text, or an array) is 0.1 and more on those sides, the first step
    puts them on 0 as the host stepper does, and the solution agrees with it to the same 1e-10"""
    want, counts = host_steps(0.5, 2, U0_HOT)
    form = timed_form()
    d = stepping_driver(ctx, 0.5, 2, form)
    try:
        if as_array:
            xy = d.coords()
            d.set_initial(0.2 * (1 - xy[:, 0] * xy[:, 0]) + 0.1)
        else:
            d.set_initial(U0_HOT)
        sides = np.abs(np.abs(d.coords()[:, 1]) - 1.0) < 1e-12
        assert sides.any() and np.abs(d.solution()[sides]).min() >= 0.1 - 1e-15
        out = d.run(DT, NSTEPS, tol=TOL, max_newton=15, lin_maxit=30)
        u = d.solution()
        err = np.abs(u - want).max()
        print("initial state off the boundary values: |u - host stepper| = %.3e of %.3e, Newton iterations %s (host %s)"
              % (err, np.abs(want).max(), [len(o["newton_history"]) for o in out], list(counts)))
        assert all(o["converged"] for o in out)
        assert np.all(u[sides] == 0.0)
        assert err <= 1e-10 * np.abs(want).max()
        assert tuple(len(o["newton_history"]) for o in out) == counts
    finally:
        d.destroy()
        form.destroy()


@pytest.mark.parametrize("theta,p", [(1.0, 1), (0.5, 2)])
def test_temporal_orders_of_the_heat_equation(ctx, theta, p):
    """u_t = lap u on tri_box(4, 4, (0, 0), (1, 1)), linear family, one level (the exact solve), T = 0.1, against exp(-T M^-1 K) u0: steps 8, 16, 32, the last
    observed order within 0.15 of p (tests/test_transient_reference_host.py has the same figures from the host stepper)"""
    from femus_amd import capi
    from femus_amd.transient import TransientQuasilinearElements
    lv, free, M, K, u0 = tr.heat_system()
    exact = tr.heat_exact(free, M, K, u0)
    form = capi.TransientForm()
    d = TransientQuasilinearElements(ctx, lv, "linear", 1, form, dirichlet={f: None for f in (-2, -3, -4, -5)}, theta=theta)
    try:
        err = []
        for n in (8, 16, 32):
            d.set_initial(u0)
            out = d.run(tr.HEAT_T / n, n, tol=1e-6)
            assert all(o["converged"] for o in out) and abs(d.time - tr.HEAT_T) < 1e-14
            err.append(np.abs(d.solution() - exact).max())
        orders = tr.observed_orders(err)
        print("theta %g: errors %s, orders %s" % (theta, err, orders))
        assert err[0] > err[1] > err[2]
        assert abs(orders[-1] - p) <= 0.15
    finally:
        d.destroy()
        form.destroy()


def test_a_stationary_solution_is_a_fixed_point(ctx):
    """the result of QuasilinearElements.solve for form B of tests/test_gpu_quasilinear_solve.py (no t in it): in three Crank-Nicolson steps the first Newton
    iteration already has ||EPS||_2 < 1e-10 ||SOL||_2"""
    from femus_amd import capi
    from femus_amd.transient import TransientQuasilinearElements
    from test_gpu_quasilinear_solve import device_run, problem
    lv, fe, text, _, _, _, _, dirichlet, flux = problem("B")
    start = device_run(ctx, "B", 2, tol=0.0, max_newton=30, lin_maxit=30)
    assert start["converged"]
    form = capi.QuasilinearForm(**text)
    d = TransientQuasilinearElements(ctx, lv, fe, 2, form, dirichlet=dirichlet, flux=flux, theta=0.5)
    try:
        d.set_initial(start["solution"])
        out = d.run(0.1, 3, tol=1e-6, lin_maxit=30)
        first = [o["newton_history"][0][2] for o in out]
        print("||EPS|| / ||SOL|| of the first iteration of each step:", first)
        assert all(o["converged"] for o in out)
        assert all(r < 1e-10 for r in first)
        assert np.abs(d.solution() - start["solution"]).max() <= 1e-9 * np.abs(start["solution"]).max()
    finally:
        d.destroy()
        form.destroy()


def test_a_flagged_top_level(ctx):
    """two uniform levels and one refined where x > 0: the steps converge, and after them every hanging dof is its constraint row applied to the solution (1e-12)"""
    form = timed_form()
    d = stepping_driver(ctx, 0.5, 3, form, selective_levels=1, flag="x>0")
    try:
        d.set_initial(U0)
        out = d.run(DT, 3, tol=TOL, max_newton=15, lin_maxit=30)
        assert all(o["converged"] for o in out)
        hang, ptr, master, w = d.constraints
        u = d.solution()
        assert hang.size > 0
        gap = max(abs(u[h] - w[ptr[k]:ptr[k + 1]] @ u[master[ptr[k]:ptr[k + 1]]]) for k, h in enumerate(hang))
        print("flagged level: %d dofs, %d hanging, largest gap %.3e, Newton iterations %s" % (u.size, hang.size, gap, [len(o["newton_history"]) for o in out]))
        assert gap <= 1e-12
        assert np.isfinite(u).all() and np.abs(u).max() > 0.01
    finally:
        d.destroy()
        form.destroy()


def test_run_is_its_steps_and_a_second_driver_after_destroy(ctx):
    """run(dt, n) equals n times step + copy_solution_to_old bit for bit; destroy() frees everything, and a second driver on the same context works"""
    form = timed_form()
    kw = dict(tol=TOL, max_newton=15, lin_maxit=30)
    try:
        d = stepping_driver(ctx, 0.5, 2, form)
        try:
            d.set_initial(U0)
            a = d.run(DT, 3, **kw)
            ua = d.solution()
        finally:
            d.destroy()
        d = stepping_driver(ctx, 0.5, 2, form)
        try:
            d.set_initial(U0)
            b = []
            for _ in range(3):
                b.append(d.step(DT, **kw))
                d.copy_solution_to_old()
            ub = d.solution()
            norms = d.error_norms(lambda t: "0.3*(1-y*y)*%r" % t)
        finally:
            d.destroy()
        assert np.array_equal(ua.view(np.uint64), ub.view(np.uint64))
        assert a == b
        assert np.isfinite(norms["l2"]) and norms["l2"] > 0
    finally:
        form.destroy()


def test_a_flux_over_time_is_refused(ctx):
    from femus_amd import capi
    from femus_amd.transient import TransientQuasilinearElements
    form = timed_form()
    e = capi.Expr("0.5*(1+y)*t", "x,y,z,t")
    try:
        for flux in ({-3: e}, {-3: "0.5*(1+y)*t"}):
            with pytest.raises(ValueError, match="x, y, z only, a time-dependent flux is not served"):
                TransientQuasilinearElements(ctx, level0(), FE, 1, form, dirichlet={-5: G_LEFT}, flux=flux)
    finally:
        e.destroy()
        form.destroy()
