"""femus_amd.transient.TransientSystemElements: theta-steps of coupled systems on resident element meshes against the host stepper of
tests/system_transient_reference.py (Newton on the restatement's system with scipy's sparse LU); the time-dependent ex04 with its algebraic equation; the
temporal orders against the semi-discrete exact solution; a stationary solution as a fixed point; a flagged top level; run() against its steps and a second
driver after destroy().  tri_box meshes of the sizes tests/test_gpu_transient_solve.py uses (at most three levels from 2 x 2; the linear problems: 4 x 4), and its
bounds: 1e-10 of the host stepper's largest entry and the same Newton counts.

The stepping problem: form S of tests/system_reference.py (m = 2) with its sources times 1 + t on (-1, 1)^2.  u_0: on the left side (flag -5) 0.3 (1 - y^2) t, 0 on
the bottom and top sides (-2, -4), the flux 0.5 (1 + y) on the right side (-3).  u_1: 0.1 (1 - y^2) t on the right side, 0 on the left side, natural elsewhere.
U(0) = (0.2, 0.1) (1 - x^2) (1 - y^2).
The time-dependent ex04, u_t + lap lap u = f as (u, v = -lap u) on (-0.5, 0.5)^2 with u = v = 0 on the boundary:
  equation 0:  u_t - lap v = f            M_00 = 1, A_00 = 0, A_01 = 1
  equation 1:  -lap u - v = 0             algebraic (row 1 of M is zero): A_10 = 1, A_11 = 0, c_1 = -u1
f = 4 pi^4 cos(pi x) cos(pi y) (1 + t), u(0) = 0.1 cos(pi x) cos(pi y), v(0) = 2 pi^2 u(0)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import quasilinear_reference as qr
import system_reference as sr
import system_transient_reference as st
import transient_reference as tr
from femus_amd import mixed_mesh

pytestmark = pytest.mark.gpu
DT, NSTEPS, TOL = 0.05, 3, 1e-9
FE = "biquadratic"
DIRICHLET = [{-5: "0.3*(1-y*y)*t", -2: None, -4: None}, {-3: "0.1*(1-y*y)*t", -5: None}]
FLUX = [{-3: "0.5*(1+y)"}, {}]
U0 = ["0.2*(1-x*x)*(1-y*y)", "0.1*(1-x*x)*(1-y*y)"]
KW = dict(tol=TOL, max_newton=15, lin_maxit=30)

UE = "(cos(pi*x)*cos(pi*y))"
EX04_TEXT = dict(m=2, A=[["0", "1"], ["1", "0"]], f=["4*pi*pi*pi*pi*%s*(1+t)" % UE, None], c=[None, "-u1"], c_u=[[None, None], [None, "-1"]])
EX04_M = [[1.0, 0.0], [0.0, 0.0]]
EX04_U0 = ["0.1*%s" % UE, "0.2*pi*pi*%s" % UE]
ALL = (-2, -3, -4, -5)
KAPPA = 2.0


def level0():
    return mixed_mesh.tri_box(2, 2, (-1., -1.), (1., 1.))


def refined(lv, nlevels):
    for _ in range(1, nlevels):
        lv = mixed_mesh.refine(*lv[:4])
    return lv


def at_dofs(texts, lv, ndof):
    from femus_amd import capi
    x4 = np.zeros((ndof, 4))
    x4[:, :2] = lv[2][:ndof]
    out = []
    for t in texts:
        e = capi.Expr(t, "x,y,z,t")
        out.append(e(x4))
        e.destroy()
    return np.array(out)


def host_run(lv, fe, form, dirichlet, flux, M, theta, u0, dt, nsteps, tol=TOL):
    """(the solution [m, ndof] after every step, Newton iterations of every step) of the host stepper; the texts compiled over x, y, z, t"""
    from femus_amd import capi
    made = []

    def compiled(d):
        out = {}
        for f, t in d.items():
            out[f] = None if t is None else capi.Expr(t, "x,y,z,t")
            made.append(out[f])
        return out

    s = st.HostStepper(lv, fe, form, [compiled(d) for d in dirichlet], [compiled(d) for d in flux], M=M, theta=theta)
    s.set_initial(at_dofs(u0, lv, s.ndof))
    states, counts = [], []
    for _ in range(nsteps):
        counts.append(s.step(dt, tol=tol, max_newton=15))
        s.copy_solution_to_old()
        states.append(s.solution().copy())
    for e in made:
        if e is not None:
            e.destroy()
    return states, tuple(counts)


@functools.lru_cache(maxsize=None)
def host_steps(theta, nlevels):
    return host_run(refined(level0(), nlevels), FE, st.form_s(2)[1], DIRICHLET, FLUX, None, theta, U0, DT, NSTEPS)


def stepping_driver(ctx, theta, nlevels, form, **kw):
    from femus_amd.transient import TransientSystemElements
    return TransientSystemElements(ctx, level0(), FE, nlevels, form, dirichlet=DIRICHLET, flux=FLUX, theta=theta, **kw)


def timed_form():
    from femus_amd import capi
    return capi.TransientSystemForm(**st.form_s(2)[0])


@pytest.mark.parametrize("nlevels", [2, 1])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_steps_against_the_host_stepper(ctx, theta, nlevels):
    """three steps: every variable within 1e-10 of the host stepper's largest entry, and the same number of Newton iterations in every step"""
    states, counts = host_steps(theta, nlevels)
    want = states[-1]
    form = timed_form()
    d = stepping_driver(ctx, theta, nlevels, form)
    try:
        d.set_initial(U0)
        out = d.run(DT, NSTEPS, **KW)
        u = d.solution()
        err = [np.abs(u[k] - want[k]).max() / np.abs(want[k]).max() for k in range(2)]
        print("theta %g, %d levels: |u_k - host stepper| / max |u_k| = %s, Newton iterations %s (host %s)"
              % (theta, nlevels, err, [len(o["newton_history"]) for o in out], list(counts)))
        assert u.shape == want.shape and all(o["converged"] for o in out)
        assert abs(d.time - NSTEPS * DT) < 1e-14 and abs(out[-1]["time"] - d.time) == 0.0
        assert max(err) <= 1e-10
        assert tuple(len(o["newton_history"]) for o in out) == counts
        if nlevels == 1:
            assert all(h[0] <= 1 for o in out for h in o["newton_history"])
    finally:
        d.destroy()
        form.destroy()


def test_the_time_dependent_ex04_takes_its_constraint_at_the_new_time(ctx):
    """one level with the exact solve, Crank-Nicolson: u and v agree with the host stepper after every step, and after every step the rows of the algebraic
    equation vanish in the stationary residual at the new state, -lap u - v = 0 -- at theta = 0.5 for that equation they would not"""
    from femus_amd import capi
    from femus_amd.transient import TransientSystemElements
    lv = mixed_mesh.tri_box(4, 4, (-0.5, -0.5), (0.5, 0.5))
    one, zero = (lambda V: np.ones(len(V))), (lambda V: np.zeros(len(V)))
    f0 = capi.Expr("4*pi*pi*pi*pi*%s" % UE, "x,y,z,t")
    source = lambda V: f0(np.concatenate([V[:, :3], np.zeros((len(V), 1))], axis=1))
    call = lambda t: dict(m=2, A=[[zero, one], [one, zero]], f=[lambda V: source(V) * (1 + t), None], c=[None, lambda V: -V[:, 4]],
                          c_u=[[None, None], [None, lambda V: -one(V)]])
    dirichlet = [{f: None for f in ALL}] * 2
    theta, dt, nsteps = 0.5, 0.01, 3
    states, counts = host_run(lv, FE, call, dirichlet, [{}, {}], EX04_M, theta, EX04_U0, dt, nsteps)
    form = capi.TransientSystemForm(**EX04_TEXT)
    d = TransientSystemElements(ctx, lv, FE, 1, form, dirichlet=dirichlet, mass=EX04_M, theta=theta)
    try:
        d.set_initial(EX04_U0)
        n = d.solution().shape[1]
        free = np.ones(n, bool)
        free[[node for _, node in tr.boundary_nodes(lv[0], lv[1], lv[3], FE, set(ALL))]] = False
        for step in range(nsteps):
            out = d.step(dt, **KW)
            d.copy_solution_to_old()
            u = d.solution()
            err = [np.abs(u[k] - states[step][k]).max() / np.abs(states[step][k]).max() for k in range(2)]
            F = sr.assemble(lv[0], lv[1], lv[2], FE, call(d.time), u)[1]
            gap = np.abs(F[n:][free]).max() / np.abs(sr.assemble(lv[0], lv[1], lv[2], FE, call(d.time), np.stack([u[0], 0 * u[1]]))[1][n:][free]).max()
            print("step %d: |u - host| = %.3e, |v - host| = %.3e (relative), constraint rows %.3e of their lap u part, Newton iterations %d (host %d)"
                  % (step + 1, err[0], err[1], gap, len(out["newton_history"]), counts[step]))
            assert out["converged"] and max(err) <= 1e-10
            assert len(out["newton_history"]) == counts[step]
            assert all(h[0] <= 1 for h in out["newton_history"])
            assert gap <= 1e-9
        assert np.abs(states[-1][1] - states[0][1]).max() > 1e-3 * np.abs(states[0][1]).max()       # v moves: the agreement is not that of a standstill
    finally:
        d.destroy()
        form.destroy()
        f0.destroy()


@pytest.mark.parametrize("theta,p", [(1.0, 1), (0.5, 2)])
def test_temporal_orders_of_two_coupled_heat_equations(ctx, theta, p):
    """d_t u_0 = lap u_0 - kappa u_1, d_t u_1 = lap u_1 - kappa u_0 (c_0 = kappa u1, c_1 = kappa u0, kappa = 2) on tri_box(4, 4, (0, 0), (1, 1)), linear family,
    one level, T = 0.1, against exp(-T M^-1 K) U0 on the block matrices M = kron(1, Mass), K = [[K, kappa Mass], [kappa Mass, K]]: steps 8, 16, 32, the last
    observed order within 0.15 of p, as tests/test_gpu_transient_solve.py asserts it"""
    from femus_amd import capi
    from femus_amd.transient import TransientSystemElements
    lv, free, M, K, u0 = tr.heat_system()
    U0h = np.concatenate([u0, -0.5 * u0])
    MM = sp.kron(sp.identity(2), M, format="csr")
    KK = (sp.kron(sp.identity(2), K) + KAPPA * sp.kron(sp.csr_matrix([[0.0, 1.0], [1.0, 0.0]]), M)).tocsr()
    exact = tr.heat_exact(np.concatenate([free, free]), MM, KK, U0h).reshape(2, -1)
    form = capi.TransientSystemForm(2, c=["%r*u1" % KAPPA, "%r*u0" % KAPPA], c_u=[[None, "%r" % KAPPA], ["%r" % KAPPA, None]])
    d = TransientSystemElements(ctx, lv, "linear", 1, form, dirichlet=[{f: None for f in ALL}] * 2, theta=theta)
    try:
        err = []
        for n in (8, 16, 32):
            d.set_initial(U0h.reshape(2, -1))
            out = d.run(tr.HEAT_T / n, n, tol=1e-6)
            assert all(o["converged"] for o in out) and abs(d.time - tr.HEAT_T) < 1e-14
            err.append(np.abs(d.solution() - exact).max())
        orders = tr.observed_orders(err)
        print("theta %g: errors %s, orders %s" % (theta, err, orders))
        assert err[0] > err[1] > err[2]
        assert abs(orders[-1] - p) <= 0.15
        assert np.abs(exact[1] + 0.5 * exact[0]).max() > 1e-3 * np.abs(exact).max()                # the coupling has acted
    finally:
        d.destroy()
        form.destroy()


def test_a_stationary_solution_is_a_fixed_point(ctx):
    """the result of SystemElements.solve for form S with the manufactured source of tests/test_gpu_system_solve.py (no t in it): in three Crank-Nicolson steps
    the first Newton iteration already has ||EPS||_2 < 1e-10 ||SOL||_2"""
    from femus_amd import capi
    from femus_amd.transient import TransientSystemElements
    from test_gpu_system_solve import device_run, problem
    lv, text, _, _, _, dirichlet, flux = problem("S-faces")
    start = device_run(ctx, "S-faces", 2, tol=0.0, max_newton=30, lin_maxit=30)
    assert start["converged"]
    form = capi.SystemForm(**text)
    d = TransientSystemElements(ctx, lv, FE, 2, form, dirichlet=dirichlet, flux=flux, theta=0.5)
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
    """two uniform levels and one refined where x > 0: the steps converge, and after them every hanging dof of every variable is its constraint row applied to
    the solution (1e-12)"""
    form = timed_form()
    d = stepping_driver(ctx, 0.5, 3, form, selective_levels=1, flag="x>0")
    try:
        d.set_initial(U0)
        out = d.run(DT, 3, **KW)
        assert all(o["converged"] for o in out)
        hang, ptr, master, w = d.constraints
        assert hang.size > 0
        for k, u in enumerate(d.solution()):
            gap = max(abs(u[h] - w[ptr[j]:ptr[j + 1]] @ u[master[ptr[j]:ptr[j + 1]]]) for j, h in enumerate(hang))
            print("flagged level, variable %d: %d dofs, %d hanging, largest gap %.3e, Newton iterations %s" % (k, u.size, hang.size, gap,
                                                                                                              [len(o["newton_history"]) for o in out]))
            assert gap <= 1e-12
            assert np.isfinite(u).all() and np.abs(u).max() > 0.01
    finally:
        d.destroy()
        form.destroy()


def test_run_is_its_steps_and_a_second_driver_after_destroy(ctx):
    """run(dt, n) equals n times step + copy_solution_to_old bit for bit; destroy() frees everything, and a second driver on the same context works; the
    initial state as an array is the one as texts; error_norms has one entry per variable"""
    form = timed_form()
    try:
        d = stepping_driver(ctx, 0.5, 2, form)
        try:
            d.set_initial(U0)
            start = d.solution()
            a = d.run(DT, 3, **KW)
            ua = d.solution()
        finally:
            d.destroy()
        d = stepping_driver(ctx, 0.5, 2, form)
        try:
            d.set_initial(start)
            b = []
            for _ in range(3):
                b.append(d.step(DT, **KW))
                d.copy_solution_to_old()
            ub = d.solution()
            norms = d.error_norms([lambda t: "0.3*(1-y*y)*%r" % t, "0"])
        finally:
            d.destroy()
        assert ua.shape == (2, start.shape[1]) and np.array_equal(ua.view(np.uint64), ub.view(np.uint64))
        assert a == b
        assert len(norms["l2"]) == len(norms["h1"]) == 2 and all(np.isfinite(v) and v > 0 for v in norms["l2"])
    finally:
        form.destroy()


def test_what_the_driver_refuses(ctx):
    from femus_amd import capi
    from femus_amd.transient import TransientSystemElements
    form = timed_form()
    e = capi.Expr("0.5*(1+y)*t", "x,y,z,t")
    try:
        for flux in ([{-3: e}, {}], [{}, {-3: "0.5*(1+y)*t"}]):
            with pytest.raises(ValueError, match="x, y, z only, a time-dependent flux is not served"):
                TransientSystemElements(ctx, level0(), FE, 1, form, dirichlet=[{-5: "t"}, {}], flux=flux)
        with pytest.raises(ValueError, match="one dict per variable"):
            TransientSystemElements(ctx, level0(), FE, 1, form, dirichlet=[{-5: "t"}])
        with pytest.raises(ValueError, match="variable 1: face flags \\[-3\\] are both"):
            TransientSystemElements(ctx, level0(), FE, 1, form, dirichlet=[{}, {-3: None}], flux=[{}, {-3: "1"}])
        with pytest.raises(ValueError, match="mass must be a finite 2 x 2 matrix"):
            TransientSystemElements(ctx, level0(), FE, 1, form, mass=np.eye(3))
        with pytest.raises(ValueError, match="theta must be in"):
            TransientSystemElements(ctx, level0(), FE, 1, form, theta=1.5)
        d = TransientSystemElements(ctx, level0(), FE, 1, form, dirichlet=DIRICHLET)
        try:
            with pytest.raises(ValueError, match="initial state has shape"):
                d.set_initial(np.zeros(7))
            with pytest.raises(ValueError, match="dt must be positive"):
                d.step(0.0)
        finally:
            d.destroy()
    finally:
        e.destroy()
        form.destroy()
