"""femus_amd.quasilinear.QuasilinearElements: Newton on resident element meshes against a host Newton on the system of tests/quasilinear_reference.py solved
with scipy's sparse LU, the one-level exact solve, the convergence orders against a manufactured solution, and a flagged top level.

Form B (ex03b plus a reaction), -div((1 + u^2) grad u) + sqrt(1 + u^2) = f, on tri_box(2, 2, (-1, -1), (1, 1)) with u_e = sin(pi x) cos(pi y / 2): the flux
a(u_e) du_e/dn on the right side (flag -3), u_e on the other three.  With lap u_e = -(5 pi^2 / 4) u_e:
    f = (1 + u_e^2) (5 pi^2 / 4) u_e - 2 u_e |grad u_e|^2 + sqrt(1 + u_e^2).
Form A (ex03), -lap u + u (ux + uy + uz) = f, on cube_Tet.neu with u_e = cos(pi x) cos(pi y) cos(pi z), Dirichlet everywhere:
    f = 3 pi^2 u_e + u_e (du_e/dx + du_e/dy + du_e/dz).
A wrong f would show in the convergence orders below."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import quasilinear_reference as qr
from femus_amd import mixed_mesh

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

UE2 = "(sin(pi*x)*cos(pi*y/2))"
UE2_X, UE2_Y = "(pi*cos(pi*x)*cos(pi*y/2))", "(-pi/2*sin(pi*x)*sin(pi*y/2))"
F_B = "(1+U*U)*(5*pi*pi/4)*U-2*U*(UX*UX+UY*UY)+sqrt(1+U*U)".replace("UX", UE2_X).replace("UY", UE2_Y).replace("U", UE2)
FLUX_B = "(1+U*U)*UX".replace("UX", UE2_X).replace("U", UE2)
UE3 = "(cos(pi*x)*cos(pi*y)*cos(pi*z))"
UE3_D = ["(-pi*sin(pi*x)*cos(pi*y)*cos(pi*z))", "(-pi*cos(pi*x)*sin(pi*y)*cos(pi*z))", "(-pi*cos(pi*x)*cos(pi*y)*sin(pi*z))"]
F_A = "3*pi*pi*U+U*(%s)".replace("U", UE3) % "+".join(UE3_D)


def problem(name):
    """(level0, fe, form texts, form callables, source text, exact text, gradient texts, {Dirichlet flag: text}, {flux flag: text})"""
    if name == "B":
        lv = mixed_mesh.tri_box(2, 2, (-1., -1.), (1., 1.))
        text, call = qr.form_b(2)
        return lv, "biquadratic", dict(text, f=F_B), call, F_B, UE2, [UE2_X, UE2_Y], {-2: UE2, -4: UE2, -5: UE2}, {-3: FLUX_B}
    lv = mixed_mesh.read_gambit(os.path.join(GOLDEN, "cube_Tet.neu"))
    text, call = qr.form_a(3)
    flags = sorted(int(f) for f in np.unique(lv[3]) if f < -1)
    return lv, "serendipity", dict(text, f=F_A), call, F_A, UE3, UE3_D, {f: UE3 for f in flags}, {}


def host_flux(kind, ed, xs, ff, fe, flux):
    """sum over the flux edges of a two-dimensional mesh of int phi_i tau ds: the line element's own tables, its nodes in the order ends, then middle"""
    from femus_amd import capi
    b = np.zeros(int(ed.max()) + 1)
    w, _ = capi.fe_gauss("line", ORDER["B"])
    phi, dphi = capi.fe_tables("line", fe, ORDER["B"])
    for e, f in zip(*np.nonzero(ff < -1)):
        if int(ff[e, f]) not in flux:
            continue
        nodes = ed[e, capi.fe_face_nodes(kind[e], fe, f)]
        x = xs[nodes]
        for g in range(w.size):
            t = dphi[g, :, 0] @ x
            xg = np.zeros(4)
            xg[:2] = phi[g] @ x
            b[nodes] += phi[g] * flux[int(ff[e, f])](xg) * np.hypot(*t) * w[g]
    return b


@functools.lru_cache(maxsize=None)
def host_newton(name, nlevels):
    """(solution, Newton steps) of the host Newton on the restatement's system, the steps counted as the driver stops: until ||EPS||_2 < 1e-12"""
    from femus_amd import capi
    lv, fe, _, call, f_text, _, _, dirichlet, flux = problem(name)
    for _ in range(1, nlevels):
        lv = mixed_mesh.refine(*lv[:4])
    kind, ed, xs, ff, own = lv
    dim, ndof = xs.shape[1], own[qr.FAM[fe]]
    exprs = {t: capi.Expr(t, "x,y,z,t") for t in set(dirichlet.values()) | set(flux.values()) | {f_text}}
    fx = exprs[f_text]
    form = dict(call, f=lambda v: fx(np.array([v[0], v[1], v[2], 0.0])))
    u = np.zeros(ndof)
    for e, f in zip(*np.nonzero(ff < -1)):                          # elements and faces in order; a later face overwrites an earlier one
        if int(ff[e, f]) in dirichlet:
            for n in ed[e, capi.fe_face_nodes(kind[e], fe, f)]:
                x4 = np.zeros(4)
                x4[:dim] = xs[n]
                u[n] = exprs[dirichlet[int(ff[e, f])]](x4)
    fixed = np.array(sorted({int(n) for e, f in zip(*np.nonzero(ff < -1)) if int(ff[e, f]) in dirichlet for n in ed[e, capi.fe_face_nodes(kind[e], fe, f)]}))
    b = host_flux(kind, ed, xs, ff, fe, {k: exprs[t] for k, t in flux.items()}) if flux else np.zeros(ndof)
    free = np.ones(ndof, bool)
    free[fixed] = False
    D = sp.diags(free.astype(float))
    steps = 0
    for steps in range(1, 31):
        K, F = qr.assemble(kind, ed, xs, fe, form, u, order=ORDER[name])
        F = (F + b[:ndof]) * free
        du = spla.splu(sp.csc_matrix(D @ K @ D + sp.diags(1.0 - free))).solve(F)
        u += du
        if np.linalg.norm(du) < 1e-12:
            break
    for e in exprs.values():
        e.destroy()
    u.setflags(write=False)
    return u, steps


ORDER = {"B": "seventh", "A": "fifth"}          # the Gauss rule of both sides; the lower one keeps the host Newton on 840 tetrahedra to a few seconds


def device_run(ctx, name, nlevels, fe=None, **kw):
    from femus_amd import capi
    from femus_amd.quasilinear import QuasilinearElements
    lv, fe0, text, _, _, ue, grad, dirichlet, flux = problem(name)
    form = capi.QuasilinearForm(**text)
    exprs = {t: capi.Expr(t, "x,y,z,t") for t in set(dirichlet.values()) | set(flux.values())}
    try:
        q = QuasilinearElements(ctx, lv, fe or fe0, nlevels, form, dirichlet={k: exprs[t] for k, t in dirichlet.items()}, flux={k: exprs[t] for k, t in flux.items()},
                                order=ORDER[name])
        return q.solve(exact=ue, exact_gradient=grad[:lv[2].shape[1]], **kw)
    finally:
        form.destroy()
        for e in exprs.values():
            e.destroy()


@pytest.mark.parametrize("nlevels", [2, 1])
@pytest.mark.parametrize("name", ["B", "A"])
def test_newton_against_a_host_newton_with_a_direct_solve(ctx, name, nlevels):
    """tol cannot be reached, so ||EPS||_2 < 1e-12 stops the iteration; two levels: V-cycle-preconditioned GMRES of at most 30 steps; one level: the exact solve.
    The solution within 1e-10 max |u| of the host Newton's (the project's bound for solutions against direct solves), in no more Newton steps than it plus one"""
    want, steps = host_newton(name, nlevels)
    out = device_run(ctx, name, nlevels, tol=0.0, max_newton=30, lin_maxit=30)
    d = np.abs(out["solution"] - want).max()
    print("form %s, %d levels: %d dofs, |u - host Newton| = %.3e of %.3e, Newton steps %d (host %d), history %s"
          % (name, nlevels, out["dofs"], d, np.abs(want).max(), len(out["newton_history"]), steps, out["newton_history"]))
    assert out["converged"]
    assert d <= 1e-10 * np.abs(want).max()
    assert len(out["newton_history"]) <= steps + 1
    if nlevels == 1:
        assert all(h[0] <= 1 for h in out["newton_history"])


@pytest.mark.parametrize("fe,p", [("linear", 1), ("biquadratic", 2)])
def test_convergence_orders_of_form_b_on_the_triangle_box(ctx, fe, p):
    """errors fall from level to level, and the last observed orders are within 0.15 of p + 1 (L2) and p (H1 semi-norm): the margin of
    tests/test_gpu_convergence_rates.py"""
    runs = [device_run(ctx, "B", nl, fe=fe, tol=1e-11, max_newton=30, lin_maxit=30) for nl in (2, 3, 4)]
    l2, h1 = [r["l2_error"] for r in runs], [r["h1_error"] for r in runs]
    o2, o1 = np.log2(l2[-2] / l2[-1]), np.log2(h1[-2] / h1[-1])
    print("%s: L2 errors %s, H1 errors %s, last orders %.3f and %.3f" % (fe, l2, h1, o2, o1))
    assert all(r["converged"] for r in runs)
    assert l2[0] > l2[1] > l2[2] and h1[0] > h1[1] > h1[2]
    assert abs(o2 - (p + 1)) <= 0.15
    assert abs(o1 - p) <= 0.15


def test_a_flagged_top_level(ctx):
    """two uniform levels and one refined where x > 0: Newton converges, every hanging dof is its constraint row applied to the solution (1e-12), and the L2
    error is not larger than that of the uniform hierarchy below it"""
    below = device_run(ctx, "B", 2, tol=1e-11, max_newton=30, lin_maxit=30)
    out = device_run(ctx, "B", 3, tol=1e-11, max_newton=30, lin_maxit=30, selective_levels=1, flag="x>0")
    assert out["converged"] and below["converged"]
    hang, ptr, master, w = out["constraints"]
    u = out["solution"]
    assert hang.size > 0 and np.array_equal(hang, out["hanging"])
    gap = max(abs(u[h] - w[ptr[k]:ptr[k + 1]] @ u[master[ptr[k]:ptr[k + 1]]]) for k, h in enumerate(hang))
    print("flagged level: %d dofs, %d hanging, largest gap %.3e, L2 error %.6e (uniform level below: %.6e)" % (out["dofs"], hang.size, gap, out["l2_error"],
                                                                                                          below["l2_error"]))
    assert gap <= 1e-12
    assert out["l2_error"] <= below["l2_error"]
