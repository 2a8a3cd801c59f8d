"""femus_amd.system.SystemElements: Newton for coupled systems on resident element meshes against a host Newton on the system of tests/system_reference.py
solved with scipy's sparse LU; ex04 (the biharmonic equation as two coupled Laplacians) in both row orders; convergence orders of both variables; Dirichlet
faces that differ per variable; a flagged top level.  Triangle boxes, as tests/test_gpu_quasilinear_solve.py.

ex04 on [-0.5, 0.5]^2, u = v = 0 on the boundary, f = 4 pi^4 cos(pi x) cos(pi y):  u_e = cos(pi x) cos(pi y),  v_e = lap u_e = -2 pi^2 u_e.
  "reference": row u is -lap v = -f, row v is -lap u + v = 0     (A_00 = A_11 = 0, A_01 = A_10 = 1, c_1 = u1): diagonal blocks 0 and M, the exact solve
  "exchanged": row 0 is -lap u + v = 0, row 1 is -lap v = -f     (KK = [[K, M], [0, K]]): multigrid
Form S of tests/system_reference.py (m = 2) on [-1, 1]^2 with the manufactured solution
  u0_e = sin(pi x) cos(pi y / 2),  u1_e = cos(pi x / 2) sin(pi y) / 2     (lap u_e = -(5 pi^2 / 4) u_e for both):
  f_0 = -[(1 + u0^2) lap u0 + 2 u0 |grad u0|^2] - [(0.5 + x) lap u1 + d_x u1] + u0 d_x u0 + u1 d_y u0
  f_1 = -[u0 u1 lap u0 + (u1 grad u0 + u0 grad u1) . grad u0] - [(1 + u1^2) lap u1 + 2 u1 |grad u1|^2] + u0 d_x u1 + u1 d_y u1
A wrong f would show in the errors against the exact solution, which must fall from one level to two."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import quasilinear_reference as qr
import system_reference as sr
from femus_amd import mixed_mesh
from test_gpu_quasilinear_solve import host_flux

pytestmark = pytest.mark.gpu
ORDER = "seventh"

UE = "(cos(pi*x)*cos(pi*y))"
UE_D = ["(-pi*sin(pi*x)*cos(pi*y))", "(-pi*cos(pi*x)*sin(pi*y))"]
VE, VE_D = "(-2*pi*pi*%s)" % UE, ["(-2*pi*pi*%s)" % d for d in UE_D]
F04 = "(4*pi*pi*pi*pi*%s)" % UE

T = dict(u0="(sin(pi*x)*cos(pi*y/2))", u0x="(pi*cos(pi*x)*cos(pi*y/2))", u0y="(-pi/2*sin(pi*x)*sin(pi*y/2))",
         u1="(0.5*cos(pi*x/2)*sin(pi*y))", u1x="(-pi/4*sin(pi*x/2)*sin(pi*y))", u1y="(pi/2*cos(pi*x/2)*cos(pi*y))")
T["u0l"], T["u1l"] = "(-5*pi*pi/4*%s)" % T["u0"], "(-5*pi*pi/4*%s)" % T["u1"]
FS = ["-((1+{u0}*{u0})*{u0l}+2*{u0}*({u0x}*{u0x}+{u0y}*{u0y}))-((0.5+x)*{u1l}+{u1x})+{u0}*{u0x}+{u1}*{u0y}".format(**T),
      ("-({u0}*{u1}*{u0l}+({u1}*{u0x}+{u0}*{u1x})*{u0x}+({u1}*{u0y}+{u0}*{u1y})*{u0y})-((1+{u1}*{u1})*{u1l}+2*{u1}*({u1x}*{u1x}+{u1y}*{u1y}))"
       "+{u0}*{u1x}+{u1}*{u1y}").format(**T)]
FLUX_S1 = "{u0}*{u1}*{u0x}+(1+{u1}*{u1})*{u1x}".format(**T)          # A_10 d_x u0 + A_11 d_x u1 on the right side (flag -3, normal +x)
ALL = (-2, -3, -4, -5)


def problem(name):
    """(level0, form texts, form callables with f still a text, exact texts, exact gradient texts, [Dirichlet {flag: text or None}], [flux {flag: text}])"""
    if name in ("ex04-reference", "ex04-exchanged"):
        lv = mixed_mesh.tri_box(2, 2, (-0.5, -0.5), (0.5, 0.5))
        one, zero, v = (lambda V: np.ones(len(V))), (lambda V: np.zeros(len(V))), (lambda V: V[:, 4])
        if name == "ex04-reference":
            text = dict(m=2, A=[["0", "1"], ["1", "0"]], f=["-" + F04, None], c=[None, "u1"], c_u=[[None, None], [None, "1"]])
            call = dict(m=2, A=[[zero, one], [one, zero]], f=["-" + F04, None], c=[None, v], c_u=[[None, None], [None, one]])
        else:
            text = dict(m=2, f=[None, "-" + F04], c=["u1", None], c_u=[[None, "1"], [None, None]])
            call = dict(m=2, f=[None, "-" + F04], c=[v, None], c_u=[[None, one], [None, None]])
        return lv, text, call, [UE, VE], [UE_D, VE_D], [{f: None for f in ALL}] * 2, [{}, {}]
    lv = mixed_mesh.tri_box(2, 2, (-1., -1.), (1., 1.))
    text, call = sr.form_s(2)
    text, call = dict(text, f=FS), dict(call, f=FS)
    exact, grad = [T["u0"], T["u1"]], [[T["u0x"], T["u0y"]], [T["u1x"], T["u1y"]]]
    if name == "S":
        return lv, text, call, exact, grad, [{f: T["u0"] for f in ALL}, {f: T["u1"] for f in ALL}], [{}, {}]
    assert name == "S-faces"              # u_0 Dirichlet on all of the boundary; u_1 Dirichlet on the left side alone, a flux on the right, natural elsewhere
    left = [f for f in ALL if f != -3][0]
    return lv, text, call, exact, grad, [{f: T["u0"] for f in ALL}, {left: T["u1"]}], [{}, {-3: FLUX_S1}]


@functools.lru_cache(maxsize=None)
def host_newton(name, nlevels, fe="biquadratic"):
    """(solution [m, ndof], Newton steps) of the host Newton on the restatement's system, the steps counted as the driver stops: until ||EPS||_2 < 1e-12"""
    from femus_amd import capi
    lv, _, call, _, _, dirichlet, flux = problem(name)
    for _ in range(1, nlevels):
        lv = mixed_mesh.refine(*lv[:4])
    kind, ed, xs, ff, own = lv
    assert sorted(int(f) for f in np.unique(ff[ff < -1])) == sorted(ALL)
    m, dim, ndof = call["m"], xs.shape[1], own[qr.FAM[fe]]
    texts = {t for d in dirichlet + flux for t in d.values() if t is not None} | {t for t in call["f"] if t is not None}
    exprs = {t: capi.Expr(t, "x,y,z,t") for t in texts}
    at_points = lambda e: (lambda V: e(np.concatenate([V[:, :3], np.zeros((len(V), 1))], axis=1)))
    form = dict(call, f=[at_points(exprs[t]) if t is not None else None for t in call["f"]])
    u, free, b = np.zeros((m, ndof)), np.ones((m, ndof), bool), np.zeros((m, ndof))
    for k in range(m):
        for e, f in zip(*np.nonzero(ff < -1)):                      # elements and faces in order; a later face overwrites an earlier one
            if int(ff[e, f]) in dirichlet[k]:
                t = dirichlet[k][int(ff[e, f])]
                for n in ed[e, capi.fe_face_nodes(kind[e], fe, f)]:
                    x4 = np.zeros(4)
                    x4[:dim] = xs[n]
                    u[k, n], free[k, n] = (exprs[t](x4) if t is not None else 0.0), False
        if flux[k]:
            b[k] = host_flux(kind, ed, xs, ff, fe, {g: exprs[t] for g, t in flux[k].items()})[:ndof]
    free, b = free.ravel().astype(float), b.ravel()
    D = sp.diags(free)
    steps = 0
    for steps in range(1, 31):
        K, F = sr.assemble(kind, ed, xs, fe, form, u, order=ORDER)
        du = spla.splu(sp.csc_matrix(D @ K @ D + sp.diags(1.0 - free))).solve((F + b) * free)
        u += du.reshape(m, ndof)
        if np.linalg.norm(du) < 1e-12:
            break
    for e in exprs.values():
        e.destroy()
    u.setflags(write=False)
    return u, steps


def device_run(ctx, name, nlevels, fe="biquadratic", **kw):
    from femus_amd import capi
    from femus_amd.system import SystemElements
    lv, text, _, exact, grad, dirichlet, flux = problem(name)
    form = capi.SystemForm(**text)
    exprs = {t: capi.Expr(t, "x,y,z,t") for d in dirichlet + flux for t in d.values() if t is not None}
    of = lambda d: {k: exprs[t] if t is not None else None for k, t in d.items()}
    try:
        q = SystemElements(ctx, lv, fe, nlevels, form, dirichlet=[of(d) for d in dirichlet], flux=[of(d) for d in flux], order=ORDER)
        return q.solve(exact=exact, exact_gradient=grad, **kw)
    finally:
        form.destroy()
        for e in exprs.values():
            e.destroy()


def against_host(ctx, name, nlevels, **kw):
    want, steps = host_newton(name, nlevels)
    out = device_run(ctx, name, nlevels, tol=0.0, max_newton=30, lin_maxit=30, **kw)
    d = [np.abs(out["solution"][k] - want[k]).max() / np.abs(want[k]).max() for k in range(len(want))]
    print("%s, %d levels: %d dofs per variable, |U - host Newton| / max |u_k| = %s, Newton steps %d (host %d), history %s, L2 errors %s"
          % (name, nlevels, out["dofs"], d, len(out["newton_history"]), steps, out["newton_history"], out["l2_error"]))
    assert out["solution"].shape == want.shape
    assert out["converged"]
    assert max(d) <= 1e-10
    assert len(out["newton_history"]) <= steps + 1
    return out


def test_ex04_in_the_reference_row_order_on_one_level(ctx):
    """diagonal blocks 0 and M: a matter for the exact solve, not for a smoother"""
    out = against_host(ctx, "ex04-reference", 1)
    assert all(h[0] <= 1 for h in out["newton_history"])


def test_ex04_with_the_rows_exchanged_on_three_levels(ctx):
    """KK = [[K, M], [0, K]], the default smoother: V-cycle-preconditioned GMRES converges to the host's direct solve of the top-level system"""
    against_host(ctx, "ex04-exchanged", 3)


@pytest.mark.parametrize("fe,p", [("linear", 1), ("biquadratic", 2)])
def test_convergence_orders_of_both_variables_of_ex04(ctx, fe, p):
    """errors of u and v fall from level to level, and their last observed orders are within 0.15 of p + 1 (L2) and p (H1 semi-norm): the margin of
    tests/test_gpu_convergence_rates.py.  Levels 3, 4 and 5 of the 2 x 2 box: 16, 32 and 64 intervals per wavelength of u_e, chosen before anything was run"""
    runs = [device_run(ctx, "ex04-exchanged", nl, fe=fe, tol=1e-11, max_newton=30, lin_maxit=30) for nl in (3, 4, 5)]
    assert all(r["converged"] for r in runs)
    for k, var in enumerate("uv"):
        l2, h1 = [r["l2_error"][k] for r in runs], [r["h1_error"][k] for r in runs]
        o2, o1 = np.log2(l2[-2] / l2[-1]), np.log2(h1[-2] / h1[-1])
        print("%s, %s: L2 errors %s, H1 errors %s, last orders %.3f and %.3f" % (fe, var, l2, h1, o2, o1))
        assert l2[0] > l2[1] > l2[2] and h1[0] > h1[1] > h1[2]
        assert abs(o2 - (p + 1)) <= 0.15
        assert abs(o1 - p) <= 0.15


@pytest.mark.parametrize("nlevels", [2, 1])
def test_form_s_against_a_host_newton_with_a_direct_solve(ctx, nlevels):
    out = against_host(ctx, "S", nlevels)
    if nlevels == 1:
        assert all(h[0] <= 1 for h in out["newton_history"])
    else:
        coarse = device_run(ctx, "S", 1, tol=1e-11, max_newton=30, lin_maxit=30)
        assert all(out["l2_error"][k] < coarse["l2_error"][k] for k in range(2))          # the manufactured f is the solution's


def test_different_dirichlet_faces_per_variable(ctx):
    """u_0 Dirichlet on all of the boundary; u_1 Dirichlet on one side, with a flux on another and the natural condition on the rest"""
    out = against_host(ctx, "S-faces", 2)
    want, _ = host_newton("S-faces", 2)
    assert np.abs(want[1] - host_newton("S", 2)[0][1]).max() > 1e-3                       # the other boundary conditions give another solution


def test_a_flagged_top_level(ctx):
    """two uniform levels and one refined where x > 0: Newton converges, every hanging dof of every variable is its constraint row applied to the solution
    (1e-12), and the L2 error of every variable is not larger than that of the uniform hierarchy below it"""
    below = device_run(ctx, "S", 2, tol=1e-11, max_newton=30, lin_maxit=30)
    out = device_run(ctx, "S", 3, tol=1e-11, max_newton=30, lin_maxit=30, selective_levels=1, flag="x>0")
    assert out["converged"] and below["converged"]
    hang, ptr, master, w = out["constraints"]
    assert hang.size > 0 and np.array_equal(hang, out["hanging"])
    for k in range(2):
        u = out["solution"][k]
        gap = max(abs(u[h] - w[ptr[j]:ptr[j + 1]] @ u[master[ptr[j]:ptr[j + 1]]]) for j, h in enumerate(hang))
        print("flagged level, variable %d: %d dofs, %d hanging, largest gap %.3e, L2 error %.6e (uniform level below: %.6e)"
              % (k, out["dofs"], hang.size, gap, out["l2_error"][k], below["l2_error"][k]))
        assert gap <= 1e-12
        assert out["l2_error"][k] <= below["l2_error"][k]
