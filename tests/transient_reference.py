"""TEST INFRASTRUCTURE ONLY.  The yardstick of fh_generic_assembler_assemble_transient (include/femus_hip.h) and of femus_amd.transient, composed from
tests/quasilinear_reference.py and not from the kernel.  For u_t - div(a grad u) + c = f, one Newton iteration of one theta-step scaled by dt:
    M      = qr.assemble(form = {a: 0, c: u, c_u: 1})[0]                                  the mass matrix
    K_tr   = M + dt theta K_qr(u; t_new)
    RES_tr = -M (u - uo) + dt theta F_qr(u; t_new) + dt (1 - theta) F_qr(uo; t_old)        t_new = time, t_old = time - dt
A form is a callable t -> dict of callables of the 7-vector v (quasilinear_reference's form with t closed over).  With theta == 1 nothing is evaluated at uo,
with theta == 0 nothing at u.
Also a host time-stepper, Newton with scipy's sparse LU on that system, stopped as femus_amd.transient stops, and the semi-discrete exact solution of the
linear heat equation by a dense generalised eigendecomposition."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import quasilinear_reference as qr
from femus_amd import capi, mixed_mesh

MASS = {"a": lambda v: 0.0, "c": lambda v: v[3], "c_u": lambda v: 1.0}


def mass(kind, ed, xs, fe, order="seventh"):
    return qr.assemble(kind, ed, xs, fe, MASS, None, order=order)[0]


def pieces(kind, ed, xs, fe, form, u, uo, time, dt, order="seventh", old=True, M=None, new=True):
    """(M, K_qr(u; time), F_qr(u; time), F_qr(uo; time - dt)): what every theta combines; without `new` the two at u, without `old` the one at uo are None"""
    M = mass(kind, ed, xs, fe, order) if M is None else M
    Kn, Fn = qr.assemble(kind, ed, xs, fe, form(time), u, order=order) if new else (None, None)
    Fo = qr.assemble(kind, ed, xs, fe, form(time - dt), uo, order=order)[1] if old else None
    return M, Kn, Fn, Fo


def combine(p, u, uo, dt, theta):
    M, Kn, Fn, Fo = p
    K = ((M + dt * theta * Kn) if theta != 0.0 else M.copy()).tocsr()
    F = -(M @ (u - uo))
    if theta != 0.0:
        F = F + dt * theta * Fn
    if theta != 1.0:
        F = F + dt * (1.0 - theta) * Fo
    K.sort_indices()
    return K, F


def assemble(kind, ed, xs, fe, form, u, uo, time, dt, theta, order="seventh", M=None):
    """(K_tr scipy csr, RES_tr)"""
    return combine(pieces(kind, ed, xs, fe, form, u, uo, time, dt, order, old=theta != 1.0, M=M, new=theta != 0.0), u, uo, dt, theta)


def timed(pair, dim):
    """(texts over x,y,z,u,ux,uy,uz,t; t -> callables) of a form of quasilinear_reference with the source f (1 + t), f that of qr.with_source"""
    text, call = qr.with_source(pair, dim)
    f0 = call["f"]
    return dict(text, f="(%s)*(1+t)" % text["f"]), lambda t: dict(call, f=lambda v: f0(v) * (1 + t))


def boundary_nodes(kind, ed, ff, fe, flags):
    """[(flag, node)] of the faces with one of the flags, elements and faces in order (a later face overwrites an earlier one where values are set)"""
    return [(int(ff[e, f]), int(n)) for e, f in zip(*np.nonzero(ff < -1)) if int(ff[e, f]) in flags for n in ed[e, capi.fe_face_nodes(kind[e], fe, f)]]


def edge_flux(kind, ed, xs, ff, fe, flux, order="seventh"):
    """sum over the flux edges of a two-dimensional mesh of int phi_i tau ds; flux: {flag: callable of (x, y, z, t)}"""
    b = np.zeros(int(ed.max()) + 1)
    w, _ = capi.fe_gauss("line", order)
    phi, dphi = capi.fe_tables("line", fe, order)
    for e, f in zip(*np.nonzero(ff < -1)):
        if int(ff[e, f]) not in flux:
            continue
        nodes = ed[e, capi.fe_face_nodes(kind[e], fe, f)]
        x = xs[nodes]
        for g in range(len(w)):
            t = dphi[g, :, 0] @ x
            xg = np.zeros(4)
            xg[:2] = phi[g] @ x
            b[nodes] += phi[g] * flux[int(ff[e, f])](xg) * np.hypot(*t) * w[g]
    return b


class HostStepper:
    """the theta-method with Newton and a direct solve on the system above.  level: (kind, ed, xs, ff, own); form: t -> dict; dirichlet: {flag: callable of
    (x, y, z, t) or None (= 0)}; flux: {flag: callable of (x, y, z, t)}, constant in time (two-dimensional meshes)"""

    def __init__(self, level, fe, form, dirichlet=None, flux=None, theta=1.0, order="seventh"):
        self.kind, self.ed, self.xs, self.ff, own = level
        self.fe, self.form, self.theta, self.order = fe, form, float(theta), order
        self.dim, self.ndof = self.xs.shape[1], own[qr.FAM[fe]]
        self.dirichlet = dict(dirichlet or {})
        self.bnodes = boundary_nodes(self.kind, self.ed, self.ff, fe, set(self.dirichlet))
        self.free = np.ones(self.ndof, bool)
        self.free[[n for _, n in self.bnodes]] = False
        self.b = edge_flux(self.kind, self.ed, self.xs, self.ff, fe, flux, order)[:self.ndof] if flux else np.zeros(self.ndof)
        self.M = mass(self.kind, self.ed, self.xs, fe, order)
        self.u, self.uo, self.time = np.zeros(self.ndof), np.zeros(self.ndof), 0.0

    def set_initial(self, values):
        self.u, self.uo, self.time = np.array(values, dtype=float), np.array(values, dtype=float), 0.0

    def step(self, dt, tol=1e-6, max_newton=15):
        """time += dt, the Dirichlet values at the new time, Newton; returns the number of Newton iterations"""
        self.time += dt
        for flag, n in self.bnodes:
            g = self.dirichlet[flag]
            x4 = np.zeros(4)
            x4[:self.dim], x4[3] = self.xs[n], self.time
            self.u[n] = g(x4) if g is not None else 0.0
        D = sp.diags(self.free.astype(float))
        Fo = None
        for it in range(1, int(max_newton) + 1):
            Kn, Fn = qr.assemble(self.kind, self.ed, self.xs, self.fe, self.form(self.time), self.u, order=self.order)
            if Fo is None and self.theta != 1.0:
                Fo = qr.assemble(self.kind, self.ed, self.xs, self.fe, self.form(self.time - dt), self.uo, order=self.order)[1]
            K, F = combine((self.M, Kn, Fn, Fo), self.u, self.uo, dt, self.theta)
            F = (F + dt * self.b) * self.free
            du = spla.splu(sp.csc_matrix(D @ K @ D + sp.diags(1.0 - self.free))).solve(F)
            self.u = self.u + du
            en, sn = np.linalg.norm(du), np.linalg.norm(self.u)
            if en / (sn + 1e-50) < tol or en < 1e-12 or sn < 1e-12:
                break
        return it

    def copy_solution_to_old(self):
        self.uo = self.u.copy()


# ---- the linear heat equation u_t = lap u of the temporal-order tests ----
HEAT_T = 0.1
HEAT_U0 = "sin(pi*x)*sin(pi*y)"


def heat_level():
    return mixed_mesh.tri_box(4, 4, (0., 0.), (1., 1.))


def heat_system(order="seventh"):
    """(level, free[ndof], M, K, u0): linear family, homogeneous Dirichlet all round, u0 the interpolant of sin(pi x) sin(pi y)"""
    lv = heat_level()
    kind, ed, xs, ff, own = lv
    ndof = own[0]
    free = np.ones(ndof, bool)
    free[[n for _, n in boundary_nodes(kind, ed, ff, "linear", {-2, -3, -4, -5})]] = False
    M = mass(kind, ed, xs, "linear", order)
    K = qr.assemble(kind, ed, xs, "linear", {}, None, order=order)[0]
    u0 = np.sin(np.pi * xs[:ndof, 0]) * np.sin(np.pi * xs[:ndof, 1]) * free
    return lv, free, M, K, u0


def heat_exact(free, M, K, u0, T=HEAT_T):
    """exp(-T M^-1 K) u0 on the free dofs, by the generalised symmetric eigenproblem K q = lambda M q"""
    Mf, Kf = M[free][:, free].toarray(), K[free][:, free].toarray()
    lam, Q = scipy.linalg.eigh(Kf, Mf)                  # Q^T M Q = 1
    u = np.zeros(u0.size)
    u[free] = Q @ (np.exp(-T * lam) * (Q.T @ (Mf @ u0[free])))
    return u


def observed_orders(errors):
    return [float(np.log2(errors[k] / errors[k + 1])) for k in range(len(errors) - 1)]
