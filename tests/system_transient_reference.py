"""TEST INFRASTRUCTURE ONLY.  The yardstick of fh_generic_assembler_assemble_system_transient (include/femus_hip.h) and of
femus_amd.transient.TransientSystemElements, composed from tests/system_reference.py (assemble) and tests/transient_reference.py (mass) and not from the kernel.
For m variables, equation k:  sum_l M_kl d_t u_l - sum_l div(A_kl grad u_l) + c_k = f_k;  one Newton iteration of one theta-step scaled by dt:
    K_tr   = kron(M, Mass) + dt diag(th_k) K_sr(U; time)
    RES_tr = -kron(M, Mass) (U - Uo) + dt th_k F_sr(U; time) + dt (1 - th_k) F_sr(Uo; time - dt)
row-block-wise (row block k holds the unknowns k ndof .. (k + 1) ndof - 1, and block (k, l) the columns l ndof + j: the numbering of Mat.block_system).
th_k = theta, or 1 for an algebraic equation (row k of M entirely zero).  A form is a callable t -> dict of callables of the states V[ne, 3 + 4 m]
(system_reference's form with t closed over).  Nothing is evaluated at U where every th_k is 0, nothing at Uo where every th_k is 1, and a row block takes
nothing from a state its th_k leaves out.
Also a host theta-stepper, Newton with scipy's sparse LU on that system, stopped as femus_amd.transient stops; and the timed forms S (m = dim) and R (m = 4) of
system_reference.py, their sources times 1 + t: only + - * / and sqrt, so that host and device agree to rounding."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import quasilinear_reference as qr
import system_reference as sr
import transient_reference as tr


def thetas(M, theta):
    """th_k of every equation"""
    M = np.asarray(M, dtype=float)
    return np.array([float(theta) if np.any(M[k] != 0.0) else 1.0 for k in range(M.shape[0])])


def mass_matrix(m, M=None):
    M = np.eye(m) if M is None else np.asarray(M, dtype=float)
    assert M.shape == (m, m)
    return M


def combine(Mass, M, th, Kn, Fn, Fo, u, uo, dt):
    """(K_tr csr, RES_tr) from the pieces; Kn, Fn may be None where every th_k is 0, Fo where every th_k is 1"""
    m, ndof = M.shape[0], Mass.shape[0]
    KM = sp.kron(sp.csr_matrix(M), Mass, format="csr")
    K = KM
    F = -(KM @ (np.asarray(u).ravel() - np.asarray(uo).ravel()))
    rows = lambda k: slice(k * ndof, (k + 1) * ndof)
    if np.any(th != 0.0):
        K = K + sp.diags(np.repeat(dt * th, ndof)) @ Kn
    for k in range(m):
        if th[k] != 0.0:
            F[rows(k)] += dt * th[k] * Fn[rows(k)]
        if th[k] != 1.0:
            F[rows(k)] += dt * (1.0 - th[k]) * Fo[rows(k)]
    K = sp.csr_matrix(K)
    K.sum_duplicates()
    K.sort_indices()
    return K, F


def assemble(kind, ed, xs, fe, form, u, uo, time, dt, theta, M=None, order="seventh", Mass=None):
    """(K_tr scipy csr [m ndof, m ndof], RES_tr [m ndof]).  form: t -> dict (system_reference's form); u, uo: [m ndof] or [m, ndof]; M: [m, m] or None (identity)"""
    m = form(time)["m"]
    M = mass_matrix(m, M)
    th = thetas(M, theta)
    Mass = tr.mass(kind, ed, xs, fe, order) if Mass is None else Mass
    Kn, Fn = sr.assemble(kind, ed, xs, fe, form(time), u, order=order) if np.any(th != 0.0) else (None, None)
    Fo = sr.assemble(kind, ed, xs, fe, form(time - dt), uo, order=order)[1] if np.any(th != 1.0) else None
    return combine(Mass, M, th, Kn, Fn, Fo, u, uo, dt)


def timed(pair):
    """(texts over SystemForm.variables(m) + ",t"; t -> callables) of a pair of system_reference with every source f_k times (1 + t)"""
    text, call = pair
    f0 = list(call["f"])
    return (dict(text, f=["(%s)*(1+t)" % f for f in text["f"]]),
            lambda t: dict(call, f=[(lambda V, fk=fk: fk(V) * (1 + t)) for fk in f0]))


def form_s(dim):
    return timed(sr.form_s(dim))


def form_r(dim=None):
    return timed(sr.form_r(dim))


def untimed(call):
    """a form of system_reference (no t in it) as t -> dict"""
    return lambda t: call


class HostStepper:
    """the theta-method with Newton and a direct solve on the system above.  level: (kind, ed, xs, ff, own); form: t -> dict; dirichlet, flux: lists of m dicts
    {flag: callable of (x, y, z, t) or None (= 0)} and {flag: callable of (x, y, z, t)}, the flux constant in time (two-dimensional meshes)"""

    def __init__(self, level, fe, form, dirichlet=None, flux=None, M=None, theta=1.0, order="seventh"):
        self.kind, self.ed, self.xs, self.ff, own = level
        self.fe, self.form, self.theta, self.order = fe, form, float(theta), order
        self.dim, self.ndof = self.xs.shape[1], own[qr.FAM[fe]]
        m = self.m = form(0.0)["m"]
        n = self.ndof
        self.M = mass_matrix(m, M)
        self.th = thetas(self.M, theta)
        self.dirichlet = [dict(d or {}) for d in (dirichlet or [None] * m)]
        flux = [dict(f or {}) for f in (flux or [None] * m)]
        self.bnodes = [tr.boundary_nodes(self.kind, self.ed, self.ff, fe, set(self.dirichlet[k])) for k in range(m)]
        self.free = np.ones(m * n, bool)
        for k in range(m):
            self.free[[k * n + node for _, node in self.bnodes[k]]] = False
        self.b = np.concatenate([tr.edge_flux(self.kind, self.ed, self.xs, self.ff, fe, flux[k], order)[:n] if flux[k] else np.zeros(n) for k in range(m)])
        self.Mass = tr.mass(self.kind, self.ed, self.xs, fe, order)
        self.u, self.uo, self.time = np.zeros(m * n), np.zeros(m * n), 0.0

    def set_initial(self, values):
        self.u = np.array(values, dtype=float).ravel()
        self.uo, self.time = self.u.copy(), 0.0

    def step(self, dt, tol=1e-6, max_newton=15):
        """time += dt, the Dirichlet values of every variable at the new time, Newton; returns the number of Newton iterations"""
        self.time += dt
        n = self.ndof
        for k in range(self.m):
            for flag, node in self.bnodes[k]:
                g = self.dirichlet[k][flag]
                x4 = np.zeros(4)
                x4[:self.dim], x4[3] = self.xs[node], self.time
                self.u[k * n + node] = g(x4) if g is not None else 0.0
        D = sp.diags(self.free.astype(float))
        args = (self.kind, self.ed, self.xs, self.fe)
        Fo = None
        for it in range(1, int(max_newton) + 1):
            Kn, Fn = sr.assemble(*args, self.form(self.time), self.u, order=self.order) if np.any(self.th != 0.0) else (None, None)
            if Fo is None and np.any(self.th != 1.0):
                Fo = sr.assemble(*args, self.form(self.time - dt), self.uo, order=self.order)[1]
            K, F = combine(self.Mass, self.M, self.th, Kn, Fn, Fo, self.u, self.uo, dt)
            F = (F + dt * self.b) * self.free
            du = spla.splu(sp.csc_matrix(D @ K @ D + sp.diags(1.0 - self.free))).solve(F)
            self.u = self.u + du
            en, sn = np.linalg.norm(du), np.linalg.norm(self.u)
            if en / (sn + 1e-50) < tol or en < 1e-12 or sn < 1e-12:
                break
        return it

    def copy_solution_to_old(self):
        self.uo = self.u.copy()

    def solution(self):
        return self.u.reshape(self.m, self.ndof)
