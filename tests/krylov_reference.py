"""Host restatements (float64) of the outer Krylov solvers of fh_mg_solve (femus_amd/csrc/fh_krylov.hip), iterate by iterate, and the seeded
problems they are compared on.  Imported by tests/test_krylov_reference_host.py (which keeps this module honest on a machine without a GPU) and
by tests/test_gpu_krylov.py (which compares the device with it).

Every solver is stated twice.
  by recurrence: the device's algorithm -- Knoll guess, classical Gram-Schmidt, Givens rotations, the short recurrences of CG, the stop test
                 `rn <= max(rtol * ref, atol) || its >= maxit || rn > dtol * ref` where the solver has it;
  by definition: what the iterate IS -- the minimiser of a residual norm over a Krylov space (dense least squares on a basis orthogonalised by
                 modified Gram-Schmidt applied twice), the Galerkin projection of CG, the closed-form sum of Richardson.
The distance between the two is the reference's own error; the device is allowed MARGIN times that (different summation order of its dot
products of length n, its own hypot).

The operator A is a scipy matrix and the preconditioner M the multigrid cycle of the oracle (fo.vcycle) -- as a dense matrix, applied to unit
vectors, for the small problems, as a function for BIG.  Nothing here comes from the device."""
import functools
import math
import types

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import femus_oracle as fo

RICHARDSON_SCALE = 0.99999          # fixed by the reference for the outer Richardson (fh_krylov_richardson)
MARGIN = 100.0                      # device tolerance = MARGIN * distance between the two reference forms
STEP_FRACTION = 1e-2                # ... and at most this fraction of |x_{k+1} - x_k| / |x_direct| at every compared k
K_LIST = (1, 2, 3, 4, 5, 8, 9, 29, 30, 31, 45, 60)
K_BIG = (1, 2, 3, 4, 5, 6, 7)       # BIG: k <= 7 with restart 3: two full cycles and the first column of a third
RESTARTS = (30, 4, 1)
RESTART_BIG = 3
SOLVERS = ("gmres", "fgmres", "cg", "richardson")      # "gmres" stands for both of its drivers (option gmres_device 1 and 0)
NO_STOP = dict(rtol=0.0, atol=0.0, dtol=1e50)


# ---------------------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------------------
def linear_interpolation(n, nc):
    """n fine points from nc coarse points on the same interval, both ends shared"""
    t = np.arange(n) * ((nc - 1.0) / (n - 1.0))
    j = np.minimum(t.astype(np.int64), nc - 2)
    w = t - j
    P = sp.coo_matrix((np.concatenate([1.0 - w, w]), (np.concatenate([np.arange(n)] * 2), np.concatenate([j, j + 1]))), shape=(n, nc)).tocsr()
    P.eliminate_zeros()
    P.sort_indices()
    return P


def unsymmetric_operator(rng, n, diag0, off_band):
    d = diag0 + rng.uniform(0.0, 0.2, n)
    lo = -1.0 - 0.6 * rng.uniform(0.5, 1.0, n - 1)
    up = -1.0 + 0.6 * rng.uniform(0.5, 1.0, n - 1)
    A = sp.diags([lo, d, up], [-1, 0, 1], format="coo")
    if off_band:
        i = rng.integers(0, n, n // 4)
        j = (i + rng.integers(2, n - 1, n // 4)) % n            # 2 .. n - 2 columns further, cyclically: never on the three bands
        A = A + sp.coo_matrix((rng.uniform(-0.2, 0.2, n // 4), (i, j)), shape=(n, n))
    A = A.tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


class Problem:
    """A x = b with a two-level cycle (level 0: A0 = P^T A P, solved exactly; level 1: Jacobi, omega, npre / npost sweeps) or, without P, the
    exact solve of the one level as the `cycle`"""

    def __init__(self, name, A, P, b, omega=0.6, npre=1, npost=1):
        self.name, self.A, self.P, self.b = name, A.tocsr(), P, np.asarray(b, dtype=np.float64)
        self.n = A.shape[0]
        self.omega, self.npre, self.npost = omega, npre, npost
        H = types.SimpleNamespace()
        if P is None:
            H.A, H.P = [self.A], [None]
        else:
            A0 = (P.T @ self.A @ P).tocsr()
            A0.sort_indices()
            H.A, H.P = [A0, self.A], [None, P]
        H.b = self.b
        self.H = H
        self.dense = self.n <= 2000

    def levels(self):
        """[(A_l, P_l)] coarsest first, as the device hierarchy takes them"""
        return list(zip(self.H.A, self.H.P))

    def cycle(self, v):
        return fo.vcycle(self.H, len(self.H.A) - 1, np.asarray(v, dtype=np.float64), omega=self.omega, npre=self.npre, npost=self.npost)

    @functools.cached_property
    def ops(self):
        """(v -> A v, v -> M v): dense matrices for the small problems (M = the cycle applied to unit vectors), functions for BIG"""
        if not self.dense:
            return (lambda v: self.A @ v), self.cycle
        Ad = self.A.toarray()
        Md = np.column_stack([self.cycle(e) for e in np.eye(self.n)])
        return (lambda v: Ad @ v), (lambda v: Md @ v)

    @functools.cached_property
    def x_direct(self):
        return spla.spsolve(self.A.tocsc(), self.b) if self.n > 1 else self.b / self.A.toarray()[0]


@functools.lru_cache(maxsize=None)
def problem(name):
    if name in ("U130", "U257", "S130", "D130"):
        n = int(name[1:])
        rng = np.random.default_rng(1000 + n)            # S130 and D130 are made from the operator of U130
        A = unsymmetric_operator(rng, n, 2.0, True)
        b = rng.uniform(-1.0, 1.0, n)
        P = linear_interpolation(n, 9 if n == 130 else 17)
        if name[0] == "S":                               # symmetrised and kept diagonally dominant: SPD, symmetric cycle (npre = npost)
            S = (0.5 * (A + A.T)).tolil()
            S.setdiag(0.0)
            S = S.tocsr()
            A = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + rng.uniform(0.05, 0.25, n))).tocsr()
            A.sort_indices()
        if name[0] == "D":                               # a cycle made to diverge: over-relaxed Jacobi, no post-smoothing
            return Problem(name, A, P, b, 2.5, 1, 0)
        return Problem(name, A, P, b)
    if name == "BIG":                                    # more unknowns than 8 * CUs * 256 = 524288 on an MI355X, and no multiple of 256
        n = 600001
        rng = np.random.default_rng(600001)
        return Problem(name, unsymmetric_operator(rng, n, 4.0, False), linear_interpolation(n, 33), rng.uniform(-1.0, 1.0, n))
    if name == "ONE":
        return Problem(name, sp.csr_matrix(np.array([[2.7182818284590451]])), None, np.array([0.3141592653589793]))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------------------
# by recurrence: the device's algorithms
# ---------------------------------------------------------------------------------------------------------------------------------
class Result(types.SimpleNamespace):
    """x, rn (what the solver reports), its, ref (the norm the tolerances are relative to), hist (rn after 0, 1, ... iterations)"""


def _stop(rn, ref, its, rtol, atol, dtol, maxit):
    return rn <= max(rtol * ref, atol) or its >= maxit or rn > dtol * ref


def gmres_recurrence(pb, restart, maxit, flexible=False, rtol=0.0, atol=0.0, dtol=1e50, knoll=True, snapshots=None):
    """fh_krylov_gmres_device / fh_krylov_gmres_host: GMRES(restart), classical Gram-Schmidt, Knoll guess x0 = M b.  Left-preconditioned:
    reference norm ||M b||, rn = the estimate |g[k + 1]| of ||M (b - A x)||.  Flexible: right preconditioning with the z_k = M v_k kept,
    reference norm ||b||, rn = the estimate of ||b - A x||.  At the start of a cycle rn is the norm itself.
    snapshots: a dict that receives {its: (x, rn)} -- what the same call with maxit = its returns, by the same operations in the same order."""
    Aop, Mop = pb.ops
    b = pb.b
    m = restart
    x = Mop(b) if knoll else np.zeros_like(b)
    ref = np.linalg.norm(b) if flexible else np.linalg.norm(Mop(b))
    its, hist, done = 0, [], False

    def update(x, Hm, g, kused, U):                       # x + U y, y from the back substitution
        y = sla.solve_triangular(Hm[:kused, :kused], g[:kused])
        for yj, u in zip(y, U):
            x = x + yj * u
        return x

    while not done:
        v0 = b - Aop(x) if flexible else Mop(b - Aop(x))
        beta = rn = np.linalg.norm(v0)
        if not hist:
            hist.append(beta)
        if snapshots is not None and its == 0:
            snapshots[0] = (x, beta)
        if _stop(beta, ref, its, rtol, atol, dtol, maxit):
            break
        V, Z = [v0 / beta], []
        Hm = np.zeros((m + 1, m))
        g = np.zeros(m + 1)
        g[0] = beta
        cs, sn = np.zeros(m), np.zeros(m)
        kused = 0
        for k in range(m):
            if flexible:
                Z.append(Mop(V[k]))
                w = Aop(Z[k])
            else:
                w = Mop(Aop(V[k]))
            h = np.array([v @ w for v in V])              # classical Gram-Schmidt: all projections from the same w
            for hj, v in zip(h, V):
                w = w - hj * v
            wn = np.linalg.norm(w)
            V.append(w / wn if wn != 0.0 else np.zeros_like(w))
            Hm[:k + 1, k] = h
            Hm[k + 1, k] = wn
            for j in range(k):
                a, bb = Hm[j, k], Hm[j + 1, k]
                Hm[j, k] = cs[j] * a + sn[j] * bb
                Hm[j + 1, k] = -sn[j] * a + cs[j] * bb
            a, bb = Hm[k, k], Hm[k + 1, k]
            d = math.hypot(a, bb)
            its += 1
            kused = k + 1
            if d == 0.0:                                  # column k vanished entirely (fh_hessenberg.h)
                cs[k], sn[k], Hm[k, k], g[k + 1], rn, done = 1.0, 0.0, 1.0, 0.0, 0.0, True
            else:
                cs[k], sn[k] = a / d, bb / d
                Hm[k, k], Hm[k + 1, k] = d, 0.0
                g[k + 1] = -sn[k] * g[k]
                g[k] = cs[k] * g[k]
                rn = abs(g[k + 1])
                done = _stop(rn, ref, its, rtol, atol, dtol, maxit) or wn == 0.0
            hist.append(rn)
            if snapshots is not None:
                snapshots[its] = (update(x, Hm, g, kused, Z if flexible else V), rn)
            if done:
                break
        x = update(x, Hm, g, kused, Z if flexible else V)
    return Result(x=x, rn=rn, its=its, ref=ref, hist=hist)


def cg_recurrence(pb, maxit, rtol=0.0, atol=0.0, dtol=1e50, snapshots=None):
    """fh_krylov_cg: preconditioned CG from x0 = 0, rn = ||r|| of the recurrence against ||b||"""
    Aop, Mop = pb.ops
    b = pb.b
    x = np.zeros_like(b)
    r = b.copy()
    bn = rn = np.linalg.norm(b)
    z = Mop(r)
    p = z.copy()
    rz = r @ z
    its, hist = 0, [rn]
    if snapshots is not None:
        snapshots[0] = (x, rn)
    while rn > max(rtol * bn, atol) and its < maxit and rn <= dtol * bn:
        Ap = Aop(p)
        alpha = rz / (p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        rn = np.linalg.norm(r)
        its += 1
        hist.append(rn)
        if snapshots is not None:
            snapshots[its] = (x, rn)
        z = Mop(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return Result(x=x, rn=rn, its=its, ref=bn, hist=hist)


def richardson_recurrence(pb, maxit, rtol=0.0, atol=0.0, dtol=1e50, scale=RICHARDSON_SCALE, snapshots=None):
    """fh_krylov_richardson: x <- x + 0.99999 M (b - A x) from x0 = 0, rn = ||b - A x|| against ||b||"""
    Aop, Mop = pb.ops
    b = pb.b
    x = np.zeros_like(b)
    bn = np.linalg.norm(b)
    its, hist = 0, []
    while True:
        r = b - Aop(x)
        rn = np.linalg.norm(r)
        hist.append(rn)
        if snapshots is not None:
            snapshots[its] = (x, rn)
        if _stop(rn, bn, its, rtol, atol, dtol, maxit):
            break
        x = x + scale * Mop(r)
        its += 1
    return Result(x=x, rn=rn, its=its, ref=bn, hist=hist)


def solve_recurrence(pb, solver, restart, maxit, **tol):
    if solver == "gmres":
        return gmres_recurrence(pb, restart, maxit, False, **tol)
    if solver == "fgmres":
        return gmres_recurrence(pb, restart, maxit, True, **tol)
    if solver == "cg":
        return cg_recurrence(pb, maxit, **tol)
    if solver == "richardson":
        return richardson_recurrence(pb, maxit, **tol)
    raise KeyError(solver)


# ---------------------------------------------------------------------------------------------------------------------------------
# by definition: no Givens rotations, no short recurrences
# ---------------------------------------------------------------------------------------------------------------------------------
def krylov_basis(B, v, k):
    """Q, an orthonormal basis of K_k(B, v), n x k: modified Gram-Schmidt applied twice; and B Q"""
    Q, BQ = [], []
    w = v
    for _ in range(k):
        for _twice in range(2):
            for q in Q:
                w = w - (q @ w) * q
        Q.append(w / np.linalg.norm(w))
        w = B(Q[-1])
        BQ.append(w)
    return np.column_stack(Q), np.column_stack(BQ)


def gmres_definition(pb, restart, k, flexible=False):
    """x_k of GMRES(restart) from the Knoll guess: per restart cycle of j columns, left: x0 + argmin ||M (b - A x)|| over K_j(MA, M r0);
    flexible: x0 + M Q y with y = argmin ||b - A (x0 + M Q y)||, Q a basis of K_j(AM, r0).  rn = the minimum (the norm itself for k = 0)."""
    Aop, Mop = pb.ops
    b = pb.b
    B = (lambda v: Aop(Mop(v))) if flexible else (lambda v: Mop(Aop(v)))
    x = Mop(b)
    ref = np.linalg.norm(b) if flexible else np.linalg.norm(x)
    left = k
    while True:
        r0 = b - Aop(x) if flexible else Mop(b - Aop(x))
        rn = np.linalg.norm(r0)
        j = min(restart, left)
        if j == 0 or rn == 0.0:
            break
        Q, BQ = krylov_basis(B, r0, j)
        y = np.linalg.lstsq(BQ, r0, rcond=None)[0]
        dx = Q @ y
        x = x + (Mop(dx) if flexible else dx)
        rn = np.linalg.norm(r0 - BQ @ y)
        left -= j
        if left == 0:
            break
    return Result(x=x, rn=rn, its=k, ref=ref)


def cg_definition(pb, k):
    """x_k = Q (Q^T A Q)^-1 Q^T b, Q an orthonormal basis of K_k(MA, M b): the Galerkin projection CG computes; rn = ||b - A x_k||"""
    Aop, Mop = pb.ops
    b = pb.b
    x = np.zeros_like(b)
    if k > 0:
        Q, _ = krylov_basis(lambda v: Mop(Aop(v)), Mop(b), k)
        AQ = np.column_stack([Aop(Q[:, i]) for i in range(k)])
        x = Q @ np.linalg.solve(Q.T @ AQ, Q.T @ b)
    return Result(x=x, rn=np.linalg.norm(b - Aop(x)), its=k, ref=np.linalg.norm(b))


def richardson_definition(pb, k, scale=RICHARDSON_SCALE):
    """x_k = sum_{j < k} (I - s M A)^j s M b; rn = ||b - A x_k||"""
    Aop, Mop = pb.ops
    b = pb.b
    x = np.zeros_like(b)
    term = scale * Mop(b)
    for _ in range(k):
        x = x + term
        term = term - scale * Mop(Aop(term))
    return Result(x=x, rn=np.linalg.norm(b - Aop(x)), its=k, ref=np.linalg.norm(b))


def solve_definition(pb, solver, restart, k):
    if solver == "gmres":
        return gmres_definition(pb, restart, k, False)
    if solver == "fgmres":
        return gmres_definition(pb, restart, k, True)
    if solver == "cg":
        return cg_definition(pb, k)
    if solver == "richardson":
        return richardson_definition(pb, k)
    raise KeyError(solver)


# ---------------------------------------------------------------------------------------------------------------------------------
# the iterate cases: which k are compared, at what tolerance
# ---------------------------------------------------------------------------------------------------------------------------------
def iterate_cases():
    """(problem, solver, restart) of tests (a) and (d); restart 0 where the solver has none"""
    out = []
    for name in ("U130", "U257"):
        out += [(name, s, m) for s in ("gmres", "fgmres") for m in RESTARTS] + [(name, "richardson", 0)]
    out.append(("S130", "cg", 0))
    out += [("BIG", "gmres", RESTART_BIG), ("BIG", "fgmres", RESTART_BIG), ("BIG", "richardson", 0)]
    return out


@functools.lru_cache(maxsize=None)
def iterate_case(name, solver, restart):
    """The reference of one case: for every listed k both forms of x_k, their distance |x_k - x_k'| / |x_direct| and the step
    |x_{k+1} - x_k| / |x_direct| of the recurrence.  tol = MARGIN * the largest distance over the compared k; a k is compared when
    tol <= STEP_FRACTION * step there (dropping a k can only lower tol, so the loop below ends)."""
    pb = problem(name)
    listed = K_BIG if name == "BIG" else K_LIST
    xdn = np.linalg.norm(pb.x_direct)
    snap = {}
    ref = solve_recurrence(pb, solver, restart, max(listed) + 1, snapshots=snap, **NO_STOP).ref
    rec = {k: Result(x=snap[k][0], rn=snap[k][1], its=k, ref=ref) for k in sorted(set(listed) | {k + 1 for k in listed})}
    dfn = {k: solve_definition(pb, solver, restart, k) for k in listed}
    dist = {k: np.linalg.norm(rec[k].x - dfn[k].x) / xdn for k in listed}
    step = {k: np.linalg.norm(rec[k + 1].x - rec[k].x) / xdn for k in listed}
    ks = list(listed)
    while True:
        tol = MARGIN * max(dist[k] for k in ks)
        keep = [k for k in ks if tol <= STEP_FRACTION * step[k]]
        if keep == ks or not keep:
            break
        ks = keep
    return types.SimpleNamespace(problem=pb, solver=solver, restart=restart, listed=listed, ks=tuple(ks), dropped=tuple(k for k in listed if k not in ks),
                                 tol=tol, dist=dist, step=step, rec=rec, dfn=dfn, xdn=xdn, max_dist=max(dist[k] for k in ks))


RN_RTOL = 1e-8
RN_FLOOR = 1e-8


def rn_comparable(res):
    """rn is compared (relative RN_RTOL) only where the reference value is above RN_FLOOR * ref: below, an estimate and a true norm part ways"""
    return res.rn > RN_FLOOR * res.ref


# ---------------------------------------------------------------------------------------------------------------------------------
# the stopping cases
# ---------------------------------------------------------------------------------------------------------------------------------
def stop_cases():
    """(solver, restart) of test (b) on U130 (CG: S130)"""
    return [("gmres", 30), ("gmres", 4), ("fgmres", 30), ("fgmres", 4), ("cg", 0), ("richardson", 0)]


def stop_problem(solver):
    return problem("S130" if solver == "cg" else "U130")


@functools.lru_cache(maxsize=None)
def stop_case(solver, restart):
    """A threshold midway between two consecutive reference residuals hist[i] > hist[i + 1] that differ by at least a factor 1.5, hist[i] the
    smallest so far: a solver that tests `rn <= threshold` stops after exactly i + 1 iterations.  Returns the threshold, the reference norm
    and i + 1."""
    pb = stop_problem(solver)
    run = solve_recurrence(pb, solver, restart, 60, **NO_STOP)
    hist, ref = run.hist, run.ref
    first = restart if 0 < restart < 30 else 2           # a short restart: past the first cycle where the history has such a gap there
    for i in list(range(first, len(hist) - 1)) + list(range(first)):
        if hist[i] == min(hist[:i + 1]) and hist[i] >= 1.5 * hist[i + 1]:
            return types.SimpleNamespace(problem=pb, threshold=0.5 * (hist[i] + hist[i + 1]), ref=ref, index=i + 1, hist=hist)
    raise AssertionError("no factor-1.5 gap in the residual history of %s(%d)" % (solver, restart))


@functools.lru_cache(maxsize=None)
def divergence_case(solver):
    """D130, the cycle that diverges.  Richardson: dtol midway in log scale between two consecutive growing residuals hist[i] < hist[i + 1]
    (each the largest so far): `rn > dtol * ref` first holds after i + 1 iterations.  GMRES and FGMRES: inside a cycle the residual norm
    cannot grow, but the norm at the first restart -- ||M (b - A M b)|| against ||M b||, ||b - A M b|| against ||b|| -- has grown over the
    reference norm; dtol midway in log scale between 1 and their ratio stops the solver there, after 0 iterations, with the Knoll guess."""
    pb = problem("D130")
    if solver in ("gmres", "fgmres"):
        r0 = gmres_recurrence(pb, 30, 0, solver == "fgmres")
        assert r0.rn > 1.2 * r0.ref
        return types.SimpleNamespace(problem=pb, dtol=math.sqrt(r0.rn / r0.ref), ref=r0.ref, index=0, hist=[r0.ref, r0.rn])
    hist = richardson_recurrence(pb, 12).hist
    ref = hist[0]
    for i in range(2, len(hist) - 1):
        if hist[i] == max(hist[:i + 1]) and hist[i + 1] >= 1.5 * hist[i]:
            return types.SimpleNamespace(problem=pb, dtol=math.sqrt(hist[i] * hist[i + 1]) / ref, ref=ref, index=i + 1, hist=hist)
    raise AssertionError("the diverging cycle does not diverge")
