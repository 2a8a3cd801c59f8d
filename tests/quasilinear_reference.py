"""TEST INFRASTRUCTURE ONLY.  A literal restatement of the element loop of fh_generic_assembler_assemble_form (include/femus_hip.h) in numpy: the yardstick of
the quasilinear kernel and of femus_amd.quasilinear.  For -div(a grad u) + c = f with a = a(x, u), c = c(x, u, grad u):
    RES_i = sum_g [ f phi_i - a (grad phi_i . grad u) - c phi_i ] w
    KK_ij = sum_g [ a (grad phi_i . grad phi_j) + a_u phi_j (grad phi_i . grad u) + phi_i ( c_u phi_j + c_g . grad phi_j ) ] w
Python loops over elements and Gauss points, the sums over an element's nodes as numpy products (the suite calls this many times); the geometry as elem_type::Jacobian (Jac[a][b] = sum_n dphi_n/dxi_a x_n[b], grad phi_n = Jac^-1 dphi_n,
w = det w_g).  Gauss weights and the tables phi, dphi come from capi.fe_gauss / capi.fe_tables (host code, no device).  The coefficients are Python callables
of the 7-vector v = (x, y, z, u, ux, uy, uz) at the Gauss point (unused entries 0); a missing one is a = 1, everything else 0.

form: a dict with any of the keys "f", "a", "a_u", "c", "c_u" (callables) and "c_g" (a list of at most dim callables)."""
import numpy as np
import scipy.sparse as sp

from femus_amd import capi, mixed_mesh

FAM = {"linear": 0, "serendipity": 1, "biquadratic": 2}


def tables(shape, fe, order):
    w, _ = capi.fe_gauss(shape, order)
    phi, dphi = capi.fe_tables(shape, fe, order)
    return np.asarray(w), phi, dphi


def element(x, u, w, phi, dphi, form):
    """(Ke[nc, nc], Fe[nc]) of one element: x[nc, dim] its nodes, u[nc] the state at them"""
    nc, dim = x.shape
    f, a, a_u, c, c_u = (form.get(k) for k in ("f", "a", "a_u", "c", "c_u"))
    c_g = list(form.get("c_g") or [])
    assert len(c_g) <= dim
    Ke, Fe = np.zeros((nc, nc)), np.zeros(nc)
    for g in range(w.size):
        J = dphi[g].T @ x                              # the sums over the nodes n are numpy products: [dim, nc] [nc, dim]
        weight = np.linalg.det(J) * w[g]
        grad = dphi[g] @ np.linalg.inv(J).T            # grad[n] = Jac^-1 dphi_n
        v = np.zeros(7)
        v[:dim] = phi[g] @ x
        v[3] = phi[g] @ u
        v[4:4 + dim] = u @ grad
        gu = v[4:4 + dim].copy()
        fv = f(v) if f else 0.0
        av = a(v) if a else 1.0
        auv = a_u(v) if a_u else 0.0
        cv = c(v) if c else 0.0
        cuv = c_u(v) if c_u else 0.0
        cgv = np.array([c_g[d](v) if d < len(c_g) and c_g[d] else 0.0 for d in range(dim)])
        S = grad @ gu                                  # S_n = grad phi_n . grad u
        T = cuv * phi[g] + grad @ cgv                  # T_n = c_u phi_n + c_g . grad phi_n
        Ke += (av * (grad @ grad.T) + auv * np.outer(S, phi[g]) + np.outer(phi[g], T)) * weight
        Fe += (fv * phi[g] - av * S - cv * phi[g]) * weight
    return Ke, Fe


def assemble(kind, ed, xs, fe, form, sol=None, order="seventh"):
    """(K scipy csr [ndof, ndof], RES [ndof]).  kind: one shape name per element or one name for all; ed: elem_dof, the family's dofs first in every row"""
    kind = np.broadcast_to(np.asarray(kind), ed.shape[:1])
    T = {s: tables(s, fe, order) for s in sorted(set(kind.tolist()))}
    NC = {s: mixed_mesh.CLASSES[s][FAM[fe]] for s in T}
    ndof = max(int(ed[e, :NC[kind[e]]].max()) for e in range(ed.shape[0])) + 1
    u = np.zeros(ndof) if sol is None else np.asarray(sol, dtype=float)
    rows, cols, vals = [], [], []
    F = np.zeros(ndof)
    for e in range(ed.shape[0]):
        s = kind[e]
        nc = NC[s]
        dof = ed[e, :nc].astype(np.int64)
        Ke, Fe = element(np.asarray(xs, dtype=float)[dof], u[dof], *T[s], form)
        rows.append(np.repeat(dof, nc))
        cols.append(np.tile(dof, nc))
        vals.append(Ke.ravel())
        np.add.at(F, dof, Fe)
    K = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(ndof, ndof))
    K.sum_duplicates()
    K.sort_indices()
    return K, F


# ---- the two test forms (tests/test_gpu_quasilinear.py, tests/test_quasilinear_reference_host.py) as texts for the device and callables for the loop above ----
def form_a(dim):
    """ex03: -lap u + u sum_d du/dx_d = f"""
    g = ["ux", "uy", "uz"][:dim]
    text = dict(c="u*(%s)" % "+".join(g), c_u="+".join(g), c_g=["u"] * dim)
    call = dict(c=lambda v: v[3] * v[4:4 + dim].sum(), c_u=lambda v: v[4:4 + dim].sum(), c_g=[lambda v: v[3]] * dim)
    return text, call


def form_b(dim):
    """ex03b plus a reaction: -div((1 + u^2) grad u) + sqrt(1 + u^2) = f"""
    text = dict(a="1+u*u", a_u="2*u", c="sqrt(1+u*u)", c_u="u/sqrt(1+u*u)")
    call = dict(a=lambda v: 1 + v[3] * v[3], a_u=lambda v: 2 * v[3], c=lambda v: np.sqrt(1 + v[3] * v[3]), c_u=lambda v: v[3] / np.sqrt(1 + v[3] * v[3]))
    return text, call


def with_source(pair, dim):
    """the form with the source of tests/test_gpu_generic_assembler.py: f = exp(x) (1 + y) [- z]"""
    text, call = dict(pair[0]), dict(pair[1])
    text["f"] = "exp(x)*(1+y)" if dim == 2 else "exp(x)*(1+y)-z"
    call["f"] = (lambda v: np.exp(v[0]) * (1 + v[1])) if dim == 2 else (lambda v: np.exp(v[0]) * (1 + v[1]) - v[2])
    return text, call
