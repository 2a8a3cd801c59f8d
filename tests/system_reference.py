"""TEST INFRASTRUCTURE ONLY.  A restatement in numpy of the element loop of fh_generic_assembler_assemble_system (include/femus_hip.h), written from its
formulas: the yardstick of the system kernel and of femus_amd.system.  m variables u_0 .. u_{m-1} of one family, equation k
    -sum_l div(A_kl grad u_l) + c_k = f_k,      A_kl = A_kl(x, U),  c_k = c_k(x, U, grad U)
    RES_(k,i)      = sum_g [ f_k phi_i - sum_l A_kl (grad phi_i . grad u_l) - c_k phi_i ] w
    KK_(k,i),(l,j) = sum_g [ A_kl (grad phi_i . grad phi_j) + (grad phi_i . W_kl) phi_j + phi_i ( C_kl phi_j + D_kl . grad phi_j ) ] w
    W_kl = sum_p (dA_kp/du_l) grad u_p,   C_kl = dc_k/du_l,   D_kl = dc_k/d(grad u_l)
Unknown (k, i) has the number k ndof + i.  The geometry as elem_type::Jacobian (Jac[a][b] = sum_n dphi_n/dxi_a x_n[b], grad phi_n = Jac^-1 dphi_n, w = det w_g).
The Python loops run over Gauss points and pairs of variables; all elements of one shape go through numpy at once (the suite calls this many times).

form: {"m": m, "f": [m], "A": [m][m], "A_u": [m][m][m] (A_u[k][p][l] = dA_kp/du_l), "c": [m], "c_u": [m][m], "c_g": [m][m][<= dim]}, any key but "m" may be
missing and any entry None; an entry is a callable of the state V[ne, 3 + 4 m] = (x, y, z, u_0 .., d_x u_0, d_y u_0, d_z u_0, d_x u_1, ..) of ne Gauss points
(unused entries 0) that returns ne values.  A missing A[k][k] is 1, everything else missing is 0."""
import numpy as np
import scipy.sparse as sp

from femus_amd import mixed_mesh
from quasilinear_reference import FAM, tables


def entry(form, key, *index):
    v = form.get(key)
    for i in index:
        if v is None or i >= len(v):
            return None
        v = v[i]
    return v


def elements(x, U, w, phi, dphi, form):
    """(Ke[ne, m, nc, m, nc], Fe[ne, m, nc]) of ne elements of one shape: x[ne, nc, dim] their nodes, U[m, ne, nc] the state at them"""
    ne, nc, dim = x.shape
    m = form["m"]
    Ke, Fe = np.zeros((ne, m, nc, m, nc)), np.zeros((ne, m, nc))
    for g in range(w.size):
        J = np.einsum("na,enb->eab", dphi[g], x)
        weight = np.linalg.det(J) * w[g]
        grad = np.einsum("eab,nb->ena", np.linalg.inv(J), dphi[g])          # grad[e, n] = Jac^-1 dphi_n
        V = np.zeros((ne, 3 + 4 * m))
        V[:, :dim] = np.einsum("n,end->ed", phi[g], x)
        gu = []
        for k in range(m):
            V[:, 3 + k] = U[k] @ phi[g]
            gu.append(np.einsum("en,ena->ea", U[k], grad))
            V[:, 3 + m + 3 * k:3 + m + 3 * k + dim] = gu[k]
        val = lambda fn: np.broadcast_to(np.asarray(fn(V), dtype=float), (ne,))
        GG = np.einsum("eia,eja->eij", grad, grad)
        PP = np.outer(phi[g], phi[g])
        for k in range(m):
            fk, ck = entry(form, "f", k), entry(form, "c", k)
            if fk:
                Fe[:, k] += (val(fk) * weight)[:, None] * phi[g]
            if ck:
                Fe[:, k] -= (val(ck) * weight)[:, None] * phi[g]
            for l in range(m):
                A = entry(form, "A", k, l)
                Av = val(A) if A else np.ones(ne) if k == l else None
                if Av is not None:
                    Ke[:, k, :, l, :] += (Av * weight)[:, None, None] * GG
                    Fe[:, k] -= (Av * weight)[:, None] * np.einsum("ena,ea->en", grad, gu[l])
                Wkl = None
                for p in range(m):
                    Au = entry(form, "A_u", k, p, l)
                    if Au:
                        Wkl = (0 if Wkl is None else Wkl) + val(Au)[:, None] * gu[p]
                if Wkl is not None:
                    Ke[:, k, :, l, :] += weight[:, None, None] * np.einsum("ena,ea->en", grad, Wkl)[:, :, None] * phi[g][None, None, :]
                C = entry(form, "c_u", k, l)
                if C:
                    Ke[:, k, :, l, :] += (val(C) * weight)[:, None, None] * PP
                D = [entry(form, "c_g", k, l, d) for d in range(dim)]
                if any(D):
                    Dv = np.stack([val(D[d]) if D[d] else np.zeros(ne) for d in range(dim)], axis=1)
                    Ke[:, k, :, l, :] += weight[:, None, None] * phi[g][None, :, None] * np.einsum("ena,ea->en", grad, Dv)[:, None, :]
    return Ke, Fe


def assemble(kind, ed, xs, fe, form, sol=None, order="seventh"):
    """(K scipy csr [m ndof, m ndof], RES [m ndof]).  kind: one shape name per element or one name for all; ed: elem_dof, the family's dofs first in every row;
    sol: [m ndof] or [m, ndof]"""
    kind = np.broadcast_to(np.asarray(kind), ed.shape[:1])
    m = form["m"]
    NC = {s: mixed_mesh.CLASSES[s][FAM[fe]] for s in sorted(set(kind.tolist()))}
    ndof = max(int(ed[kind == s][:, :nc].max()) for s, nc in NC.items()) + 1
    u = np.zeros((m, ndof)) if sol is None else np.asarray(sol, dtype=float).reshape(m, ndof)
    xs = np.asarray(xs, dtype=float)
    rows, cols, vals = [], [], []
    F = np.zeros(m * ndof)
    for s, nc in NC.items():
        dof = ed[kind == s][:, :nc].astype(np.int64)
        Ke, Fe = elements(xs[dof], u[:, dof], *tables(s, fe, order), form)
        sysdof = (np.arange(m)[None, :, None] * ndof + dof[:, None, :]).reshape(dof.shape[0], m * nc)
        rows.append(np.repeat(sysdof, m * nc, axis=1).ravel())
        cols.append(np.tile(sysdof, (1, m * nc)).ravel())
        vals.append(Ke.ravel())
        np.add.at(F, sysdof.ravel(), Fe.ravel())
    K = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m * ndof, m * ndof))
    K.sum_duplicates()
    K.sort_indices()
    return K, F


def lift(fn):
    """a callable of one state vector (tests/quasilinear_reference.py) as a callable of many"""
    return lambda V: np.array([fn(v) for v in V])


def from_scalar(forms):
    """scalar forms of quasilinear_reference side by side: variable k sees (x, y, z, u_k, grad u_k) only"""
    m = len(forms)
    sel = lambda k: [0, 1, 2, 3 + k, 3 + m + 3 * k, 4 + m + 3 * k, 5 + m + 3 * k]
    pick = lambda fn, k: (lambda V: lift(fn)(V[:, sel(k)])) if fn else None
    diag = lambda key: [[pick(forms[k].get(key), k) if k == l else None for l in range(m)] for k in range(m)]
    return {"m": m, "f": [pick(forms[k].get("f"), k) for k in range(m)], "c": [pick(forms[k].get("c"), k) for k in range(m)], "A": diag("a"), "c_u": diag("c_u"),
            "A_u": [[[pick(forms[k].get("a_u"), k) if k == p == l else None for l in range(m)] for p in range(m)] for k in range(m)],
            "c_g": [[[pick(g, k) for g in (forms[k].get("c_g") or [])] if k == l else None for l in range(m)] for k in range(m)]}


def scalar_texts(texts):
    """the same for the device: the texts of scalar forms, u -> u_k, as the arguments of capi.SystemForm"""
    import re
    m = len(texts)
    ren = lambda t, k: None if t is None else re.sub(r"\bu([xyz]?)\b", lambda mo: "u%d%s" % (k, mo.group(1)), t)
    diag = lambda key: [[ren(texts[k].get(key), k) if k == l else None for l in range(m)] for k in range(m)]
    return dict(m=m, f=[ren(texts[k].get("f"), k) for k in range(m)], c=[ren(texts[k].get("c"), k) for k in range(m)], A=diag("a"), c_u=diag("c_u"),
                A_u=[[[ren(texts[k].get("a_u"), k) if k == p == l else None for l in range(m)] for p in range(m)] for k in range(m)],
                c_g=[[[ren(g, k) for g in (texts[k].get("c_g") or [])] if k == l else None for l in range(m)] for k in range(m)])


# ---- the two test forms as texts for the device and callables for the loop above: only + - * / and sqrt, so that host and device agree to rounding ----
def form_s(dim):
    """a viscous Burgers system with cross-diffusion, m = dim:  c_k = sum_d u_d d_d u_k,  A_kk = 1 + u_k^2,  A_01 = 0.5 + x,  A_10 = u0 u1,
    f_k = (k + 1) (1 + x) (1 + y) - k y [- z]"""
    m = dim
    u = lambda k: 3 + k
    gd = lambda k, d: 3 + m + 3 * k + d
    N = lambda: [[None] * m for _ in range(m)]
    xyz = "xyz"
    tA, cA = N(), N()
    tAu, cAu = [N() for _ in range(m)], [N() for _ in range(m)]
    tC, cC, tD, cD = N(), N(), N(), N()
    tf, cf, tc, cc = [], [], [], []
    for k in range(m):
        tA[k][k], cA[k][k] = "1+u%d*u%d" % (k, k), (lambda V, k=k: 1 + V[:, u(k)] ** 2)
        tAu[k][k][k], cAu[k][k][k] = "2*u%d" % k, (lambda V, k=k: 2 * V[:, u(k)])
        tc.append("+".join("u%d*u%d%s" % (d, k, xyz[d]) for d in range(dim)))
        cc.append(lambda V, k=k: sum(V[:, u(d)] * V[:, gd(k, d)] for d in range(dim)))
        tf.append("%d*(1+x)*(1+y)-%d*y%s" % (k + 1, k, "-z" if dim == 3 else ""))
        cf.append(lambda V, k=k: (k + 1) * (1 + V[:, 0]) * (1 + V[:, 1]) - k * V[:, 1] - (V[:, 2] if dim == 3 else 0))
        for l in range(m):
            tC[k][l], cC[k][l] = "u%d%s" % (k, xyz[l]), (lambda V, k=k, l=l: V[:, gd(k, l)])               # dc_k/du_l = d_l u_k
        tD[k][k], cD[k][k] = ["u%d" % d for d in range(dim)], [(lambda V, d=d: V[:, u(d)]) for d in range(dim)]   # dc_k/d(d_d u_k) = u_d
    tA[0][1], cA[0][1] = "0.5+x", (lambda V: 0.5 + V[:, 0])
    tA[1][0], cA[1][0] = "u0*u1", (lambda V: V[:, u(0)] * V[:, u(1)])
    tAu[1][0][0], cAu[1][0][0] = "u1", (lambda V: V[:, u(1)])                                              # dA_10/du_0
    tAu[1][0][1], cAu[1][0][1] = "u0", (lambda V: V[:, u(0)])                                              # dA_10/du_1
    return (dict(m=m, f=tf, A=tA, A_u=tAu, c=tc, c_u=tC, c_g=tD), dict(m=m, f=cf, A=cA, A_u=cAu, c=cc, c_u=cC, c_g=cD))


def form_r(dim=None):
    """four species:  -lap u_k + u_k u_{k+1 mod 4} + sqrt(1 + u_k^2) = (k + 1) (1 + x)"""
    m = 4
    u = lambda k: 3 + k
    N = lambda: [[None] * m for _ in range(m)]
    tC, cC = N(), N()
    tc, cc, tf, cf = [], [], [], []
    for k in range(m):
        n = (k + 1) % m
        tc.append("u%d*u%d+sqrt(1+u%d*u%d)" % (k, n, k, k))
        cc.append(lambda V, k=k, n=n: V[:, u(k)] * V[:, u(n)] + np.sqrt(1 + V[:, u(k)] ** 2))
        tC[k][k], cC[k][k] = "u%d+u%d/sqrt(1+u%d*u%d)" % (n, k, k, k), (lambda V, k=k, n=n: V[:, u(n)] + V[:, u(k)] / np.sqrt(1 + V[:, u(k)] ** 2))
        tC[k][n], cC[k][n] = "u%d" % k, (lambda V, k=k: V[:, u(k)])
        tf.append("%d*(1+x)" % (k + 1))
        cf.append(lambda V, k=k: (k + 1) * (1 + V[:, 0]))
    return dict(m=m, f=tf, c=tc, c_u=tC), dict(m=m, f=cf, c=cc, c_u=cC)
