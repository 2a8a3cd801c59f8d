"""TEST INFRASTRUCTURE ONLY.  A literal restatement of GetErrorNorm_L2_H1_with_analytical_sol (FE_convergence.hpp:1336-1415) for one variable and one process, in
plain Python loops, and of its variants: the exact function's nodal interpolant (exactSol_from_dofs_gss, :1553-1596) and a second discrete function
(norms_inexact_dofs, :738, :748).  The yardstick of fh_elem_error_norms_host and fh_elem_mesh_error_norms.  Weight, phi and phi_x of every Gauss point come from
amr_flag_reference.elem_type(...).jacobian (the family's own Jacobian: the geometry map over the family's first nc nodes).

Beside the norms it returns, per element, B_i: the same sum with every product and difference replaced by magnitudes -- (sum |phi_i sol_i| + |u|)^2 |weight|
for L2 and (sum |phi_x[i,j] sol_i| + |g[j]|)^2 |weight| for every j -- where u and g[j] of the interpolated modes are themselves taken as sums of magnitudes;
and N, the number of (element, point, term) contributions of each of the two sums."""
import math

import numpy as np

import amr_flag_reference as ref

QP, DOFS, VECTOR = "qp", "dofs", "vector"


def error_norms(kind, ed, xs, fe, sol, mode, exact=None, gradient=None, other=None, order="seventh"):
    """exact(x) -> float and gradient(x) -> [dim floats] take the list x of dim coordinates.  Returns {"l2", "h1", "elem_l2", "elem_h1", "B_l2", "B_h1", "N_l2",
    "N_h1"}"""
    fe = ref.FE[fe] if not isinstance(fe, str) else fe
    dim = xs.shape[1]
    ets = {s: ref.elem_type(s, fe, order) for s in sorted(set(kind.tolist()))}
    nel = kind.shape[0]
    elem_l2, elem_h1, B_l2, B_h1 = [0.] * nel, [0.] * nel, [0.] * nel, [0.] * nel
    seminorm = l2norm = 0.
    N_l2 = N_h1 = 0
    for iel in range(nel):
        et = ets[kind[iel]]
        nDofu = et.nc
        dof = [int(ed[iel, i]) for i in range(nDofu)]
        solu = [float(sol[d]) for d in dof]
        x = [[float(xs[d, j]) for d in dof] for j in range(dim)]
        if mode == DOFS:
            solu_other = [float(exact([x[j][i] for j in range(dim)])) for i in range(nDofu)]
        elif mode == VECTOR:
            solu_other = [float(other[d]) for d in dof]
        for ig in range(et.ng):
            weight, phi, phi_x = et.jacobian(x, ig)
            solu_gss = other_gss = a_solu = a_other = 0.
            gradSolu_gss, gradOther_gss, a_grad, a_gradOther = [0.] * dim, [0.] * dim, [0.] * dim, [0.] * dim
            x_gss = [0.] * dim
            for i in range(nDofu):
                solu_gss += phi[i] * solu[i]
                a_solu += abs(phi[i] * solu[i])
                if mode != QP:
                    other_gss += phi[i] * solu_other[i]
                    a_other += abs(phi[i] * solu_other[i])
                for jdim in range(dim):
                    gradSolu_gss[jdim] += phi_x[i * dim + jdim] * solu[i]
                    a_grad[jdim] += abs(phi_x[i * dim + jdim] * solu[i])
                    x_gss[jdim] += x[jdim][i] * phi[i]
                    if mode != QP:
                        gradOther_gss[jdim] += phi_x[i * dim + jdim] * solu_other[i]
                        a_gradOther[jdim] += abs(phi_x[i * dim + jdim] * solu_other[i])
            if mode == QP:
                exactGradSol = [float(v) for v in gradient([float(v) for v in x_gss])]
                exactSol = float(exact([float(v) for v in x_gss]))
                a_other, a_gradOther = abs(exactSol), [abs(v) for v in exactGradSol]
            else:
                exactGradSol, exactSol = gradOther_gss, other_gss
            for j in range(dim):
                term = ((gradSolu_gss[j] - exactGradSol[j]) * (gradSolu_gss[j] - exactGradSol[j])) * weight
                seminorm += term
                elem_h1[iel] += term
                B_h1[iel] += (a_grad[j] + a_gradOther[j]) ** 2 * abs(weight)
                N_h1 += 1
            term = (exactSol - solu_gss) * (exactSol - solu_gss) * weight
            l2norm += term
            elem_l2[iel] += term
            B_l2[iel] += (a_solu + a_other) ** 2 * abs(weight)
            N_l2 += 1
    return {"l2": math.sqrt(l2norm), "h1": math.sqrt(seminorm), "elem_l2": np.array([float(v) for v in elem_l2]), "elem_h1": np.array([float(v) for v in elem_h1]),
            "B_l2": np.array([float(v) for v in B_l2]), "B_h1": np.array([float(v) for v in B_h1]), "N_l2": N_l2, "N_h1": N_h1}


def magnitude_bounds(kind, ed, xs, fe, sol, mode, exact=None, gradient=None, other=None, order="seventh"):
    """B_i and N of error_norms alone, in array operations (the loop above takes seconds on a few hundred hexahedra): {"B_l2", "B_h1", "N_l2", "N_h1"}.  The same
    magnitudes from the same tables, summed in another order: equal to the loop's within rounding (tests/test_element_error_norms_host.py holds that).  Here
    exact(x[..., dim]) -> [...] and gradient(x[..., dim]) -> [..., dim] take arrays"""
    fe = ref.FE[fe] if not isinstance(fe, str) else fe
    dim, nel = xs.shape[1], kind.shape[0]
    B_l2, B_h1, N = np.zeros(nel), np.zeros(nel), 0
    for s in sorted(set(kind.tolist())):
        et = ref.elem_type(s, fe, order)
        idx = np.nonzero(kind == s)[0]
        dof = ed[idx, :et.nc]
        X, S = xs[dof], np.asarray(sol)[dof]                                  # [ne, nc, dim], [ne, nc]
        J = np.einsum("gna,enb->egab", et.dphi, X)
        weight = np.abs(np.linalg.det(J) * et.w[None, :])                       # [ne, ng]
        gp = np.einsum("gnb,egab->egna", et.dphi, np.linalg.inv(J))             # [ne, ng, nc, dim]
        a_solu = np.einsum("gn,en->eg", np.abs(et.phi), np.abs(S))
        a_grad = np.einsum("egna,en->ega", np.abs(gp), np.abs(S))
        if mode == QP:
            xg = np.einsum("gn,enj->egj", et.phi, X)
            a_other, a_gother = np.abs(exact(xg)), np.abs(gradient(xg))
        else:
            U = exact(X) if mode == DOFS else np.asarray(other)[dof]
            a_other = np.einsum("gn,en->eg", np.abs(et.phi), np.abs(U))
            a_gother = np.einsum("egna,en->ega", np.abs(gp), np.abs(U))
        B_l2[idx] = ((a_solu + a_other) ** 2 * weight).sum(axis=1)
        B_h1[idx] = ((a_grad + a_gother) ** 2 * weight[:, :, None]).sum(axis=(1, 2))
        N += idx.size * et.ng
    return {"B_l2": B_l2, "B_h1": B_h1, "N_l2": N, "N_h1": N * dim}
