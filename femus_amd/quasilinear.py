"""Newton's method for a quasilinear scalar equation  -div(a(x, u) grad u) + c(x, u, grad u) = f  on resident element meshes of any shape: the driver of
NonLinearImplicitSystem::MGsolve (src/08_equations/00_stationary/NonLinearImplicitSystem.cpp:157-361) for the problems of
applications/000_tutorial/ex03_poisson_plus_nonlin_advection and ex03b_div_grad_nonlinear_diffusivity, on triangles, tetrahedra, prisms and mixed meshes.

The levels, transfers, pattern, plan and boundary data are made where the levels live, as app_poisson.Poisson001.run_elements(mesh_data="device") makes them
(capi.ElementMesh.refine / prolongator / boundary_dofs / matrix / boundary_owners / boundary_faces, capi.GenericAssembler.from_mesh); Jacobian and residual of
every Newton step come from capi.GenericAssembler.assemble_form (femus_amd/csrc/fh_quasilinear.hip) at the current state."""
import numpy as np

from . import capi

FAMILY = {"linear": 0, "serendipity": 1, "biquadratic": 2}


class ResidentHierarchy:
    """What the Newton drivers on resident element meshes share (QuasilinearElements here, transient.TransientQuasilinearElements): the levels, transfers,
    boundary lists, P_amr wiring of flagged levels, pattern, plan, flux faces, work vectors and the Multigrid object, made once and kept until destroy(); and one
    nonlinear iteration on them.  dirichlet: {face flag: Expr over "x,y,z,t" or None (= 0)}; flux: {face flag: Expr}.
    nvars > 1 (system.SystemElements): that many variables of the one family stacked, unknown (k, i) = k ndof + i; dirichlet and flux are lists of nvars such
    dicts; the boundary rows of a level are k ndof_l + the Dirichlet dofs of variable k and the hanging dofs, for every k; the transfers and P_amr are
    Mat.block_diagonal of the scalar ones (PP after its P_amr product); K is Mat.block_system of the scalar pattern S, on which the plan is made; the flux faces
    of every variable are integrated once into one vector of the system's size."""

    def __init__(self, ctx, level0, fe, nlevels, dirichlet, flux, order, selective_levels=0, flag=None, amr_mode="reference", nvars=1):
        nv = self.nvars = int(nvars)
        nl, fam = int(nlevels), FAMILY[fe]
        selective_levels = int(selective_levels)
        if selective_levels and (not 0 < selective_levels < nl or flag is None):
            raise ValueError("selective_levels must be 0 .. nlevels - 1 = %d and come with a flag expression over x, y, z, level" % (nl - 1))
        if amr_mode not in ("reference", "coarsest"):
            raise ValueError("amr_mode must be \"reference\" or \"coarsest\", not %r" % (amr_mode,))
        self.ctx, self.fe, self.fam, self.nl, self.order, self.selective_levels = ctx, fe, fam, nl, order, selective_levels
        self.dirichlet, self.flux = dirichlet, flux
        top, n_uniform = nl - 1, nl - selective_levels
        dirichlets, fluxes = ([dirichlet], [flux]) if nv == 1 else (list(dirichlet), list(flux))
        d_flags = [sorted(int(f) for f in d) for d in dirichlets]
        owned = self.owned = []                                       # every device object made here but the levels
        resident = self.resident = [capi.ElementMesh.from_arrays(ctx, *level0)]
        try:
            for l in range(1, nl):
                if l < n_uniform:
                    resident.append(resident[-1].refine())
                else:
                    resident[-1].flag(flag)
                    resident.append(resident[-1].refine("resident"))
            m = self.top = resident[top]
            hanging, P_amr, self.constraints = [np.zeros(0, np.int32)] * nl, [None] * nl, None
            for l, lv in enumerate(resident):
                if not lv.homogeneous:
                    c = lv.amr_constraints(fam, amr_mode)
                    hanging[l], P_amr[l] = c[0], lv.amr_prolongator(fam, amr_mode)
                    owned.append(P_amr[l])
                    if l == top:
                        self.constraints = c
            self.hanging = hanging
            bdc, P = self.bdc, self.P = [], [None]
            for l, lv in enumerate(resident):
                bdc.append(np.concatenate([k * lv.own[fam] + np.union1d(lv.boundary_dofs(fam, d_flags[k]), hanging[l]) for k in range(nv)]).astype(np.int32))
                if l:
                    P.append(resident[l - 1].prolongator(lv, fam))
                    owned.append(P[l])
            self.K = m.matrix(fam)
            owned.append(self.K)
            self.gen = capi.GenericAssembler.from_mesh(m, fam, self.K, order=order)
            owned.append(self.gen)
            if nv > 1:                                                # the plan stays on the scalar pattern S; the system's matrix is its block matrix
                self.S, self.K = self.K, self.K.block_system(nv)
                owned.append(self.K)
            self.xs, self.ndof, self.dim = m.coords(), m.own[fam], m.dim
            self.owners = [m.boundary_owners(fam, d_flags[k]) for k in range(nv)]
            self.b_dofs, self.b_flag, self.b_xy = self.owners[0]
            self.flux_exprs, self.flux_calls = self.flux_faces(fluxes[0])
            self.dirichlets, self.fluxes = dirichlets, fluxes
            for l in range(1, nl):                                    # PP[l] <- PP[l] PPamr[l - 1], before the Dirichlet zeroing; then ZeroInterpolatorDirichletNodes
                if P_amr[l - 1] is not None:
                    P[l] = P[l].matmul(P_amr[l - 1])
                    owned.append(P[l])
                if nv > 1:
                    P[l] = P[l].block_diagonal(nv)
                    owned.append(P[l])
                if bdc[l].size:
                    P[l].mat_zero_rows(bdc[l], 0.0)
                if bdc[l - 1].size:
                    P[l].zero_cols(bdc[l - 1])
            n = nv * self.ndof
            self.SOL, self.RES, self.EPS = ctx.vector(n), ctx.vector(n), ctx.vector(n)
            owned += [self.SOL, self.RES, self.EPS]
            self.PA = P_amr[top]
            if nv > 1:
                if self.PA is not None:
                    self.PA = self.PA.block_diagonal(nv)
                    owned.append(self.PA)
                self.FLUX = self.system_flux()
            self.mg = capi.Multigrid(ctx, nl)
            owned.append(self.mg)
            self.A = [None] * nl
            if self.PA is None:
                self.A[top] = self.K
        except BaseException:
            self.destroy()
            raise

    def flux_faces(self, flux):
        """(exprs, calls) of one variable's flux faces: by kind of face (a prism has quadrilaterals and triangles), each flag's in (element, face) order"""
        f_flags = sorted(int(f) for f in flux)
        faces = {f: self.top.boundary_faces(self.fam, [f]) for f in f_flags}
        calls = []
        widths = sorted({int(n) for f in f_flags for n in faces[f][3]})
        for nn in widths:
            nodes = np.concatenate([faces[f][2][faces[f][3] == nn][:, :nn] for f in f_flags])
            which = np.concatenate([np.full(int((faces[f][3] == nn).sum()), k) for k, f in enumerate(f_flags)])
            calls.append(("lineface" if self.dim == 2 else "triface" if nn in (3, 6, 7) else "quadface", nodes, which))
        return [flux[f] for f in f_flags], calls

    def system_flux(self):
        """the flux faces of every variable, integrated once into a scalar vector each and composed into one vector of the system's size (set-up)"""
        if not any(self.fluxes):
            return None
        scalar, parts = self.ctx.vector(self.ndof), []
        try:
            for k in range(self.nvars):
                scalar.zero()
                self.add_flux(scalar, *self.flux_faces(self.fluxes[k]))
                parts.append(scalar.to_numpy())
        finally:
            scalar.destroy()
        out = self.ctx.vector_from(np.concatenate(parts))
        self.owned.append(out)
        return out

    def boundary_values(self, time=0.0, zeros=False, var=0):
        """(dofs, values): the Dirichlet dofs of variable `var` whose flag has an expression, numbered in the system, and that expression at their coordinates
        and `time`; with zeros also the dofs of the flags given as None, with the value 0 they stand for (a start vector of zeros has them already, a state
        that was set from outside has not)"""
        b_dofs, b_flag, b_xy = self.owners[var]
        b_dofs = b_dofs + var * self.ndof if var else b_dofs
        dofs, values = [], []
        for f in np.unique(b_flag):
            fn = self.dirichlets[var][int(f)]
            sel = b_flag == f
            if fn is not None:
                x4 = np.zeros((int(sel.sum()), 4))
                x4[:, :self.dim], x4[:, 3] = b_xy[sel], time
                dofs.append(b_dofs[sel])
                values.append(fn(x4))
            elif zeros:
                dofs.append(b_dofs[sel])
                values.append(np.zeros(int(sel.sum())))
        return (np.concatenate(dofs), np.concatenate(values)) if dofs else (np.zeros(0, np.int32), np.zeros(0))

    def make_conforming(self, v):
        """v <- P_amr v on a flagged top level: every hanging dof on its constraint row (RES is the scratch)"""
        if self.PA is not None:
            self.RES.matrix_mult(v, self.PA)
            v.assign(self.RES)

    def add_flux(self, res, exprs=None, calls=None):
        """res += the integrals of the flux faces (of the one variable, or those given); a system adds the vector composed at set-up"""
        if self.nvars > 1 and calls is None:
            if self.FLUX is not None:
                res.add(1.0, self.FLUX)
            return
        exprs, calls = (self.flux_exprs, self.flux_calls) if calls is None else (exprs, calls)
        for fgeom, nodes, which in calls:
            if self.dim == 2:
                capi.assemble_neumann_edges(self.ctx, self.fe, nodes, which, exprs, self.xs, res, order=self.order)
            else:
                capi.assemble_neumann_faces_expr(self.ctx, fgeom, self.fe, nodes, which, exprs, self.xs, res, order=self.order)

    def newton_iteration(self, assemble, lin_maxit, smoother, omega, npre, npost):
        """assemble() has to leave Jacobian and residual at SOL in K and RES; then, on a flagged top level, RES <- P_amr^T RES and the operator P_amr^T KK P_amr;
        the boundary rows; the Galerkin chain PP^T KK PP; at most lin_maxit GMRES steps preconditioned by one V-cycle (one level: the exact solve); EPS <- P_amr EPS;
        SOL += EPS.  Returns (Krylov steps, ||RES||_2 before the step, ||EPS||_2, ||SOL||_2 after it)"""
        nl, top = self.nl, self.nl - 1
        A, P, PA, K, bdc = self.A, self.P, self.PA, self.K, self.bdc
        SOL, RES, EPS = self.SOL, self.RES, self.EPS
        mg, owned = self.mg, self.owned
        assemble()
        if PA is not None:
            EPS.matrix_mult_transpose(RES, PA)
            RES.assign(EPS)
            if A[top] is None:
                A[top] = capi.Mat.ptap(PA, K)
                owned.append(A[top])
            else:
                A[top].ptap_numeric(PA, K)
        if bdc[top].size:
            A[top].mat_zero_rows(bdc[top], 1.0)
            RES.set(bdc[top], np.zeros(bdc[top].size))
        rn = RES.l2_norm()
        for l in range(top, 0, -1):
            if A[l - 1] is None:
                A[l - 1] = capi.Mat.ptap(P[l], A[l])
                owned.append(A[l - 1])
            else:
                A[l - 1].ptap_numeric(P[l], A[l])
        for l in range(top):
            if bdc[l].size:
                A[l].mat_zero_rows(bdc[l], 1.0)
        for l in range(nl):
            mg.set_level(l, A[l], P[l], None, smoother, omega, npre if l > 0 else 1, npost if l > 0 else 0)
        mg.setup()
        EPS.zero()
        its, _ = mg.solve(RES, EPS, outer="gmres" if nl > 1 else "preonly", rtol=1e-12, atol=1e-20, maxit=int(lin_maxit))
        if PA is not None:
            RES.matrix_mult(EPS, PA)
            EPS.assign(RES)
        SOL.add(1.0, EPS)
        return its, rn, EPS.l2_norm(), SOL.l2_norm()

    def destroy(self):
        seen = set()
        for q in sorted(reversed(self.owned), key=lambda q: not isinstance(q, capi.Multigrid)):       # the cycle before the operators it holds
            if id(q) not in seen:
                seen.add(id(q))
                q.destroy()
        for lv in self.resident:
            lv.destroy()
        self.owned, self.resident = [], []


class QuasilinearElements:
    def __init__(self, ctx, level0, fe, nlevels, form, dirichlet=None, flux=None, order="seventh", npre=1, npost=1):
        """level0: (kind, ed, xs, ff, own), the arrays of mixed_mesh.read_gambit / tri_box; fe: "linear", "serendipity" or "biquadratic"; nlevels: levels of
        the hierarchy, level0 included; form: a capi.QuasilinearForm (the caller's: it is not destroyed here).
        dirichlet: {face flag: Expr over "x,y,z,t" or None (= 0)}, the boundary values; flux: {face flag: Expr over "x,y,z,t"}, the flux a du/dn on faces that
        are not Dirichlet (a boundary face in neither carries the natural condition, flux 0).  A Dirichlet dof shared by two flags takes the value of the last
        (element, face) that holds it, as GenerateBdc does."""
        if fe not in FAMILY:
            raise ValueError("fe must be one of %s, not %r" % (sorted(FAMILY), fe))
        if int(nlevels) < 1:
            raise ValueError("nlevels must be at least 1, not %r" % (nlevels,))
        self.ctx, self.level0, self.fe, self.nlevels, self.form, self.order = ctx, level0, fe, int(nlevels), form, order
        self.dirichlet, self.flux = dict(dirichlet or {}), dict(flux or {})
        both = set(self.dirichlet) & set(self.flux)
        if both:
            raise ValueError("face flags %s are both Dirichlet and flux faces" % sorted(both))
        self.npre, self.npost = int(npre), int(npost)

    def solve(self, tol=1e-6, max_newton=15, lin_maxit=4, smoother=capi.SMOOTH_GS_COLOR, omega=1.0, selective_levels=0, flag=None, amr_mode="reference", exact=None,
              exact_gradient=None, log=None):
        """Every nonlinear iteration: assemble_form at SOL; the flux faces; on a flagged top level RES <- P_amr^T RES and the operator P_amr^T KK P_amr; the
        boundary rows; the Galerkin chain PP^T KK PP; at most lin_maxit GMRES steps preconditioned by one V-cycle (one level: the exact solve, ex03b's PREONLY);
        EPS <- P_amr EPS; SOL += EPS.  It stops as HasNonLinearConverged does (NonLinearImplicitSystem.cpp:113-153): ||EPS||_2 / (||SOL||_2 + 1e-50) < tol, or
        ||EPS||_2 < 1e-12, or ||SOL||_2 < 1e-12 -- or after max_newton iterations, not converged.
        selective_levels > 0: the last so many levels come from the flagged refinement `flag` (an expression over x, y, z, level), wired as
        Poisson001.run_elements wires them (hanging dofs into the boundary rows, PP[l + 1] <- PP[l + 1] P_amr[l], a conforming start).
        Returns {"solution", "coords", "newton_history": [(Krylov steps, ||RES||_2 before the step, ||EPS||_2 / ||SOL||_2 after it)], "converged", "dofs"};
        with exact (an expression over "x,y,z,t"; exact_gradient: dim of them, else the nodal interpolant is the yardstick) also "l2_error" and "h1_error" from
        capi.ElementMesh.error_norms; with selective_levels also "hanging", "constraints" (capi.ElementMesh.amr_constraints of the top level), "elem_levels"."""
        if exact is None and exact_gradient is not None:
            raise ValueError("exact_gradient without exact")
        h = ResidentHierarchy(self.ctx, self.level0, self.fe, self.nlevels, self.dirichlet, self.flux, self.order, selective_levels, flag, amr_mode)
        try:
            SOL, RES, K = h.SOL, h.RES, h.K
            # the start vector: 0 with the boundary values
            sol0 = np.zeros(h.ndof)
            dofs, values = h.boundary_values()
            sol0[dofs] = values
            SOL.upload(sol0)
            h.make_conforming(SOL)

            def assemble():
                h.gen.assemble_form(K, RES, SOL, self.form)
                h.add_flux(RES)

            history, converged = [], False
            for it in range(int(max_newton)):
                its, rn, en, sn = h.newton_iteration(assemble, lin_maxit, smoother, omega, self.npre, self.npost)
                rel = en / (sn + 1e-50)
                history.append((its, rn, rel))
                if log:
                    log("Nonlinear iteration %d: %d Krylov steps, Res_l2norm = %.6e, Eps_l2norm/Sol_l2norm = %.6e, Eps_l2norm = %.6e" % (it + 1, its, rn, rel, en))
                if rel < tol or en < 1e-12 or sn < 1e-12:
                    converged = True
                    break
            out = {"solution": SOL.to_numpy(), "coords": h.xs[:h.ndof], "newton_history": history, "converged": converged, "dofs": h.ndof}
            if exact is not None:
                en = h.top.error_norms(h.fam, SOL, exact=exact, gradient=exact_gradient, order=self.order)
                out["l2_error"], out["h1_error"] = en["l2"], en["h1"]
            if h.selective_levels:
                out["hanging"], out["constraints"], out["elem_levels"] = h.hanging[h.nl - 1], h.constraints, h.top.elem_levels()[0]
            return out
        finally:
            h.destroy()
