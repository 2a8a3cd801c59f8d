"""Newton's method for a coupled system of m = 1 .. 4 variables of one family,  -sum_l div(A_kl(x, U) grad u_l) + c_k(x, U, grad U) = f_k,  on resident element
meshes of any shape: NonLinearImplicitSystem::MGsolve (src/08_equations/00_stationary/NonLinearImplicitSystem.cpp:157-361) for systems whose variables are
stacked in one matrix, as applications/000_tutorial/ex04 and ex05 (the biharmonic equation as two coupled Laplacians) stack them, on triangles, tetrahedra,
prisms and mixed meshes.  Unknown (k, i) has the number k ndof + i (KKoffset order on one process).

The hierarchy is quasilinear.ResidentHierarchy with nvars = m: levels, scalar transfers, pattern and plan are made where the levels live; the system's matrix is
capi.Mat.block_system of the scalar pattern, its transfers and P_amr capi.Mat.block_diagonal of the scalar ones; Jacobian and residual of every Newton step come
from capi.GenericAssembler.assemble_system (femus_amd/csrc/fh_system.hip) at the current state.

Which row order multigrid needs: the smoothers divide by the diagonal of every level's operator.  ex04 in the reference's order (row u: -lap v = -f, row v:
-lap u + v = 0) has the diagonal blocks 0 and M: it is solved on one level, by the exact solve.  With the rows exchanged, KK = [[K, M], [0, K]], the diagonal
blocks are the two Laplacians, and the default smoother and the V-cycle work as for a scalar equation."""
import numpy as np

from . import capi
from .quasilinear import FAMILY, ResidentHierarchy


class SystemElements:
    def __init__(self, ctx, level0, fe, nlevels, form, dirichlet=None, flux=None, order="seventh", npre=1, npost=1):
        """level0: (kind, ed, xs, ff, own), the arrays of mixed_mesh.read_gambit / tri_box; fe: "linear", "serendipity" or "biquadratic"; nlevels: levels of
        the hierarchy, level0 included; form: a capi.SystemForm of m variables (the caller's: it is not destroyed here).
        dirichlet, flux: lists of m dicts, one per variable, {face flag: Expr over "x,y,z,t" or None (= 0)} the boundary values and {face flag: Expr} the flux
        sum_l A_kl du_l/dn on faces that are not Dirichlet for that variable; every variable has its own Dirichlet faces."""
        if fe not in FAMILY:
            raise ValueError("fe must be one of %s, not %r" % (sorted(FAMILY), fe))
        if int(nlevels) < 1:
            raise ValueError("nlevels must be at least 1, not %r" % (nlevels,))
        m = self.m = int(form.m)
        self.ctx, self.level0, self.fe, self.nlevels, self.form, self.order = ctx, level0, fe, int(nlevels), form, order
        self.dirichlet = [dict(d or {}) for d in (dirichlet if dirichlet is not None else [None] * m)]
        self.flux = [dict(f or {}) for f in (flux if flux is not None else [None] * m)]
        if len(self.dirichlet) != m or len(self.flux) != m:
            raise ValueError("dirichlet and flux are lists of one dict per variable: %d and %d given for %d variables" % (len(self.dirichlet), len(self.flux), m))
        for k in range(m):
            both = set(self.dirichlet[k]) & set(self.flux[k])
            if both:
                raise ValueError("variable %d: face flags %s are both Dirichlet and flux faces" % (k, sorted(both)))
        self.npre, self.npost = int(npre), int(npost)

    def solve(self, tol=1e-6, max_newton=15, lin_maxit=4, smoother=capi.SMOOTH_GS_COLOR, omega=1.0, selective_levels=0, flag=None, amr_mode="reference", exact=None,
              exact_gradient=None, log=None, coarse_direct=None):
        """The iteration, stopping rule, history and lin_maxit of quasilinear.QuasilinearElements.solve, with assemble_system at SOL and the flux vector composed
        at set-up added to RES in every iteration.
        coarse_direct: the context's option of that name for the duration of the solve (afterwards it is back at its default, 1); None: 2, the sparse exact
        solve, for a system of several variables, and no change for one.  The stacked numbering can put a zero block on the diagonal of the coarsest operator
        (ex04 in the reference's row order: 0 and M), which the dense inverse, pivoting inside its 32 x 32 blocks only, cannot factor; the sparse exact solve
        pivots in its fronts.
        Returns {"solution": [m, ndof], "coords", "newton_history", "converged", "dofs" (of one variable)}; with exact (m expressions over "x,y,z,t" or their
        texts; exact_gradient: m lists of dim, else the nodal interpolants are the yardstick) also "l2_error"[k] and "h1_error"[k] from
        capi.ElementMesh.error_norms on the slice of variable k, taken on the device; with selective_levels also "hanging", "constraints" (of one variable;
        they hold for every variable) and "elem_levels"."""
        m = self.m
        if exact is None and exact_gradient is not None:
            raise ValueError("exact_gradient without exact")
        if exact is not None and (len(exact) != m or (exact_gradient is not None and len(exact_gradient) != m)):
            raise ValueError("exact and exact_gradient are lists of one entry per variable")
        h = ResidentHierarchy(self.ctx, self.level0, self.fe, self.nlevels, self.dirichlet, self.flux, self.order, selective_levels, flag, amr_mode, nvars=m) \
            if m > 1 else ResidentHierarchy(self.ctx, self.level0, self.fe, self.nlevels, self.dirichlet[0], self.flux[0], self.order, selective_levels, flag, amr_mode)
        if coarse_direct is None and m > 1:
            coarse_direct = 2
        try:
            if coarse_direct is not None:
                self.ctx.set_option("coarse_direct", int(coarse_direct))
            SOL, RES, K, n = h.SOL, h.RES, h.K, h.ndof
            sol0 = np.zeros(m * n)                                 # the start vector: 0 with the boundary values of every variable
            for k in range(m):
                dofs, values = h.boundary_values(var=k)
                sol0[dofs] = values
            SOL.upload(sol0)
            h.make_conforming(SOL)

            def assemble():
                h.gen.assemble_system(K, RES, SOL, self.form)
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
            out = {"solution": SOL.to_numpy().reshape(m, n), "coords": h.xs[:n], "newton_history": history, "converged": converged, "dofs": n}
            if exact is not None:
                out["l2_error"], out["h1_error"] = [], []
                part = self.ctx.vector(n)
                h.owned.append(part)
                for k in range(m):
                    idx = capi.Index(self.ctx, np.arange(k * n, (k + 1) * n, dtype=np.int32))
                    try:
                        idx.gather_vector(part, SOL)
                        en = h.top.error_norms(h.fam, part, exact=exact[k], gradient=exact_gradient[k] if exact_gradient is not None else None, order=self.order)
                    finally:
                        idx.destroy()
                    out["l2_error"].append(en["l2"])
                    out["h1_error"].append(en["h1"])
            if h.selective_levels:
                out["hanging"], out["constraints"], out["elem_levels"] = h.hanging[h.nl - 1], h.constraints, h.top.elem_levels()[0]
            return out
        finally:
            if coarse_direct is not None:
                self.ctx.set_option("coarse_direct", 1)
            h.destroy()
