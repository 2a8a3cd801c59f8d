"""The theta-method for  u_t - div(a(x, u, t) grad u) + c(x, u, grad u, t) = f(x, u, grad u, t)  on resident element meshes of any shape:
TransientSystem<NonLinearImplicitSystem> (src/08_equations/01_time_dependent/TransientSystem.cpp:62-113: SetUpForSolve, MGsolve, CopySolutionToOldSolution) for
problems like applications/000_tutorial/ex20_time_dependent, on triangles, tetrahedra, prisms and mixed meshes.

The hierarchy -- levels, transfers, pattern, plan, boundary data, P_amr of flagged levels, the Multigrid object -- is quasilinear.ResidentHierarchy, built once
and kept until destroy().  Jacobian and residual of every Newton iteration of every step come from capi.GenericAssembler.assemble_transient
(femus_amd/csrc/fh_transient.hip) at SOL and SOL_old.

TransientSystemElements is the same for a coupled system of m = 1 .. 4 variables of one family,  sum_l M_kl d_t u_l - sum_l div(A_kl grad u_l) + c_k = f_k
(reaction-diffusion systems, the time-dependent biharmonic equation as (u, v = -lap u), Cahn-Hilliard-type splits): ResidentHierarchy with nvars = m, unknown
(k, i) = k ndof + i, and capi.GenericAssembler.assemble_system_transient (femus_amd/csrc/fh_system_transient.hip)."""
import numpy as np

from . import capi
from .quasilinear import FAMILY, ResidentHierarchy


class TransientQuasilinearElements:
    def __init__(self, ctx, level0, fe, nlevels, form, dirichlet=None, flux=None, order="seventh", npre=1, npost=1, theta=1.0, selective_levels=0, flag=None,
                 amr_mode="reference"):
        """level0, fe, nlevels, selective_levels, flag, amr_mode: as quasilinear.QuasilinearElements; form: a capi.TransientForm (the caller's).
        dirichlet: {face flag: text or Expr over "x,y,z,t", or None (= 0)}: the boundary values g(x, t), set at the new time in every step.
        flux: {face flag: text or Expr over "x,y,z"}: the flux a du/dn, constant in time (an Expr compiled over "x,y,z,t", as QuasilinearElements takes
        it, is refused even where it does not use t: compile it over "x,y,z").  theta in [0, 1]: 1 backward Euler, 0.5 Crank-Nicolson."""
        if fe not in FAMILY:
            raise ValueError("fe must be one of %s, not %r" % (sorted(FAMILY), fe))
        if int(nlevels) < 1:
            raise ValueError("nlevels must be at least 1, not %r" % (nlevels,))
        if not 0.0 <= float(theta) <= 1.0:
            raise ValueError("theta must be in [0, 1], not %r" % (theta,))
        dirichlet, flux = dict(dirichlet or {}), dict(flux or {})
        both = set(dirichlet) & set(flux)
        if both:
            raise ValueError("face flags %s are both Dirichlet and flux faces" % sorted(both))
        self.ctx, self.fe, self.form, self.order, self.theta = ctx, fe, form, order, float(theta)
        self.npre, self.npost = int(npre), int(npost)
        self.time, self.h, self._made = 0.0, None, []
        try:
            for f, e in flux.items():
                if isinstance(e, capi.Expr):
                    if e.n_variables() > 3:
                        raise ValueError("the flux of face flag %s is given over %d variables: it may depend on x, y, z only, a time-dependent flux is not served "
                                         "(compile it over \"x,y,z\")" % (f, e.n_variables()))
                else:
                    flux[f] = self._compile(str(e), "x,y,z", "the flux of face flag %s: %%s (it may depend on x, y, z only, a time-dependent flux is not served)" % f)
            for f, e in dirichlet.items():
                if e is not None and not isinstance(e, capi.Expr):
                    dirichlet[f] = self._compile(str(e), "x,y,z,t", "the Dirichlet value of face flag %s: %%s" % f)
            h = self.h = ResidentHierarchy(ctx, level0, fe, nlevels, dirichlet, flux, order, selective_levels, flag, amr_mode)
            self.SOL_old = ctx.vector(h.ndof)
            h.owned.append(self.SOL_old)
            self.FLUX = ctx.vector(h.ndof)
            h.owned.append(self.FLUX)
            self.FLUX.zero()
            h.add_flux(self.FLUX)                                     # once: the face routine has neither a time nor a scale
            self.has_flux = bool(h.flux_calls)
            h.SOL.zero()
            self.SOL_old.zero()
        except BaseException:
            self.destroy()
            raise

    def _compile(self, text, variables, message):
        try:
            e = capi.Expr(text, variables)
        except capi.FemusHipError as err:
            raise ValueError(message % err) from None
        self._made.append(e)
        return e

    def set_initial(self, value):
        """SOL = SOL_old = value at time 0: a text or Expr over "x,y,z,t" evaluated at the dofs with t = 0, or an array of one value per dof; hanging dofs of a
        flagged top level are put on their constraint rows"""
        h = self.h
        if isinstance(value, (str, capi.Expr)):
            e = value if isinstance(value, capi.Expr) else capi.Expr(value, "x,y,z,t")
            try:
                x4 = np.zeros((h.ndof, 4))
                x4[:, :h.dim] = h.xs[:h.ndof]
                u0 = e(x4)
            finally:
                if e is not value:
                    e.destroy()
        else:
            u0 = np.asarray(value, dtype=float)
            if u0.shape != (h.ndof,):
                raise ValueError("the initial state has shape %s, the mesh has %d dofs" % (u0.shape, h.ndof))
        h.SOL.upload(u0)
        h.make_conforming(h.SOL)
        self.SOL_old.assign(h.SOL)
        self.time = 0.0

    def step(self, dt, tol=1e-6, max_newton=15, lin_maxit=4, smoother=capi.SMOOTH_GS_COLOR, omega=1.0, log=None):
        """TransientSystem::MGsolve: time += dt; the Dirichlet dofs of SOL take g(x, time) (UpdateBdc(_time)); then Newton as QuasilinearElements.solve runs it,
        with assemble_transient at (SOL, SOL_old, time, dt, theta) and dt times the flux vector added to RES, stopped as HasNonLinearConverged does.
        SOL_old is left alone: copy_solution_to_old() ends the step.  Returns {"time", "newton_history": [(Krylov steps, ||RES||_2 before the iteration,
        ||EPS||_2 / ||SOL||_2 after it)], "converged"}"""
        h, dt = self.h, float(dt)
        if not dt > 0.0:
            raise ValueError("dt must be positive, not %r" % (dt,))
        self.time += dt
        dofs, values = h.boundary_values(self.time, zeros=True)       # a flag given as None is g = 0: the initial state need not vanish there
        if dofs.size:
            h.SOL.set(dofs, values)
            h.make_conforming(h.SOL)

        def assemble():
            h.gen.assemble_transient(h.K, h.RES, h.SOL, self.SOL_old, self.form, self.time, dt, self.theta)
            if self.has_flux:
                h.RES.add(dt, self.FLUX)

        history, converged = [], False
        for it in range(int(max_newton)):
            its, rn, en, sn = h.newton_iteration(assemble, lin_maxit, smoother, omega, self.npre, self.npost)
            rel = en / (sn + 1e-50)
            history.append((its, rn, rel))
            if log:
                log("t = %.6e, nonlinear iteration %d: %d Krylov steps, Res_l2norm = %.6e, Eps_l2norm/Sol_l2norm = %.6e, Eps_l2norm = %.6e"
                    % (self.time, it + 1, its, rn, rel, en))
            if rel < tol or en < 1e-12 or sn < 1e-12:
                converged = True
                break
        return {"time": self.time, "newton_history": history, "converged": converged}

    def copy_solution_to_old(self):
        self.SOL_old.assign(self.h.SOL)

    def run(self, dt, nsteps, **kw):
        """nsteps times step(dt, **kw) then copy_solution_to_old(); the list of the steps' results"""
        out = []
        for _ in range(int(nsteps)):
            out.append(self.step(dt, **kw))
            self.copy_solution_to_old()
        return out

    def solution(self):
        return self.h.SOL.to_numpy()

    def coords(self):
        return self.h.xs[:self.h.ndof]

    @property
    def constraints(self):
        """capi.ElementMesh.amr_constraints of a flagged top level (hanging dofs, row pointers, masters, weights), else None"""
        return self.h.constraints

    def error_norms(self, exact, gradient=None):
        """{"l2", "h1"} of SOL against exact (capi.ElementMesh.error_norms, which has no time): exact and the entries of gradient are texts over "x,y,z", or
        callables t -> text that are given the current time"""
        at = lambda e: e(self.time) if callable(e) and not isinstance(e, capi.Expr) else e
        h = self.h
        return h.top.error_norms(h.fam, h.SOL, exact=at(exact), gradient=None if gradient is None else [at(g) for g in gradient], order=self.order)

    def destroy(self):
        if self.h is not None:
            self.h.destroy()
            self.h = None
        for e in self._made:
            e.destroy()
        self._made = []


class TransientSystemElements:
    def __init__(self, ctx, level0, fe, nlevels, form, dirichlet=None, flux=None, mass=None, theta=1.0, order="seventh", npre=1, npost=1, selective_levels=0,
                 flag=None, amr_mode="reference"):
        """level0, fe, nlevels, selective_levels, flag, amr_mode: as TransientQuasilinearElements; form: a capi.TransientSystemForm of m variables (the
        caller's).  dirichlet, flux: lists of m dicts, one per variable, as system.SystemElements takes them: {face flag: text or Expr over "x,y,z,t", or None
        (= 0)} the boundary values g_k(x, t), set at the new time in every step, and {face flag: text or Expr over "x,y,z"} the flux sum_l A_kl du_l/dn,
        constant in time; every variable has its own Dirichlet faces.  mass: the m x m matrix M (None: the identity); an equation whose row of M is zero is
        algebraic and taken at the new time whatever theta.  theta in [0, 1]: 1 backward Euler, 0.5 Crank-Nicolson."""
        if fe not in FAMILY:
            raise ValueError("fe must be one of %s, not %r" % (sorted(FAMILY), fe))
        if int(nlevels) < 1:
            raise ValueError("nlevels must be at least 1, not %r" % (nlevels,))
        if not 0.0 <= float(theta) <= 1.0:
            raise ValueError("theta must be in [0, 1], not %r" % (theta,))
        m = self.m = int(form.m)
        dirichlet = [dict(d or {}) for d in (dirichlet if dirichlet is not None else [None] * m)]
        flux = [dict(f or {}) for f in (flux if flux is not None else [None] * m)]
        if len(dirichlet) != m or len(flux) != m:
            raise ValueError("dirichlet and flux are lists of one dict per variable: %d and %d given for %d variables" % (len(dirichlet), len(flux), m))
        for k in range(m):
            both = set(dirichlet[k]) & set(flux[k])
            if both:
                raise ValueError("variable %d: face flags %s are both Dirichlet and flux faces" % (k, sorted(both)))
        self.mass = None
        if mass is not None:
            self.mass = np.array(mass, dtype=float)
            if self.mass.shape != (m, m) or not np.isfinite(self.mass).all():
                raise ValueError("mass must be a finite %d x %d matrix, not %r" % (m, m, mass))
        self.ctx, self.fe, self.form, self.order, self.theta = ctx, fe, form, order, float(theta)
        self.npre, self.npost = int(npre), int(npost)
        self.time, self.h, self._made = 0.0, None, []
        try:
            for k in range(m):
                for f, e in flux[k].items():
                    where = "the flux of variable %d on face flag %s" % (k, f)
                    if isinstance(e, capi.Expr):
                        if e.n_variables() > 3:
                            raise ValueError("%s is given over %d variables: it may depend on x, y, z only, a time-dependent flux is not served "
                                             "(compile it over \"x,y,z\")" % (where, e.n_variables()))
                    else:
                        flux[k][f] = self._compile(str(e), "x,y,z", where + ": %s (it may depend on x, y, z only, a time-dependent flux is not served)")
                for f, e in dirichlet[k].items():
                    if e is not None and not isinstance(e, capi.Expr):
                        dirichlet[k][f] = self._compile(str(e), "x,y,z,t", "the Dirichlet value of variable %d on face flag %s: %%s" % (k, f))
            if m > 1:
                h = self.h = ResidentHierarchy(ctx, level0, fe, nlevels, dirichlet, flux, order, selective_levels, flag, amr_mode, nvars=m)
                self.FLUX = h.FLUX                                        # composed once at set-up: the face routine has neither a time nor a scale
            else:
                h = self.h = ResidentHierarchy(ctx, level0, fe, nlevels, dirichlet[0], flux[0], order, selective_levels, flag, amr_mode)
                self.FLUX = None
                if h.flux_calls:
                    self.FLUX = ctx.vector(h.ndof)
                    h.owned.append(self.FLUX)
                    self.FLUX.zero()
                    h.add_flux(self.FLUX)
            self.SOL_old = ctx.vector(m * h.ndof)
            h.owned.append(self.SOL_old)
            h.SOL.zero()
            self.SOL_old.zero()
        except BaseException:
            self.destroy()
            raise

    _compile = TransientQuasilinearElements._compile

    def set_initial(self, values):
        """SOL = SOL_old = values at time 0: m texts or Exprs over "x,y,z,t", evaluated at the dofs with t = 0, or an array [m, ndof]; hanging dofs of a flagged
        top level are put on their constraint rows"""
        h, m = self.h, self.m
        if isinstance(values, (str, capi.Expr)) or (not isinstance(values, np.ndarray) and len(values) == m and all(isinstance(v, (str, capi.Expr)) for v in values)):
            if isinstance(values, (str, capi.Expr)):
                values = [values]
            if len(values) != m:
                raise ValueError("%d initial states given for %d variables" % (len(values), m))
            x4 = np.zeros((h.ndof, 4))
            x4[:, :h.dim] = h.xs[:h.ndof]
            u0 = np.empty((m, h.ndof))
            for k, value in enumerate(values):
                e = value if isinstance(value, capi.Expr) else capi.Expr(value, "x,y,z,t")
                try:
                    u0[k] = e(x4)
                finally:
                    if e is not value:
                        e.destroy()
        else:
            u0 = np.asarray(values, dtype=float)
            if u0.shape != (m, h.ndof):
                raise ValueError("the initial state has shape %s, %d variables on this mesh have (%d, %d)" % (u0.shape, m, m, h.ndof))
        h.SOL.upload(np.ascontiguousarray(u0).ravel())
        h.make_conforming(h.SOL)
        self.SOL_old.assign(h.SOL)
        self.time = 0.0

    def step(self, dt, tol=1e-6, max_newton=15, lin_maxit=4, smoother=capi.SMOOTH_GS_COLOR, omega=1.0, log=None, coarse_direct=None):
        """What TransientQuasilinearElements.step does, per variable: time += dt; the Dirichlet dofs of variable k take g_k(x, time); Newton with
        assemble_system_transient at (SOL, SOL_old, time, dt, theta, mass), dt times the constant flux vector added to RES, stopped by the same rule.
        coarse_direct: as system.SystemElements.solve handles it -- the context's option for the duration of the step (afterwards back at its default, 1); None:
        2, the sparse exact solve, for several variables (an algebraic equation can put a zero block on the coarsest operator's diagonal), no change for one.
        Returns {"time", "newton_history", "converged"}"""
        h, dt = self.h, float(dt)
        if not dt > 0.0:
            raise ValueError("dt must be positive, not %r" % (dt,))
        if coarse_direct is None and self.m > 1:
            coarse_direct = 2
        self.time += dt
        touched = False
        for k in range(self.m):
            dofs, values = h.boundary_values(self.time, zeros=True, var=k)
            if dofs.size:
                h.SOL.set(dofs, values)
                touched = True
        if touched:
            h.make_conforming(h.SOL)

        def assemble():
            h.gen.assemble_system_transient(h.K, h.RES, h.SOL, self.SOL_old, self.form, self.time, dt, self.theta, self.mass)
            if self.FLUX is not None:
                h.RES.add(dt, self.FLUX)

        history, converged = [], False
        try:
            if coarse_direct is not None:
                self.ctx.set_option("coarse_direct", int(coarse_direct))
            for it in range(int(max_newton)):
                its, rn, en, sn = h.newton_iteration(assemble, lin_maxit, smoother, omega, self.npre, self.npost)
                rel = en / (sn + 1e-50)
                history.append((its, rn, rel))
                if log:
                    log("t = %.6e, nonlinear iteration %d: %d Krylov steps, Res_l2norm = %.6e, Eps_l2norm/Sol_l2norm = %.6e, Eps_l2norm = %.6e"
                        % (self.time, it + 1, its, rn, rel, en))
                if rel < tol or en < 1e-12 or sn < 1e-12:
                    converged = True
                    break
        finally:
            if coarse_direct is not None:
                self.ctx.set_option("coarse_direct", 1)
        return {"time": self.time, "newton_history": history, "converged": converged}

    def copy_solution_to_old(self):
        self.SOL_old.assign(self.h.SOL)

    def run(self, dt, nsteps, **kw):
        """nsteps times step(dt, **kw) then copy_solution_to_old(); the list of the steps' results"""
        out = []
        for _ in range(int(nsteps)):
            out.append(self.step(dt, **kw))
            self.copy_solution_to_old()
        return out

    def solution(self):
        """[m, ndof]"""
        return self.h.SOL.to_numpy().reshape(self.m, self.h.ndof)

    def coords(self):
        return self.h.xs[:self.h.ndof]

    @property
    def constraints(self):
        """capi.ElementMesh.amr_constraints of a flagged top level, of one variable (they hold for every variable), else None"""
        return self.h.constraints

    def error_norms(self, exact, gradient=None):
        """{"l2": [m], "h1": [m]} of SOL against exact, variable by variable (capi.ElementMesh.error_norms on the slice of variable k): exact a list of m texts
        over "x,y,z" or callables t -> text that are given the current time; gradient: m lists of dim such entries, or None"""
        h, m, n = self.h, self.m, self.h.ndof
        if len(exact) != m or (gradient is not None and len(gradient) != m):
            raise ValueError("exact and gradient are lists of one entry per variable")
        at = lambda e: e(self.time) if callable(e) and not isinstance(e, capi.Expr) else e
        out = {"l2": [], "h1": []}
        part = self.ctx.vector(n)
        try:
            for k in range(m):
                idx = capi.Index(self.ctx, np.arange(k * n, (k + 1) * n, dtype=np.int32))
                try:
                    idx.gather_vector(part, h.SOL)
                    en = h.top.error_norms(h.fam, part, exact=at(exact[k]), gradient=None if gradient is None else [at(g) for g in gradient[k]], order=self.order)
                finally:
                    idx.destroy()
                out["l2"].append(en["l2"])
                out["h1"].append(en["h1"])
        finally:
            part.destroy()
        return out

    def destroy(self):
        if self.h is not None:
            self.h.destroy()
            self.h = None
        for e in self._made:
            e.destroy()
        self._made = []
