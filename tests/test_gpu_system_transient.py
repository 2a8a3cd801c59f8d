"""fh_generic_assembler_assemble_system_transient (capi.GenericAssembler.assemble_system_transient, femus_amd/csrc/fh_system_transient.hip): Jacobian and residual
of one Newton iteration of one theta-step of a coupled system, against tests/system_transient_reference.py -- composed from tests/system_reference.py and the
mass matrix of tests/transient_reference.py, and checked on the host by tests/test_system_transient_reference_host.py.  Nothing here compares the kernel with
itself but the repeatability, builder and alternation tests.

Meshes, state and bound are those of tests/test_gpu_system.py: the golden meshes refined once and curved; U = default_rng(11).uniform(-1, 1), and
Uo = default_rng(12).uniform(-1, 1); 1e-12 of the restatement's largest entry; time = 0.7, dt = 0.05.  Forms S (m = dim) and R (m = 4) with their sources times
1 + t: only + - * / and sqrt."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import quasilinear_reference as qr
import system_reference as sr
import system_transient_reference as st
import transient_reference as tr
from test_gpu_generic_assembler import CASES, FES, RULES, Setup, bits, same_bits
from test_gpu_quasilinear import RULE_CASES, host_setup, level
from test_gpu_system import System

pytestmark = pytest.mark.gpu
TIME, DT = 0.7, 0.05
THETAS = (1.0, 0.5, 0.0)
M_FULL = np.array([[1.0, 0.5], [0.0, 2.0]])
M_ALGEBRAIC = np.array([[1.0, 0.0], [0.0, 0.0]])
# c_k = sqrt(u_k + 2): real for u in (-1, 1), NaN for u in (-4, -3)
ROOT = (dict(m=2, c=["sqrt(u0+2)", "sqrt(u1+2)"], c_u=[["0.5/sqrt(u0+2)", None], [None, "0.5/sqrt(u1+2)"]], f=["1+x", "t"]),
        lambda t: dict(m=2, c=[lambda V: np.sqrt(V[:, 3] + 2), lambda V: np.sqrt(V[:, 4] + 2)],
                       c_u=[[lambda V: 0.5 / np.sqrt(V[:, 3] + 2), None], [None, lambda V: 0.5 / np.sqrt(V[:, 4] + 2)]],
                       f=[lambda V: 1 + V[:, 0], lambda V: np.full(V.shape[0], float(t))]))


def pair_of(name, dim):
    """(texts, t -> callables): S (m = dim), R (m = 4), S2 (form S of two variables, on a mesh of any dimension), S2u (the same without t), root"""
    if name == "root":
        return ROOT
    if name == "S2u":
        return sr.form_s(2)[0], st.untimed(sr.form_s(2)[1])
    return {"S": st.form_s, "R": st.form_r, "S2": lambda dim: st.form_s(2)}[name](dim)


def device_form(name, dim):
    from femus_amd import capi
    return capi.TransientSystemForm(**pair_of(name, dim)[0])


def state(case, fe, m, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, m * host_setup(case)[3][qr.FAM[fe]])


@functools.lru_cache(maxsize=None)
def mass(case, fe, order="seventh"):
    s = host_setup(case)
    return tr.mass(s[0], s[1], s[2], fe, order)


@functools.lru_cache(maxsize=None)
def pieces(case, fe, name, order="seventh", time=TIME):
    """(K_sr(U; time), F_sr(U; time), F_sr(Uo; time - DT)) of the restatement: computed once per case, shared, never changed"""
    s = host_setup(case)
    form = pair_of(name, s[2].shape[1])[1]
    m = form(time)["m"]
    Kn, Fn = sr.assemble(s[0], s[1], s[2], fe, form(time), state(case, fe, m, 11), order=order)
    Fo = sr.assemble(s[0], s[1], s[2], fe, form(time - DT), state(case, fe, m, 12), order=order)[1]
    Fn.setflags(write=False)
    Fo.setflags(write=False)
    return m, Kn, Fn, Fo


def reference(case, fe, name, theta, M=None, order="seventh", time=TIME):
    m, Kn, Fn, Fo = pieces(case, fe, name, order, time)
    M = st.mass_matrix(m, M)
    return st.combine(mass(case, fe, order), M, st.thetas(M, theta), Kn, Fn, Fo, state(case, fe, m, 11), state(case, fe, m, 12), DT)


class Step(System):
    """test_gpu_system.System with the old state beside the new one"""

    def __init__(self, ctx, case, fe, m, **kw):
        super().__init__(ctx, case, fe, m, **kw)
        self.case, self.fe = case, fe
        self.uo = state(case, fe, m, 12)
        self.OLD = ctx.vector_from(self.uo)

    def step(self, form, theta=0.5, mass=None, time=TIME, gen=None, K=None, old=None):
        (gen or self.gen).assemble_system_transient(K or self.K, self.RES, self.SOL, old if old is not None else self.OLD, form, time, DT, theta, mass)
        return bits(K or self.K, self.RES)

    def close(self):
        self.OLD.destroy()
        super().close()


# ---- the values ----
@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("case", CASES)
def test_form_s_against_the_restatement(ctx, case, fe):
    """theta = 1, 0.5 and 0: K and RES within 1e-12 of the restatement's largest entry; the Jacobian is not its transpose"""
    dim = level(case)[2].shape[1]
    q = Step(ctx, case, fe, dim)
    form = device_form("S", dim)
    try:
        for theta in THETAS:
            q.step(form, theta)
            print(case, fe, "form S theta", theta, q.gen.system_transient_chunks(dim), end=": ")
            q.check(reference(case, fe, "S", theta))
            if theta == 1.0:
                K = q.K.to_scipy()
                assert abs(K - K.T).max() > 1e-3 * abs(K).max()
        assert all(gc >= 1 and lanes in (16, 32, 64) for gc, lanes in q.gen.system_transient_chunks(dim).values())
    finally:
        form.destroy()
        q.close()


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("case,fe", RULE_CASES)
def test_form_r_at_every_gauss_rule(ctx, case, fe, order):
    """four variables, theta = 0.5: rules of one chunk and of several, a last chunk that is not full among them"""
    q = Step(ctx, case, fe, 4, order=order)
    form = device_form("R", 3)
    try:
        q.step(form, 0.5)
        print(case, fe, order, "form R", q.gen.system_transient_chunks(4), end=": ")
        q.check(reference(case, fe, "R", 0.5, order=order))
    finally:
        form.destroy()
        q.close()


def test_form_r_on_hex27(ctx):
    """the largest element body: HEX27, TET10, WEDGE21 with four variables"""
    case, fe = "mixed3d", "biquadratic"
    q = Step(ctx, case, fe, 4)
    form = device_form("R", 3)
    try:
        q.step(form, 0.5)
        chunks = q.gen.system_transient_chunks(4)
        print(case, fe, "form R", chunks, end=": ")
        q.check(reference(case, fe, "R", 0.5))
        assert "hex" in chunks and chunks["hex"][0] < 27                 # more than one Gauss chunk
    finally:
        form.destroy()
        q.close()


@pytest.mark.parametrize("case,fe", [("tri", "biquadratic"), ("mixed3d", "linear")])
def test_mass_matrices(ctx, case, fe):
    """M = [[1, 0.5], [0, 2]], and M = [[1, 0], [0, 0]] at theta = 0.5: equation 1 is algebraic, its rows are dt times assemble_system's at the new state"""
    from femus_amd import capi
    q = Step(ctx, case, fe, 2)
    n = q.ndof
    timed, plain, stationary = device_form("S2", 2), device_form("S2u", 2), capi.SystemForm(**sr.form_s(2)[0])
    try:
        for theta in THETAS:
            q.step(timed, theta, M_FULL)
            print(case, fe, "M full, theta", theta, end=": ")
            q.check(reference(case, fe, "S2", theta, M_FULL))
        for name, form in (("S2", timed), ("S2u", plain)):
            for theta in (0.5, 0.0):
                q.step(form, theta, M_ALGEBRAIC)
                print(case, fe, "M with a zero row, form", name, "theta", theta, end=": ")
                q.check(reference(case, fe, name, theta, M_ALGEBRAIC))
        q.step(plain, 0.5, M_ALGEBRAIC)
        Kt, Ft = q.K.to_scipy(), q.RES.to_numpy()
        q.assemble(stationary)
        Ks, Fs = q.K.to_scipy(), q.RES.to_numpy()
        dK, dF = abs(Kt[n:] - DT * Ks[n:]).max(), np.abs(Ft[n:] - DT * Fs[n:]).max()
        print("algebraic rows: |K - dt K_system| = %.3e of %.3e, |RES - dt RES_system| = %.3e of %.3e" % (dK, DT * abs(Ks).max(), dF, DT * np.abs(Fs).max()))
        assert dK <= 1e-12 * DT * abs(Ks).max() and dF <= 1e-12 * DT * np.abs(Fs).max()
        assert abs(Kt[:n] - DT * Ks[:n]).max() > 1e-3 * DT * abs(Ks).max()              # the other equation has its mass term and its theta
    finally:
        for f in (timed, plain, stationary):
            f.destroy()
        q.close()


@pytest.mark.parametrize("case,fe", [("tri", "biquadratic"), ("tet", "serendipity"), ("mixed3d", "biquadratic")])
def test_one_variable_without_a_mass_matrix_is_assemble_transient(ctx, case, fe):
    """m = 1, mass NULL: within 1e-12 of assemble_transient's result and of the restatement"""
    from femus_amd import capi
    q = Step(ctx, case, fe, 1)
    hs = host_setup(case)
    dim = hs[2].shape[1]
    text, call = tr.timed(qr.form_b(dim), dim)
    scalar, form = capi.TransientForm(**text), capi.TransientSystemForm(**sr.scalar_texts([text]))
    try:
        for theta in THETAS:
            q.gen.assemble_transient(q.s.K, q.s.RES, q.SOL, q.OLD, scalar, TIME, DT, theta)
            Kt, Ft = q.s.K.to_scipy().copy(), q.s.RES.to_numpy().copy()
            q.step(form, theta)
            dK, dF = abs(q.K.to_scipy() - Kt).max(), np.abs(q.RES.to_numpy() - Ft).max()
            print(case, fe, "theta", theta, "|K - K_transient| = %.3e of %.3e, |RES - RES_transient| = %.3e of %.3e" % (dK, abs(Kt).max(), dF, np.abs(Ft).max()), end="; ")
            assert dK <= 1e-12 * abs(Kt).max() and dF <= 1e-12 * np.abs(Ft).max()
            q.check(st.assemble(hs[0], hs[1], hs[2], fe, lambda t: sr.from_scalar([call(t)]), q.u, q.uo, TIME, DT, theta, Mass=mass(case, fe)))
        q.s.K.zero()
        q.step(form, 0.5, K=q.s.K)                                 # with one variable the object's own matrix serves as well
        q.step(form, 0.5)
        assert np.array_equal(q.s.K.to_scipy().data.view(np.uint64), q.K.to_scipy().data.view(np.uint64))
    finally:
        scalar.destroy()
        form.destroy()
        q.close()


@pytest.mark.parametrize("case,fe", [("tri", "serendipity"), ("tet", "linear")])
def test_theta_one_ignores_the_old_state_outside_the_mass_term(ctx, case, fe):
    """c_k = sqrt(u_k + 2) with Uo in (-4, -3): NaN at the old state, which theta = 1 never evaluates"""
    q = Step(ctx, case, fe, 2)
    hs = host_setup(case)
    form = device_form("root", 2)
    uo = state(case, fe, 2, 12, lo=-4.0, hi=-3.0)
    old = ctx.vector_from(uo)
    try:
        for M in (None, M_FULL, M_ALGEBRAIC):
            q.step(form, 1.0, M, old=old)
            assert np.isfinite(q.RES.to_numpy()).all() and np.isfinite(q.K.to_scipy().data).all()
            q.check(st.assemble(hs[0], hs[1], hs[2], fe, ROOT[1], q.u, uo, TIME, DT, 1.0, M=M, Mass=mass(case, fe)))
    finally:
        form.destroy()
        old.destroy()
        q.close()


@pytest.mark.parametrize("case,fe", [("tri", "serendipity"), ("tet", "linear")])
def test_theta_zero_gives_the_mass_blocks(ctx, case, fe):
    """the mirror image: U in (-4, -3), where the programs are NaN; theta = 0 never evaluates there, and KK = kron(M, mass matrix)"""
    q = Step(ctx, case, fe, 2)
    hs = host_setup(case)
    form = device_form("root", 2)
    u = state(case, fe, 2, 13, lo=-4.0, hi=-3.0)
    q.SOL.upload(u)
    try:
        for M in (None, M_FULL):
            q.step(form, 0.0, M)
            assert np.isfinite(q.RES.to_numpy()).all() and np.isfinite(q.K.to_scipy().data).all()
            q.check(st.assemble(hs[0], hs[1], hs[2], fe, ROOT[1], u, q.uo, TIME, DT, 0.0, M=M, Mass=mass(case, fe)))
            KM = sp.kron(sp.csr_matrix(st.mass_matrix(2, M)), mass(case, fe), format="csr")
            assert abs(q.K.to_scipy() - KM).max() <= 1e-12 * abs(KM).max()
    finally:
        form.destroy()
        q.close()


def test_time_is_live(ctx):
    """two calls that differ in time only give the two restatements: a t frozen into an uploaded buffer cannot pass"""
    case, fe = "tri", "biquadratic"
    q = Step(ctx, case, fe, 2)
    form = device_form("S", 2)
    try:
        seen = []
        for time in (TIME, 1.3, TIME):
            q.step(form, 0.5, time=time)
            q.check(reference(case, fe, "S", 0.5, time=time))
            seen.append(q.RES.to_numpy().copy())
        assert np.abs(seen[0] - seen[1]).max() > 1e-3 * np.abs(seen[0]).max()
        assert np.array_equal(seen[0], seen[2])
    finally:
        form.destroy()
        q.close()


# ---- the object ----
@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("case,fe,name", [("tet", "biquadratic", "S"), ("tet", "linear", "R"), ("mixed3d", "serendipity", "S"), ("tri", "linear", "S")])
def test_three_assemblies_give_the_same_bits_without_allocating(ctx, case, fe, name, poison):
    """also with debug_poison set before create: the work buffers start as 0xFF bytes, and the row pass must read nothing the element pass has not written"""
    before = int(os.environ.get("FEMUS_HIP_POISON", "0") or 0)
    ctx.set_option("debug_poison", 1 if poison else before)
    try:
        dim = level(case)[2].shape[1]
        m = 4 if name == "R" else dim
        q = Step(ctx, case, fe, m)
        form = device_form(name, dim)
        try:
            n0 = q.gen.info()
            first = q.step(form)
            n1 = q.gen.info()
            assert n1["device_allocations"] == n0["device_allocations"] + 2                     # Kb and Fb of this m
            assert n1["device_bytes"] - n0["device_bytes"] >= (m * m - 1) * 8 * q.gen.plan()[2].size
            q.check(reference(case, fe, name, 0.5))
            assert np.isfinite(q.RES.to_numpy()).all() and np.isfinite(q.K.to_scipy().data).all()
            assert same_bits(q.step(form), first) and same_bits(q.step(form), first)
            assert q.gen.info()["device_allocations"] == n1["device_allocations"]
            assert q.gen.system_transient_chunks() == q.gen.system_transient_chunks(m)
            assert all(gc == 0 for gc, _ in q.gen.system_chunks(m).values())                     # the stationary body has not been planned
        finally:
            form.destroy()
            q.close()
    finally:
        ctx.set_option("debug_poison", before)


@pytest.mark.parametrize("case,fe", [("tet", "biquadratic"), ("mixed2d", "linear")])
def test_the_bodies_alternate_on_one_object(ctx, case, fe):
    """assemble_system and assemble_system_transient at the same m, then also assemble_transient and assemble: each gives the bits it gives alone (a fresh
    object per path), and the m^2 work buffers are held once, whichever of the two system calls came first"""
    from femus_amd import capi
    dim = level(case)[2].shape[1]
    step_form, sys_form = device_form("S", dim), capi.SystemForm(**sr.form_s(dim)[0])
    tform = capi.TransientForm(**tr.timed(qr.form_b(dim), dim)[0])
    SOLD = {}

    def scalar_old(q):
        if id(q) not in SOLD:
            SOLD[id(q)] = ctx.vector_from(0.5 * q.s.u)
        return SOLD[id(q)]

    calls = {"step": lambda q: q.step(step_form),
             "system": lambda q: q.assemble(sys_form),
             "transient": lambda q: (q.gen.assemble_transient(q.s.K, q.s.RES, q.s.SOL, scalar_old(q), tform, 0.25, 0.125, 0.5), bits(q.s.K, q.s.RES))[1],
             "poisson": lambda q: q.s.resident()}
    want = {}
    try:
        for n, call in calls.items():                              # a fresh object for each path
            q = Step(ctx, case, fe, dim)
            try:
                want[n] = call(q)
            finally:
                q.close()
        for order in (("step", "system"), ("system", "step")):
            q = Step(ctx, case, fe, dim)
            try:
                a0 = q.gen.info()
                for n in order + ("step", "system", "system", "step"):
                    assert same_bits(calls[n](q), want[n]), (order, n)
                a1 = q.gen.info()
                assert a1["device_allocations"] == a0["device_allocations"] + 2                  # one Kb and one Fb for the two bodies
                assert a1["device_bytes"] - a0["device_bytes"] < 2 * dim * dim * 8 * q.gen.plan()[2].size                # not twice the m^2 nent doubles of Kb
                for n in ("transient", "step", "poisson", "system", "step", "transient", "step", "poisson", "step"):
                    assert same_bits(calls[n](q), want[n]), (order, n)
                assert q.gen.info()["device_allocations"] == a1["device_allocations"]
                q.step(step_form)
                q.check(reference(case, fe, "S", 0.5))
            finally:
                q.close()
    finally:
        for f in (step_form, sys_form, tform):
            f.destroy()
        for v in SOLD.values():
            v.destroy()


@pytest.mark.parametrize("case", CASES)
def test_both_builders_give_the_same_bits(ctx, case):
    from femus_amd import capi, mixed_mesh
    from test_gpu_generic_assembler import GOLDEN, curved
    fe = "biquadratic"
    if case == "tri":
        lv = mixed_mesh.tri_box(3, 2, (0., 0.), (1.5, 1.))
    else:
        lv = mixed_mesh.read_gambit(os.path.join(GOLDEN, {"tet": "cube_Tet.neu", "wedge": "cube_Wedge.neu", "mixed3d": "cube_all_shapes_Six_boundary_groups.neu",
                                                          "mixed2d": "square_mixed.neu"}[case]))
    lv = mixed_mesh.refine(*lv[:4])
    dim = lv[2].shape[1]
    s = Setup(ctx, case, fe, lv=(lv[0], lv[1], lv[2], lv[4]))
    mesh = capi.ElementMesh.from_arrays(ctx, lv[0], lv[1], curved(lv[2]), lv[3], lv[4])
    gd = capi.GenericAssembler.from_mesh(mesh, fe, s.K2)
    mesh.destroy()
    form = device_form("S", dim)
    K, K2 = s.K.block_system(dim), s.K2.block_system(dim)
    rng = np.random.default_rng(11)
    SOL, OLD, RES = ctx.vector_from(rng.uniform(-1, 1, dim * s.ndof)), ctx.vector_from(rng.uniform(-1, 1, dim * s.ndof)), ctx.vector(dim * s.ndof)
    try:
        s.gen.assemble_system_transient(K, RES, SOL, OLD, form, TIME, DT, 0.5, M_FULL if dim == 2 else None)
        a = bits(K, RES)
        gd.assemble_system_transient(K2, RES, SOL, OLD, form, TIME, DT, 0.5, M_FULL if dim == 2 else None)
        assert same_bits(a, bits(K2, RES))
        assert gd.system_transient_chunks(dim) == s.gen.system_transient_chunks(dim)
    finally:
        gd.destroy()
        form.destroy()
        for q in (K, K2, OLD):
            q.destroy()
        s.close()


def test_refusals_leave_the_matrix_values_as_they_were(ctx):
    from femus_amd import capi
    q = Step(ctx, "tri", "serendipity", 2)
    n = q.ndof
    form = device_form("S", 2)
    wide = capi.Expr("u0+t+w", capi.TransientSystemForm.variables(2) + ",w")
    bad_vars = capi.TransientSystemForm(2)
    bad_vars.exprs[("c", (1,))] = wide                            # past the constructor's own check
    bad_vars._refresh()
    bad_dim = capi.TransientSystemForm(2, c_g=[[None, ["u0", "u0", "u0"]], [None, None]])
    five = capi.TransientSystemForm(2)
    five._s.m = 5
    K3, short, long_ = q.s.K.block_system(3), ctx.vector(2 * n - 1), ctx.vector(2 * n + 3)
    nan_mass, inf_mass = np.array([[1.0, float("nan")], [0.0, 1.0]]), np.array([[1.0, 0.0], [float("inf"), 1.0]])
    who = "fh_generic_assembler_assemble_system_transient"
    call = lambda **kw: q.gen.assemble_system_transient(**{**dict(K=q.K, res=q.RES, sol=q.SOL, sol_old=q.OLD, form=form, time=TIME, dt=DT, theta=0.5, mass=M_FULL), **kw})
    try:
        want = q.step(form, 0.5, M_FULL)
        q.check(reference("tri", "serendipity", "S", 0.5, M_FULL))
        refused = [(dict(form=bad_vars), who + ": the program c\\[1\\] has 13 variables, at most 12"),
                   (dict(form=bad_dim), who + r": c_g\[0\]\[1\]\[2\] given on a mesh of dimension 2"),
                   (dict(form=five, mass=None), who + ": 5 variables"),
                   (dict(form=None), who + ": null form"),
                   (dict(K=K3), who + ": not the block system of 2 variables"),
                   (dict(K=q.s.K), who + ": not the block system of 2 variables"),
                   (dict(res=short), who + ": size mismatch"),
                   (dict(sol=short), who + ": size mismatch"),
                   (dict(sol_old=None), who + ": null sol_old"),
                   (dict(sol_old=short), who + ": sol_old has %d entries, 2 variables on this object have %d" % (2 * n - 1, 2 * n)),
                   (dict(sol_old=long_), who + ": sol_old has %d entries, sol has %d" % (2 * n + 3, 2 * n)),
                   (dict(dt=0.0), who + ": dt = 0 is not positive"), (dict(dt=-DT), "is not positive"),
                   (dict(theta=1.5), who + ": theta = 1.5 is outside"), (dict(theta=-0.1), "is outside"),
                   (dict(time=float("nan")), who + ": time, dt and theta must be finite"), (dict(dt=float("inf")), "must be finite"),
                   (dict(theta=float("nan")), "must be finite"),
                   (dict(mass=nan_mass), who + r": mass\[0\]\[1\] is not finite"), (dict(mass=inf_mass), who + r": mass\[1\]\[0\] is not finite")]
        for kw, message in refused:
            with pytest.raises(capi.FemusHipError, match=message):
                call(**kw)
            assert same_bits(bits(q.K, q.RES), want), message
        with pytest.raises(ValueError, match="mass has shape"):
            call(mass=np.eye(3))
        with pytest.raises(capi.FemusHipError, match="fh_generic_assembler_assemble_system: the program f\\[0\\] has 12 variables, at most 11"):
            q.gen.assemble_system(q.K, q.RES, q.SOL, form)         # the stationary call keeps its 3 + 4 m
        assert not K3.values().any()
        assert same_bits(q.step(form, 0.5, M_FULL), want)
    finally:
        for f in (form, bad_vars, bad_dim, five, wide, short, long_):
            f.destroy()
        K3.destroy()
        q.close()
