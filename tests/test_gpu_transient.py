"""fh_generic_assembler_assemble_transient (capi.GenericAssembler.assemble_transient, femus_amd/csrc/fh_transient.hip): Jacobian and residual of one Newton
iteration of one theta-step of u_t - div(a grad u) + c = f, against tests/transient_reference.py -- composed from tests/quasilinear_reference.py, and checked on
the host by tests/test_transient_reference_host.py.  Nothing here compares the kernel with itself but the repeatability, builder and alternation tests.

Meshes, families and forms A and B as tests/test_gpu_quasilinear.py; the source carries the time, f (1 + t); u = default_rng(11).uniform(-1, 1) (Setup's) and
uo = default_rng(12).uniform(-1, 1); time = 0.7, dt = 0.05.  Only + - * /, sqrt and the exp of the source, so host and device agree to rounding."""
import functools
import os

import numpy as np
import pytest

import quasilinear_reference as qr
import transient_reference as tr
from test_gpu_generic_assembler import CASES, FES, RULES, Setup, bits, same_bits
from test_gpu_quasilinear import FORMS, RULE_CASES, host_setup, level

pytestmark = pytest.mark.gpu
TIME, DT = 0.7, 0.05
THETAS = (1.0, 0.5, 0.0)
# c = sqrt(u + 2): real for u in (-1, 1), NaN for uo in (-4, -3)
ROOT = (dict(c="sqrt(u+2)", c_u="0.5/sqrt(u+2)"), dict(c=lambda v: np.sqrt(v[3] + 2), c_u=lambda v: 0.5 / np.sqrt(v[3] + 2)))


def pair_of(name, dim):
    return ROOT if name == "root" else FORMS[name](dim)


def state(case, fe, seed=12, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, host_setup(case)[3][qr.FAM[fe]])


@functools.lru_cache(maxsize=None)
def mass(case, fe, order="seventh"):
    s = host_setup(case)
    return tr.mass(s[0], s[1], s[2], fe, order)


@functools.lru_cache(maxsize=None)
def pieces(case, fe, name, order="seventh", time=TIME, old=True):
    """(M, K_qr(u; time), F_qr(u; time), F_qr(uo; time - DT)) of the restatement: computed once per case, shared, never changed"""
    s = host_setup(case)
    dim = s[2].shape[1]
    form = tr.timed(pair_of(name, dim), dim)[1]
    u, uo = state(case, fe, 11), state(case, fe)
    return tr.pieces(s[0], s[1], s[2], fe, form, u, uo, time, DT, order, old=old, M=mass(case, fe, order))


def reference(case, fe, name, theta, order="seventh", time=TIME, uo=None):
    p = pieces(case, fe, name, order, time, old=uo is None)
    return tr.combine(p, state(case, fe, 11), state(case, fe) if uo is None else uo, DT, theta)


def device_form(name, dim):
    from femus_amd import capi
    return capi.TransientForm(**tr.timed(pair_of(name, dim), dim)[0])


def check(s, ref):
    Kr, Fr = ref
    dK, dF = abs(s.K.to_scipy() - Kr).max(), np.abs(s.RES.to_numpy() - Fr).max()
    print("|K - restatement| = %.3e of %.3e, |RES - restatement| = %.3e of %.3e" % (dK, abs(Kr).max(), dF, np.abs(Fr).max()))
    assert dK <= 1e-12 * abs(Kr).max()
    assert dF <= 1e-12 * np.abs(Fr).max()


def old_state(s, case, fe, **kw):
    return s.ctx.vector_from(state(case, fe, **kw))


def tr_bits(s, form, old, theta=0.5, time=TIME, gen=None, K=None):
    (gen or s.gen).assemble_transient(K or s.K, s.RES, s.SOL, old, form, time, DT, theta)
    return bits(K or s.K, s.RES)


@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("case", CASES)
def test_values_against_the_restatement(ctx, case, fe):
    """both forms, theta = 1, 0.5 and 0: K and RES within 1e-12 of the restatement's largest entry; form A's K is not its transpose"""
    s = Setup(ctx, case, fe, lv=level(case))
    dim = s.xs.shape[1]
    forms = {n: device_form(n, dim) for n in ("A", "B")}
    old = old_state(s, case, fe)
    try:
        for name in ("A", "B"):
            for theta in THETAS:
                tr_bits(s, forms[name], old, theta)
                print(case, fe, "form", name, "theta", theta, end=": ")
                check(s, reference(case, fe, name, theta))
                if name == "A" and theta == 1.0:
                    K = s.K.to_scipy()
                    assert abs(K - K.T).max() > 1e-3 * abs(K - mass(case, fe)).max()
        print(case, fe, "Gauss chunks", s.gen.transient_chunks())
        assert all(v >= 1 for v in s.gen.transient_chunks().values())
    finally:
        for f in forms.values():
            f.destroy()
        old.destroy()
        s.close()


@pytest.mark.parametrize("case,fe", RULE_CASES)
def test_the_limit_is_the_stationary_kernel_and_the_mass_matrix(ctx, case, fe):
    """theta = 1 and sol_old = sol: RES = dt x assemble_form's RES, and K - dt x K_form = the restatement's M.  Bounds: 1e-12 of the largest entry of dt RES_form,
    and of K -- the difference K - dt K_form cancels entries of K's size, so its rounding is K's, not M's"""
    from femus_amd import capi
    s = Setup(ctx, case, fe, lv=level(case))
    dim = s.xs.shape[1]
    form = capi.QuasilinearForm(**qr.with_source(FORMS["B"](dim), dim)[0])      # no t in it: the same programs serve both calls
    try:
        s.gen.assemble_form(s.K, s.RES, s.SOL, form)
        Kf, Ff = s.K.to_scipy().copy(), s.RES.to_numpy().copy()
        s.gen.assemble_transient(s.K, s.RES, s.SOL, s.SOL, form, TIME, DT, 1.0)
        Kt, Ft = s.K.to_scipy(), s.RES.to_numpy()
        dF, dK = np.abs(Ft - DT * Ff).max(), abs(Kt - DT * Kf - mass(case, fe)).max()
        print("%s %s: |RES - dt RES_form| = %.3e of %.3e, |K - dt K_form - M| = %.3e of %.3e" % (case, fe, dF, np.abs(DT * Ff).max(), dK, abs(Kt).max()))
        assert dF <= 1e-12 * np.abs(DT * Ff).max()
        assert dK <= 1e-12 * abs(Kt).max()
    finally:
        form.destroy()
        s.close()


def test_time_is_live(ctx):
    """two calls that differ in time only give the two restatements: a t frozen into an uploaded buffer cannot pass"""
    case, fe = "tri", "biquadratic"
    s = Setup(ctx, case, fe, lv=level(case))
    form, old = device_form("B", 2), old_state(s, case, fe)
    try:
        seen = []
        for time in (TIME, 1.3, TIME):
            tr_bits(s, form, old, 0.5, time=time)
            check(s, reference(case, fe, "B", 0.5, time=time))
            seen.append(s.RES.to_numpy().copy())
        assert np.abs(seen[0] - seen[1]).max() > 1e-3 * np.abs(seen[0]).max()
        assert np.array_equal(seen[0], seen[2])
    finally:
        form.destroy()
        old.destroy()
        s.close()


@pytest.mark.parametrize("case,fe", [("tri", "serendipity"), ("tet", "linear")])
def test_theta_one_ignores_the_old_state_outside_the_mass_term(ctx, case, fe):
    """c = sqrt(u + 2) with uo in (-4, -3): NaN at the old state, which theta = 1 never evaluates"""
    s = Setup(ctx, case, fe, lv=level(case))
    form = device_form("root", s.xs.shape[1])
    uo = state(case, fe, lo=-4.0, hi=-3.0)
    old = ctx.vector_from(uo)
    try:
        tr_bits(s, form, old, 1.0)
        assert np.isfinite(s.RES.to_numpy()).all() and np.isfinite(s.K.to_scipy().data).all()
        check(s, reference(case, fe, "root", 1.0, uo=uo))
    finally:
        form.destroy()
        old.destroy()
        s.close()


@pytest.mark.parametrize("case,fe", [("tri", "serendipity"), ("tet", "linear")])
def test_theta_zero_ignores_the_new_state_outside_the_mass_term(ctx, case, fe):
    """the mirror image: u in (-4, -3), where c = sqrt(u + 2) is NaN, and uo in (-1, 1); theta = 0 never evaluates at u, and K is the mass matrix"""
    s = Setup(ctx, case, fe, lv=level(case))
    hs = host_setup(case)
    dim = s.xs.shape[1]
    form = device_form("root", dim)
    u, uo = state(case, fe, seed=13, lo=-4.0, hi=-3.0), state(case, fe)
    s.SOL.upload(u)
    old = ctx.vector_from(uo)
    try:
        tr_bits(s, form, old, 0.0)
        assert np.isfinite(s.RES.to_numpy()).all() and np.isfinite(s.K.to_scipy().data).all()
        check(s, tr.assemble(hs[0], hs[1], hs[2], fe, tr.timed(ROOT, dim)[1], u, uo, TIME, DT, 0.0, M=mass(case, fe)))
        assert abs(s.K.to_scipy() - mass(case, fe)).max() <= 1e-12 * abs(mass(case, fe)).max()
    finally:
        form.destroy()
        old.destroy()
        s.close()


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("case,fe", RULE_CASES)
def test_every_gauss_rule_against_the_restatement(ctx, case, fe, order):
    """also chunks that do not divide the number of Gauss points"""
    s = Setup(ctx, case, fe, order=order, lv=level(case))
    name = "A" if order in ("first", "fifth", "ninth") else "B"
    form, old = device_form(name, s.xs.shape[1]), old_state(s, case, fe)
    try:
        tr_bits(s, form, old, 0.5)
        print(case, fe, order, s.gen.transient_chunks(), end=": ")
        check(s, reference(case, fe, name, 0.5, order))
    finally:
        form.destroy()
        old.destroy()
        s.close()


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
    s = Setup(ctx, case, fe, lv=(lv[0], lv[1], lv[2], lv[4]))
    m = capi.ElementMesh.from_arrays(ctx, lv[0], lv[1], curved(lv[2]), lv[3], lv[4])
    gd = capi.GenericAssembler.from_mesh(m, fe, s.K2)
    m.destroy()
    forms = {n: device_form(n, s.xs.shape[1]) for n in ("A", "B")}
    old = old_state(s, case, fe)
    try:
        for name, form in forms.items():
            assert same_bits(tr_bits(s, form, old), tr_bits(s, form, old, gen=gd, K=s.K2))
        assert gd.transient_chunks() == s.gen.transient_chunks()
    finally:
        gd.destroy()
        for f in forms.values():
            f.destroy()
        old.destroy()
        s.close()


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("case,fe", [("tet", "biquadratic"), ("tet", "linear"), ("mixed3d", "serendipity"), ("tri", "linear")])
def test_three_assemblies_give_the_same_bits_without_allocating(ctx, case, fe, poison):
    """also with debug_poison set before create: the work buffers start as 0xFF bytes, and the row pass must read nothing the element pass has not written"""
    before = int(os.environ.get("FEMUS_HIP_POISON", "0") or 0)
    ctx.set_option("debug_poison", 1 if poison else before)
    try:
        s = Setup(ctx, case, fe, lv=level(case))
    finally:
        ctx.set_option("debug_poison", before)
    form, old = device_form("B", s.xs.shape[1]), old_state(s, case, fe)
    try:
        first = tr_bits(s, form, old)
        n1 = s.gen.info()["device_allocations"]
        check(s, reference(case, fe, "B", 0.5))
        assert np.isfinite(s.RES.to_numpy()).all() and np.isfinite(s.K.to_scipy().data).all()
        assert same_bits(tr_bits(s, form, old), first) and same_bits(tr_bits(s, form, old), first)
        assert s.gen.info()["device_allocations"] == n1
    finally:
        form.destroy()
        old.destroy()
        s.close()


@pytest.mark.parametrize("case,fe", [("tet", "biquadratic"), ("mixed2d", "linear")])
def test_the_three_assemblies_alternate_on_one_object(ctx, case, fe):
    """assemble, assemble_form and assemble_transient share the program buffer and the work buffers: each gives the bits of a fresh object, whatever ran before"""
    from femus_amd import capi
    dim = host_setup(case)[2].shape[1]
    qform, tform = capi.QuasilinearForm(**qr.with_source(FORMS["A"](dim), dim)[0]), device_form("B", dim)
    calls = {"poisson": lambda s, old: s.resident(),
             "form": lambda s, old: (s.gen.assemble_form(s.K, s.RES, s.SOL, qform), bits(s.K, s.RES))[1],
             "transient": lambda s, old: tr_bits(s, tform, old)}
    want = {}
    try:
        for n, call in calls.items():                              # a fresh object for each path
            s = Setup(ctx, case, fe, lv=level(case))
            old = old_state(s, case, fe)
            try:
                want[n] = call(s, old)
            finally:
                old.destroy()
                s.close()
        s = Setup(ctx, case, fe, lv=level(case))
        old = old_state(s, case, fe)
        try:
            for n in ("transient", "poisson", "transient", "form", "transient", "transient", "form", "poisson", "form", "transient"):
                assert same_bits(calls[n](s, old), want[n]), n
            check(s, reference(case, fe, "B", 0.5))
        finally:
            old.destroy()
            s.close()
    finally:
        qform.destroy()
        tform.destroy()


def test_refusals_leave_the_object_usable(ctx):
    from femus_amd import capi
    case, fe = "tri", "serendipity"
    s = Setup(ctx, case, fe, lv=level(case))
    form, old = device_form("A", 2), old_state(s, case, fe)
    wide = capi.Expr("u+t+w", "x,y,z,u,ux,uy,uz,t,w")
    bad_vars = capi.QuasilinearForm(c=wide)
    bad_dim = capi.TransientForm(c="u*(ux+uy)", c_u="ux+uy", c_g=["u", "u", "u"])
    short = ctx.vector(s.ndof + 3)
    call = lambda **kw: s.gen.assemble_transient(**{**dict(K=s.K, res=s.RES, sol=s.SOL, sol_old=old, form=form, time=TIME, dt=DT, theta=0.5), **kw})
    try:
        want = tr_bits(s, form, old)
        check(s, reference(case, fe, "A", 0.5))
        for match, kw in [("null form", dict(form=None)), ("null sol_old", dict(sol_old=None)), ("sol_old has", dict(sol_old=short)),
                          ("9 variables", dict(form=bad_vars)), (r"c_g\[2\] given on a mesh of dimension 2", dict(form=bad_dim)), ("not the matrix", dict(K=s.K2)),
                          ("not positive", dict(dt=0.0)), ("not positive", dict(dt=-DT)), ("outside", dict(theta=1.5)), ("outside", dict(theta=-0.1)),
                          ("finite", dict(time=float("nan"))), ("finite", dict(dt=float("inf"))), ("finite", dict(theta=float("nan")))]:
            with pytest.raises(capi.FemusHipError, match=match):
                call(**kw)
            assert same_bits(tr_bits(s, form, old), want), match
        with pytest.raises(capi.FemusHipError, match="8 variables"):       # the stationary call keeps its seven
            s.gen.assemble_form(s.K, s.RES, s.SOL, form)
        assert same_bits(tr_bits(s, form, old), want)
    finally:
        for q in (form, bad_vars, bad_dim, wide, old, short):
            q.destroy()
        s.close()
