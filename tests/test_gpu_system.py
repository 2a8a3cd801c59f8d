"""fh_generic_assembler_assemble_system (capi.GenericAssembler.assemble_system, femus_amd/csrc/fh_system.hip) and the block matrices Mat.block_system /
Mat.block_diagonal: Jacobian and residual of coupled systems of one family on triangles, tetrahedra, prisms and mixed meshes, against
tests/system_reference.py -- which tests/test_system_reference_host.py holds against the scalar restatement and against differences of its own residual.
Nothing here compares the kernel with itself but the repeatability and builder tests.

Meshes, state and bound are those of tests/test_gpu_quasilinear.py: test_gpu_generic_assembler.mesh refined once and curved; default_rng(11).uniform(-1, 1);
1e-12 of the restatement's largest entry.  Forms S (m = dim) and R (m = 4) of tests/system_reference.py: only + - * / and sqrt."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import quasilinear_reference as qr
import system_reference as sr
from test_gpu_generic_assembler import CASES, FES, RULES, Setup, bits, same_bits
from test_gpu_quasilinear import RULE_CASES, device_form, form_bits, host_setup, level

pytestmark = pytest.mark.gpu
FORMS = {"S": sr.form_s, "R": sr.form_r}


@functools.lru_cache(maxsize=None)
def reference(case, fe, name, order="seventh"):
    """(K, RES) of the restatement: computed once per case, shared, never changed"""
    kind, ed, xs, own = host_setup(case)
    form = FORMS[name](xs.shape[1])[1]
    u = np.random.default_rng(11).uniform(-1, 1, form["m"] * own[qr.FAM[fe]])
    K, F = sr.assemble(kind, ed, xs, fe, form, u, order=order)
    F.setflags(write=False)
    return K, F


class System:
    """a Setup (scalar pattern, object) with the block matrix, state and residual of m variables on it"""

    def __init__(self, ctx, case, fe, m, **kw):
        self.s = Setup(ctx, case, fe, lv=level(case), **kw)
        self.m, self.ndof, self.gen = m, self.s.ndof, self.s.gen
        self.K = self.s.K.block_system(m)
        self.u = np.random.default_rng(11).uniform(-1, 1, m * self.ndof)
        self.SOL, self.RES = ctx.vector_from(self.u), ctx.vector(m * self.ndof)

    def assemble(self, form, gen=None, K=None):
        (gen or self.gen).assemble_system(K or self.K, self.RES, self.SOL, form)
        return bits(K or self.K, self.RES)

    def check(self, ref):
        Kr, Fr = ref
        dK, dF = abs(self.K.to_scipy() - Kr).max(), np.abs(self.RES.to_numpy() - Fr).max()
        print("|K - restatement| = %.3e of %.3e, |RES - restatement| = %.3e of %.3e" % (dK, abs(Kr).max(), dF, np.abs(Fr).max()))
        assert dK <= 1e-12 * abs(Kr).max()
        assert dF <= 1e-12 * np.abs(Fr).max()

    def close(self):
        self.K.destroy()
        self.s.close()


def system_form(name, dim):
    from femus_amd import capi
    return capi.SystemForm(**FORMS[name](dim)[0])


# ---- the block matrices ----
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_block_matrices_against_scipy_kron(ctx, m):
    """a rectangular prolongator (with values) and a square pattern, through both calls: the integers are equal and the value bits are equal"""
    from femus_amd import capi
    rng = np.random.default_rng(5)
    P = sp.random(37, 11, density=0.3, random_state=3, format="csr")
    P.sort_indices()
    s = Setup(ctx, "mixed2d", "biquadratic", lv=level("mixed2d"))
    S = s.pat.copy()
    S.data = rng.uniform(-1, 1, S.nnz)
    s.K.set_values(S.data)
    dP = capi.Mat.from_csr(ctx, 37, 11, P.indptr, P.indices, P.data)
    made = []
    try:
        for A, dA in ((P, dP), (S, s.K)):
            for call, want in (("block_system", sp.kron(np.ones((m, m)), A, format="csr")), ("block_diagonal", sp.kron(sp.identity(m), A, format="csr"))):
                B = getattr(dA, call)(m)
                made.append(B)
                want.sort_indices()
                rp, col = B.pattern()
                assert (B.m(), B.n(), B.nnz) == (want.shape[0], want.shape[1], want.nnz)
                assert np.array_equal(rp, want.indptr) and np.array_equal(col, want.indices)
                assert all(np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0) for r in range(B.m()))
                if call == "block_system":
                    assert not B.values().any()
                else:
                    assert np.array_equal(B.values().view(np.uint64), want.data.view(np.uint64))
        # the block matrix is a matrix like any other: a product with it
        x = rng.uniform(-1, 1, 11 * m)
        X, Y = ctx.vector_from(x), ctx.vector(37 * m)
        Y.matrix_mult(X, made[1])
        assert np.abs(Y.to_numpy() - sp.kron(sp.identity(m), P) @ x).max() <= 1e-14 * 11
    finally:
        for B in made + [dP]:
            B.destroy()
        s.close()
    small = capi.Mat.from_csr(ctx, 2, 2, np.array([0, 1, 2]), np.array([0, 1]))
    try:
        with pytest.raises(capi.FemusHipError, match="fh_mat_block_system: 5 variables"):
            small.block_system(5)
        with pytest.raises(capi.FemusHipError, match="fh_mat_block_diagonal: 0 variables"):
            small.block_diagonal(0)
    finally:
        small.destroy()


# ---- the kernel ----
@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("case", CASES)
def test_form_s_against_the_restatement(ctx, case, fe):
    """K and RES within 1e-12 of the restatement's largest entry; the Jacobian is not its transpose and block (0, 1) is not block (1, 0) mirrored"""
    dim = level(case)[2].shape[1]
    q = System(ctx, case, fe, dim)
    form = system_form("S", dim)
    try:
        q.assemble(form)
        print(case, fe, "form S", q.gen.system_chunks(dim), end=": ")
        q.check(reference(case, fe, "S"))
        K, n = q.K.to_scipy(), q.ndof
        assert abs(K - K.T).max() > 1e-3 * abs(K).max()
        assert abs(K[:n, n:2 * n] - K[n:2 * n, :n].T).max() > 1e-3 * abs(K).max()
    finally:
        form.destroy()
        q.close()


@pytest.mark.parametrize("case,fe", [("tet", "biquadratic"), ("mixed3d", "linear")])
def test_form_r_against_the_restatement(ctx, case, fe):
    q = System(ctx, case, fe, 4)
    form = system_form("R", 3)
    try:
        q.assemble(form)
        print(case, fe, "form R", q.gen.system_chunks(4), end=": ")
        q.check(reference(case, fe, "R"))
    finally:
        form.destroy()
        q.close()


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("case,fe", RULE_CASES)
def test_every_gauss_rule_against_the_restatement(ctx, case, fe, order):
    """a last chunk that is not full among them"""
    dim = level(case)[2].shape[1]
    q = System(ctx, case, fe, dim, order=order)
    form = system_form("S", dim)
    try:
        q.assemble(form)
        print(case, fe, order, q.gen.system_chunks(dim), end=": ")
        q.check(reference(case, fe, "S", order))
    finally:
        form.destroy()
        q.close()


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("case,fe", [("tri", "biquadratic"), ("tet", "serendipity"), ("wedge", "linear"), ("mixed3d", "biquadratic")])
def test_one_variable_gives_the_values_of_assemble_form(ctx, case, fe, name):
    from femus_amd import capi
    q = System(ctx, case, fe, 1)
    dim = q.s.xs.shape[1]
    text = qr.with_source({"A": qr.form_a, "B": qr.form_b}[name](dim), dim)[0]
    scalar, form = capi.QuasilinearForm(**text), capi.SystemForm(**sr.scalar_texts([text]))
    try:
        form_bits(q.s, scalar)
        Kf, Ff = q.s.K.to_scipy().copy(), q.s.RES.to_numpy().copy()
        q.assemble(form)
        assert abs(q.K.to_scipy() - Kf).max() <= 1e-12 * abs(Kf).max()
        assert np.abs(q.RES.to_numpy() - Ff).max() <= 1e-12 * np.abs(Ff).max()
        q.s.K.zero()
        q.assemble(form, K=q.s.K)                                 # with one variable the object's own matrix serves as well
        assert abs(q.s.K.to_scipy() - Kf).max() <= 1e-12 * abs(Kf).max()
    finally:
        scalar.destroy()
        form.destroy()
        q.close()


@pytest.mark.parametrize("case,fe", [("tri", "biquadratic"), ("mixed3d", "serendipity")])
def test_two_scalar_forms_side_by_side(ctx, case, fe):
    """their two matrices in the diagonal blocks, stored zeros elsewhere"""
    from femus_amd import capi
    q = System(ctx, case, fe, 2)
    dim, n = q.s.xs.shape[1], q.ndof
    texts = [qr.with_source(qr.form_a(dim), dim)[0], qr.form_b(dim)[0]]
    form = capi.SystemForm(**sr.scalar_texts(texts))
    U = ctx.vector(n)
    try:
        q.assemble(form)
        K, F = q.K.to_scipy(), q.RES.to_numpy()
        assert K.nnz == 4 * q.s.K.nnz
        for k, text in enumerate(texts):
            scalar = capi.QuasilinearForm(**text)
            U.upload(q.u[k * n:(k + 1) * n])
            q.gen.assemble_form(q.s.K, q.s.RES, U, scalar)
            scalar.destroy()
            Kk, Fk = q.s.K.to_scipy(), q.s.RES.to_numpy()
            assert abs(K[k * n:(k + 1) * n, k * n:(k + 1) * n] - Kk).max() <= 1e-12 * abs(Kk).max()
            assert np.abs(F[k * n:(k + 1) * n] - Fk).max() <= 1e-12 * np.abs(Fk).max()
            off = K[k * n:(k + 1) * n, (1 - k) * n:(2 - k) * n]
            assert off.nnz == q.s.K.nnz and not off.data.any()
    finally:
        form.destroy()
        q.close()


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("case,fe,name", [("tet", "biquadratic", "S"), ("tet", "linear", "R"), ("mixed3d", "serendipity", "S"), ("tri", "linear", "S")])
def test_three_assemblies_give_the_same_bits_without_allocating(ctx, case, fe, name, poison):
    """also with debug_poison set before create: the work buffers start as 0xFF bytes, and the row pass must read nothing the element pass has not written"""
    before = int(os.environ.get("FEMUS_HIP_POISON", "0") or 0)
    ctx.set_option("debug_poison", 1 if poison else before)
    try:
        dim = level(case)[2].shape[1]
        m = 4 if name == "R" else dim
        q = System(ctx, case, fe, m)
        form = system_form(name, dim)
        try:
            n0 = q.gen.info()
            first = q.assemble(form)
            n1 = q.gen.info()
            assert n1["device_allocations"] == n0["device_allocations"] + 2                     # Kb and Fb of this m
            assert n1["device_bytes"] - n0["device_bytes"] >= (m * m - 1) * 8 * q.gen.plan()[2].size
            q.check(reference(case, fe, name))
            assert np.isfinite(q.RES.to_numpy()).all() and np.isfinite(q.K.to_scipy().data).all()
            assert same_bits(q.assemble(form), first) and same_bits(q.assemble(form), first)
            assert q.gen.info()["device_allocations"] == n1["device_allocations"]
            assert all(gc >= 1 and lanes in (16, 32, 64) for gc, lanes in q.gen.system_chunks().values())
            assert q.gen.system_chunks() == q.gen.system_chunks(m)
            assert m == 4 or all(gc == 0 for gc, _ in q.gen.system_chunks(4).values())           # no call with four variables yet
        finally:
            form.destroy()
            q.close()
    finally:
        ctx.set_option("debug_poison", before)


@pytest.mark.parametrize("case,fe", [("tet", "biquadratic"), ("mixed2d", "linear")])
def test_all_four_bodies_alternate_on_one_object(ctx, case, fe):
    """the program buffer is shared: each path still gives its own bits, whatever ran before it -- a system call after an assemble_form of the same programs
    included (the scalar form f, a = 1 and the system of one variable with f alone, whose missing A_00 is the constant 1: the directory is what differs)"""
    from femus_amd import capi
    dim = level(case)[2].shape[1]
    q = System(ctx, case, fe, dim)
    s = q.s
    sys_form = system_form("S", dim)
    text_f = qr.with_source(({}, {}), dim)[0]
    one = capi.SystemForm(1, f=[text_f["f"]])
    forms = {"A": device_form("A", dim), "f": capi.QuasilinearForm(f=text_f["f"], a="1")}
    tform = capi.TransientForm(**qr.with_source(qr.form_b(dim), dim)[0])
    OLD = ctx.vector_from(0.5 * s.u)

    def transient():
        s.gen.assemble_transient(s.K, s.RES, s.SOL, OLD, tform, 0.25, 0.125, 0.5)
        return bits(s.K, s.RES)

    def single():
        s.gen.assemble_system(s.K, s.RES, s.SOL, one)
        return bits(s.K, s.RES)

    try:
        want_sys = q.assemble(sys_form)
        q.check(reference(case, fe, "S"))
        want = {"poisson": s.resident(), "A": form_bits(s, forms["A"]), "f": form_bits(s, forms["f"]), "transient": transient(), "one": single()}
        calls = {"poisson": s.resident, "A": lambda: form_bits(s, forms["A"]), "f": lambda: form_bits(s, forms["f"]), "transient": transient, "one": single}
        for n in ("f", "one", "f", "A", "transient", "poisson", "one", "transient", "A"):
            assert same_bits(q.assemble(sys_form), want_sys), n
            assert same_bits(calls[n](), want[n]), n
        for a, b in (("f", "one"), ("one", "f"), ("A", "transient")):
            calls[a]()
            assert same_bits(calls[b](), want[b]), (a, b)
        assert same_bits(q.assemble(sys_form), want_sys)
        q.check(reference(case, fe, "S"))
    finally:
        for f in list(forms.values()) + [tform, sys_form, one]:
            f.destroy()
        q.close()


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
    form = system_form("S", dim)
    K, K2 = s.K.block_system(dim), s.K2.block_system(dim)
    SOL, RES = ctx.vector_from(np.random.default_rng(11).uniform(-1, 1, dim * s.ndof)), ctx.vector(dim * s.ndof)
    try:
        s.gen.assemble_system(K, RES, SOL, form)
        a = bits(K, RES)
        gd.assemble_system(K2, RES, SOL, form)
        assert same_bits(a, bits(K2, RES))
    finally:
        gd.destroy()
        form.destroy()
        K.destroy()
        K2.destroy()
        s.close()


def test_three_variables_after_two_on_one_object(ctx):
    """every m has work buffers and a launch geometry of its own on the one object"""
    from femus_amd import capi
    case, fe = "tet", "serendipity"
    q3 = System(ctx, case, fe, 3)
    K2 = q3.s.K.block_system(2)
    n = q3.ndof
    texts = [qr.with_source(qr.form_a(3), 3)[0], qr.form_b(3)[0]]
    two, three = capi.SystemForm(**sr.scalar_texts(texts)), system_form("S", 3)
    RES2 = ctx.vector(2 * n)
    try:
        q3.gen.assemble_system(K2, RES2, q3.SOL, two)
        first2 = bits(K2, RES2)
        a0 = q3.gen.info()["device_allocations"]
        first3 = q3.assemble(three)
        assert q3.gen.info()["device_allocations"] == a0 + 2
        q3.check(reference(case, fe, "S"))
        q3.gen.assemble_system(K2, RES2, q3.SOL, two)
        assert same_bits(bits(K2, RES2), first2)
        assert same_bits(q3.assemble(three), first3)
        assert q3.gen.info()["device_allocations"] == a0 + 2
        Kr, Fr = sr.assemble(*host_setup(case)[:3], fe, sr.from_scalar([qr.with_source(qr.form_a(3), 3)[1], qr.form_b(3)[1]]), q3.u[:2 * n])
        assert abs(K2.to_scipy() - Kr).max() <= 1e-12 * abs(Kr).max()
        assert np.abs(RES2.to_numpy() - Fr).max() <= 1e-12 * np.abs(Fr).max()
    finally:
        two.destroy()
        three.destroy()
        K2.destroy()
        q3.close()


def test_refusals_leave_the_matrix_values_as_they_were(ctx):
    from femus_amd import capi
    q = System(ctx, "tri", "serendipity", 2)
    n = q.ndof
    form = system_form("S", 2)
    wide = capi.Expr("u0+w", capi.SystemForm.variables(2) + ",w")
    bad_vars = capi.SystemForm(2)
    bad_vars.exprs[("c", (1,))] = wide                            # past the constructor's own check
    bad_vars._refresh()
    bad_dim = capi.SystemForm(2, c_g=[[None, ["u0", "u0", "u0"]], [None, None]])
    five = capi.SystemForm(2)
    five._s.m = 5
    K3, short = q.s.K.block_system(3), ctx.vector(2 * n - 1)
    who = "fh_generic_assembler_assemble_system"
    try:
        want = q.assemble(form)
        q.check(reference("tri", "serendipity", "S"))
        refused = [(bad_vars, q.K, q.RES, q.SOL, who + ": the program c\\[1\\] has 12 variables, at most 11"),
                   (bad_dim, q.K, q.RES, q.SOL, who + r": c_g\[0\]\[1\]\[2\] given on a mesh of dimension 2"),
                   (five, q.K, q.RES, q.SOL, who + ": 5 variables"),
                   (None, q.K, q.RES, q.SOL, who + ": null form"),
                   (form, K3, q.RES, q.SOL, who + ": not the block system of 2 variables"),
                   (form, q.s.K, q.RES, q.SOL, who + ": not the block system of 2 variables"),
                   (form, q.K, short, q.SOL, who + ": size mismatch"),
                   (form, q.K, q.RES, short, who + ": size mismatch")]
        for f, K, RES, SOL, message in refused:
            with pytest.raises(capi.FemusHipError, match=message):
                q.gen.assemble_system(K, RES, SOL, f)
            assert same_bits(bits(q.K, q.RES), want), message
        assert not K3.values().any()
        assert same_bits(q.assemble(form), want)
    finally:
        for f in (form, bad_vars, bad_dim, five, wide):
            f.destroy()
        K3.destroy()
        q.close()
