"""fh_generic_assembler_assemble_form (capi.GenericAssembler.assemble_form, femus_amd/csrc/fh_quasilinear.hip): Jacobian and residual of a quasilinear scalar
equation on triangles, tetrahedra, prisms and mixed meshes, against tests/quasilinear_reference.py -- whose Jacobian tests/test_quasilinear_reference_host.py
checks against differences of its residual.  Nothing here compares the kernel with itself but the repeatability and builder tests.

Meshes: those of test_gpu_generic_assembler.mesh, refined once and curved (48 triangles, 840 tetrahedra, 128 prisms, the two mixed files): two and four elements
per wave, a last workgroup that is not full, all three launch widths, three shapes in one call.
Form A (ex03):  c = u (ux + uy [+ uz]), c_u = ux + uy [+ uz], c_g = (u, u [, u]).   Form B (ex03b plus a reaction): a = 1 + u^2, a_u = 2 u, c = sqrt(1 + u^2),
c_u = u / sqrt(1 + u^2): only + - * / and sqrt, so host and device agree to rounding.  f = exp(x) (1 + y) [- z]; the state is default_rng(11).uniform(-1, 1)."""
import functools
import os

import numpy as np
import pytest

import quasilinear_reference as qr
from test_gpu_generic_assembler import CASES, FES, RULES, Setup, bits, mesh, same_bits

pytestmark = pytest.mark.gpu
FORMS = {"A": qr.form_a, "B": qr.form_b}
RULE_CASES = [("tri", "biquadratic"), ("tet", "serendipity"), ("wedge", "biquadratic"), ("mixed3d", "linear"), ("mixed2d", "serendipity")]


@functools.lru_cache(maxsize=None)
def level(case):
    return mesh(case)


@functools.lru_cache(maxsize=None)
def reference(case, fe, name, order="seventh"):
    """(K, RES) of the restatement: computed once per case, shared, never changed"""
    s = host_setup(case)
    dim = s[2].shape[1]
    pair = qr.with_source(FORMS[name](dim) if name != "f" else ({}, {}), dim)
    u = np.random.default_rng(11).uniform(-1, 1, s[3][qr.FAM[fe]])
    K, F = qr.assemble(s[0], s[1], s[2], fe, pair[1], u, order=order)
    F.setflags(write=False)
    return K, F


@functools.lru_cache(maxsize=None)
def host_setup(case):
    from test_gpu_generic_assembler import curved
    kind, ed, xs, own = level(case)
    return kind, ed, curved(xs), own


def device_form(name, dim):
    from femus_amd import capi
    text = qr.with_source(FORMS[name](dim) if name != "f" else ({}, {}), dim)[0]
    return capi.QuasilinearForm(**text)


def check(s, ref):
    Kr, Fr = ref
    dK, dF = abs(s.K.to_scipy() - Kr).max(), np.abs(s.RES.to_numpy() - Fr).max()
    print("|K - restatement| = %.3e of %.3e, |RES - restatement| = %.3e of %.3e" % (dK, abs(Kr).max(), dF, np.abs(Fr).max()))
    assert dK <= 1e-12 * abs(Kr).max()
    assert dF <= 1e-12 * np.abs(Fr).max()


def form_bits(s, form, gen=None, K=None):
    (gen or s.gen).assemble_form(K or s.K, s.RES, s.SOL, form)
    return bits(K or s.K, s.RES)


@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("case", CASES)
def test_values_against_the_restatement_and_the_poisson_limit(ctx, case, fe):
    """both forms: K and RES within 1e-12 of the restatement's largest entry; form A's K is not its transpose (a symmetrised kernel cannot pass); with f alone
    the result is GenericAssembler.assemble's, to the same bound"""
    s = Setup(ctx, case, fe, lv=level(case))
    dim = s.xs.shape[1]
    forms = {n: device_form(n, dim) for n in ("A", "B", "f")}
    try:
        for name in ("A", "B"):
            form_bits(s, forms[name])
            print(case, fe, "form", name, end=": ")
            check(s, reference(case, fe, name))
            if name == "A":
                K = s.K.to_scipy()
                assert abs(K - K.T).max() > 1e-3 * abs(K).max()
        form_bits(s, forms["f"])
        Kf, Ff = s.K.to_scipy().copy(), s.RES.to_numpy().copy()
        s.gen.assemble(s.K, s.RES, sol=s.SOL, source=s.f)
        Kp, Fp = s.K.to_scipy(), s.RES.to_numpy()
        assert abs(Kf - Kp).max() <= 1e-12 * abs(Kp).max()
        assert np.abs(Ff - Fp).max() <= 1e-12 * np.abs(Fp).max()
    finally:
        for f in forms.values():
            f.destroy()
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
    try:
        for name, form in forms.items():
            assert same_bits(form_bits(s, form), form_bits(s, form, gen=gd, K=s.K2))
    finally:
        gd.destroy()
        for f in forms.values():
            f.destroy()
        s.close()


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("case,fe", RULE_CASES)
def test_every_gauss_rule_against_the_restatement(ctx, case, fe, order):
    s = Setup(ctx, case, fe, order=order, lv=level(case))
    name = "A" if order in ("first", "fifth", "ninth") else "B"
    form = device_form(name, s.xs.shape[1])
    try:
        form_bits(s, form)
        check(s, reference(case, fe, name, order))
    finally:
        form.destroy()
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
    form = device_form("B", s.xs.shape[1])
    try:
        first = form_bits(s, form)
        n1 = s.gen.info()["device_allocations"]
        check(s, reference(case, fe, "B"))
        assert np.isfinite(s.RES.to_numpy()).all() and np.isfinite(s.K.to_scipy().data).all()
        assert same_bits(form_bits(s, form), first) and same_bits(form_bits(s, form), first)
        assert s.gen.info()["device_allocations"] == n1
        assert all(v >= 1 for v in s.gen.form_chunks().values())
    finally:
        form.destroy()
        s.close()


@pytest.mark.parametrize("case,fe", [("tet", "biquadratic"), ("mixed2d", "linear")])
def test_poisson_and_form_assemblies_alternate_on_one_object(ctx, case, fe):
    """the program buffer and the work buffers are shared: each path still gives its own bits, whatever ran before it"""
    s = Setup(ctx, case, fe, lv=level(case))
    dim = s.xs.shape[1]
    forms = {n: device_form(n, dim) for n in ("A", "B", "f")}
    try:
        poisson = s.resident()
        assert same_bits(poisson, s.reference())
        want = {n: form_bits(s, forms[n]) for n in forms}
        check_form = lambda n: same_bits(form_bits(s, forms[n]), want[n])
        for n in ("B", "f", "A", "f", "B"):
            assert same_bits(s.resident(), poisson)
            assert check_form(n)
        assert check_form("A") and check_form("B") and same_bits(s.resident(), poisson)
        form_bits(s, forms["A"])
        check(s, reference(case, fe, "A"))
    finally:
        for f in forms.values():
            f.destroy()
        s.close()


def test_refusals_leave_the_object_usable(ctx):
    from femus_amd import capi
    s = Setup(ctx, "tri", "serendipity", lv=level("tri"))
    form = device_form("A", 2)
    wide = capi.Expr("u+w", "x,y,z,u,ux,uy,uz,w")
    bad_vars = capi.QuasilinearForm(c=wide)
    bad_dim = capi.QuasilinearForm(c="u*(ux+uy)", c_u="ux+uy", c_g=["u", "u", "u"])
    try:
        want = form_bits(s, form)
        check(s, reference("tri", "serendipity", "A"))
        with pytest.raises(capi.FemusHipError, match="8 variables"):
            s.gen.assemble_form(s.K, s.RES, s.SOL, bad_vars)
        assert same_bits(form_bits(s, form), want)
        with pytest.raises(capi.FemusHipError, match=r"c_g\[2\] given on a mesh of dimension 2"):
            s.gen.assemble_form(s.K, s.RES, s.SOL, bad_dim)
        assert same_bits(form_bits(s, form), want)
        with pytest.raises(capi.FemusHipError, match="not the matrix"):
            s.gen.assemble_form(s.K2, s.RES, s.SOL, form)
        assert same_bits(form_bits(s, form), want)
    finally:
        for q in (form, bad_vars, bad_dim, wide):
            q.destroy()
        s.close()
