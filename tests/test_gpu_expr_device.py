"""The DEVICE compilation of the run-time expression evaluator (fh_expr_device_eval under hipcc, inside nine kernels), operator by operator.

a. every operator and function through capi.Expr.eval_device against tests/golden/expr_vectors.npz (mpmath at 60 digits, rounded once; made by
   tests/golden/make_expr_vectors.py): the fixture's bits for what IEEE 754 rounds correctly or what is exact, an ulp bound for the transcendental
   functions; special arguments by class.
c. a full evaluation stack, a long program, and an if() whose dead branch is not finite.
d. every kernel that takes a program, on its smallest mesh, against the oracle's quadrature of a Python callable for a text that uses if, comparisons, &,
   atan2, pow, max, hypot and %.
e. the Neumann kernel's table of concatenated programs; f. the program caches; g. expressions the kernels must refuse.

ULP BOUNDS.  No accuracy table of the device math library is installed beside the compiler (only its bitcode), so the bounds are those of the OpenCL C
specification, "Relative error as ULPs", double precision, full profile -- the table that library is built to meet: exp, exp2, log, log2, log10 3;
sin, cos, sinh, cosh, asin, acos, asinh, acosh, hypot 4; tan, tanh, atan, atanh 5; atan2 6; cbrt 2; pow 16.  cot, sec and csc are 1 / tan, 1 / cos,
1 / sin: the function's bound plus 1 for the division.  The error is measured in spacings of doubles at the fixture's value; the largest per function is
printed (DESIGN.md section 5 keeps the figures of the first run)."""
import numpy as np
import pytest

import expr_fixture as fx
import test_gpu_gauss_rules as tgr
import test_gpu_generic_assembler as tga
from femus_amd import capi
from oracle import femus_oracle as fo
from oracle import femus_oracle_1d as o1
from oracle import femus_oracle_mixed as om
from oracle import femus_oracle_tet as oq
from oracle import femus_oracle_tri as ot
from oracle import femus_oracle_wedge as ow

pytestmark = pytest.mark.gpu

ULP_BOUND = {"exp(x)": 3, "exp2(x)": 3, "log(x)": 3, "log2(x)": 3, "log10(x)": 3, "sin(x)": 4, "cos(x)": 4, "sinh(x)": 4, "cosh(x)": 4, "asin(x)": 4,
             "acos(x)": 4, "asinh(x)": 4, "acosh(x)": 4, "hypot(x,y)": 4, "tan(x)": 5, "tanh(x)": 5, "atan(x)": 5, "atanh(x)": 5, "atan2(x,y)": 6,
             "cbrt(x)": 2, "pow(x,y)": 16, "x^y": 16, "cot(x)": 5 + 1, "sec(x)": 4 + 1, "csc(x)": 4 + 1}
assert sorted(ULP_BOUND) == sorted(fx.INEXACT)


# ---- a. operator by operator ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("text", fx.EXACT)
def test_exact_operations_give_the_fixture_s_bits(ctx, text):
    x, want = fx.vectors(text)
    e = capi.Expr(text, fx.VARIABLES)
    try:
        got = e.eval_device(ctx, x)
    finally:
        e.destroy()
    bad = ~fx.same_bits(got, want)
    assert not bad.any(), (text, x[bad][:4], got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("text", fx.INEXACT)
def test_transcendental_functions_within_their_ulp_bound(ctx, text):
    x, want = fx.vectors(text)
    e = capi.Expr(text, fx.VARIABLES)
    try:
        got = e.eval_device(ctx, x)
    finally:
        e.destroy()
    err = fx.ulps(got, want)
    k = int(np.argmax(err))
    print("ULP %-11s largest error %.3f ulp (bound %d) at %s: device %.17g, fixture %.17g" % (text, err[k], ULP_BOUND[text], x[k, :2], got[k], want[k]))
    assert err[k] <= ULP_BOUND[text], (text, err[k], x[k], got[k], want[k])


@pytest.mark.parametrize("text", fx.SPECIAL_TEXTS)
def test_special_arguments_give_the_class_numpy_gives(ctx, text):
    """zeros, infinities, NaN, 1e308 and 5e-324: NaN, +inf, -inf or a finite value as numpy on the CPU has it (signs of zero are not compared)"""
    x, cls = fx.special_vectors(text)
    e = capi.Expr(text, fx.VARIABLES)
    try:
        got = e.eval_device(ctx, x)
    finally:
        e.destroy()
    bad = fx.classes(got) != cls
    assert not bad.any(), (text, x[bad], got[bad], cls[bad])


# ---- c. stack, length, laziness ---------------------------------------------------------------------------------------------------------------------

PTS64 = np.random.default_rng(64).uniform(0.0, 1.0, (64, 4))


def nested(depth):
    """x+(y*(x+(y*(... v))): every open bracket keeps one operand waiting, so the program needs depth + 1 stack slots"""
    text, py = "x", lambda x, y: x
    for k in range(depth):
        if k % 2 == 0:
            text, py = "y*(%s)" % text, (lambda x, y, inner=py: y * inner(x, y))
        else:
            text, py = "x+(%s)" % text, (lambda x, y, inner=py: x + inner(x, y))
    return text, py


def test_a_full_stack_of_16_slots_and_the_refusal_of_17(ctx):
    text, py = nested(15)
    e = capi.Expr(text, "x,y,z,t")
    try:
        got = e.eval_device(ctx, PTS64)
        want = np.array([py(p[0], p[1]) for p in PTS64])
        assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()
        assert np.array_equal(got, e(PTS64))                                # plain arithmetic: the host compilation gives the same bits
    finally:
        e.destroy()
    with pytest.raises(capi.FemusHipError, match=r"needs an evaluation stack of 17 \(limit 16\)"):
        capi.Expr(nested(16)[0], "x,y,z,t")


def long_polynomial():
    """120 terms c*u*v with irregular coefficients and u, v running through the variables: 6 program words a term, a stack of 3"""
    coef = np.random.default_rng(7).uniform(0.1, 1.5, 120).round(6)
    sign = np.random.default_rng(8).choice(["+", "-"], 120)
    return "0.5" + "".join(" %s %r*%s*%s" % (s, float(c), "xyzt"[k % 4], "yztx"[k % 3]) for k, (c, s) in enumerate(zip(coef, sign)))


def test_a_program_of_more_than_500_words_with_more_than_100_constants(ctx):
    text = long_polynomial()
    e = capi.Expr(text, "x,y,z,t")
    try:
        code, consts = e.program()
        assert code.size >= 500 and np.unique(consts).size >= 100
        got = e.eval_device(ctx, PTS64)
        want = np.array([eval(text, {"x": p[0], "y": p[1], "z": p[2], "t": p[3]}) for p in PTS64])      # the grammars agree on + - * and numbers
        assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()
    finally:
        e.destroy()


def test_if_selects_and_does_not_multiply_by_a_mask(ctx):
    """log(x - 0.5) is NaN or -inf wherever x <= 0.5: the value there must be the other branch, exactly"""
    pts = PTS64.copy()
    pts[:4, 0] = [0.5, 0.0, 0.25, 0.499]
    e = capi.Expr("if(x>0.5, log(x-0.5), 0)", "x,y,z,t")
    try:
        got = e.eval_device(ctx, pts)
    finally:
        e.destroy()
    x = pts[:, 0]
    assert (x <= 0.5).sum() >= 4 and (x > 0.5).sum() >= 4
    assert np.all(np.isfinite(got)) and np.all(got[x <= 0.5] == 0.0)
    want = np.log(x[x > 0.5] - 0.5)
    assert np.abs(got[x > 0.5] - want).max() <= 1e-15 * np.abs(want).max()


# ---- d. every kernel that takes a program -------------------------------------------------------------------------------------------------------------

TEXT = "if(x<0.4 & y>=0.3, 2+atan2(y,1+x), -pow(1.5,x)*max(y,0.2)) + hypot(x,y)%0.37"
SUFFIX = {1: " + 100*z + 1000*t", 2: " + 100*z + 1000*t", 3: " + 1000*t"}          # coordinates the mesh does not have, and t, read as 0
SHIFTS = [(1e-9, 1e-9), (-1e-9, -1e-9), (1e-9, -1e-9), (-1e-9, 1e-9)]


def f2(x, y):
    """TEXT in numpy"""
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    return np.where((x < 0.4) & (y >= 0.3), 2 + np.arctan2(y, 1 + x), -np.power(1.5, x) * np.maximum(y, 0.2)) + np.fmod(np.hypot(x, y), 0.37)


def at_point(dx=0.0, dy=0.0):
    """TEXT for the oracles that hand over one point p[d] (or arrays p[d][...])"""
    return lambda p: f2(p[0] + dx, (p[1] if len(p) > 1 else 0.0) + dy)


def at_xg(dx=0.0, dy=0.0):
    """TEXT for the tensor-product oracle's Gauss points xg[..., d]"""
    return lambda xg: f2(xg[..., 0] + dx, xg[..., 1] + dy)


def compare(ref_of, run, dim, name):
    """ref_of(dx, dy): the oracle's RES for TEXT with every Gauss point moved by (dx, dy); run(text): the device's RES.  Rows the oracle alone does not
    hold still on when its Gauss points move by 1e-9 have a jump of TEXT at a Gauss point: they are left out (at most 10 %), the others meet 1e-12 of
    the largest entry.  Then the missing coordinates and t must read as zero: the same bits with SUFFIX appended."""
    ref = np.asarray(ref_of(0.0, 0.0))
    scale = np.abs(ref).max()
    stable = np.ones(ref.size, bool)
    for dx, dy in SHIFTS:
        stable &= np.abs(np.asarray(ref_of(dx, dy)) - ref) <= 1e-6 * scale       # smooth change: 1e-9 |grad f|; a jump at one Gauss point: 1e-3 and more
    got = run(TEXT)[:ref.size]
    err = np.abs(got - ref)[stable].max() / scale
    print("EXPR %-28s |RES - oracle| = %.2e of the largest entry, %d of %d rows left out" % (name, err, (~stable).sum(), ref.size))
    assert (~stable).mean() <= 0.10
    assert scale > 1e-3 and err <= 1e-12, (name, err)
    again = run(TEXT + SUFFIX[dim])[:ref.size]
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64)), name


TENSOR = {
    "quad4x4-Q1-two-pass": dict(args=(4, 4, 0), fe="linear", order="seventh", refine=False, opts={}, path="two-pass"),
    "hex2x2x2-Q2-fifth-two-pass": dict(args=(2, 2, 2), fe="biquadratic", order="fifth", refine=False, opts={}, path="two-pass"),
    "hex-Q2-sum-factorised": dict(args=(2, 2, 2), fe="biquadratic", order="seventh", refine=True, opts={"assemble_fused": 0}, path="two-pass"),
    "hex-Q2-fused-cluster": dict(args=(2, 2, 2), fe="biquadratic", order="seventh", refine=True, opts={}, path="fused"),
    "hex-Q2-affine": dict(args=(2, 2, 2), fe="biquadratic", order="seventh", refine=True, opts={"assemble_affine": 1}, path="two-pass", flat=True),
    "hex-Q2-matrix-core": dict(args=(2, 2, 2), fe="biquadratic", order="seventh", refine=True, opts={}, late={"assemble_sf": 0}, path="two-pass"),
    "hex-Q2-fifth-tile": dict(args=(2, 2, 2), fe="biquadratic", order="fifth", refine=False, opts={"assemble_sym": 0}, path="two-pass"),
    "quad-Q2-emap-scatter": dict(args=(3, 2, 0), fe="biquadratic", order="seventh", refine=True, opts={"assemble_two_pass": 0}, path=None),
    "quad-Q2-search-scatter": dict(args=(3, 2, 0), fe="biquadratic", order="seventh", refine=True, opts={"assemble_two_pass": 0, "assemble_emap": 0}, path=None),
}
TENSOR_DEFAULTS = dict(tgr.DEFAULTS, assemble_fused=1, assemble_sf=8)


class Tensor:
    """a box mesh of the tensor-product assembler (curved inside unless flat), its oracle mesh, a matrix and the assembler under an option set"""

    def __init__(self, ctx, args, fe, order="seventh", refine=False, opts=None, flat=False, late=None, **_):
        self.ctx, self.fe, self.order = ctx, fe, order
        self.m = capi.Mesh.box(*args).refine() if refine else capi.Mesh.box(*args)
        self.mo = fo.build_levels(*args, 2 if refine else 1)[-1]
        ed, xy0, _ = self.m.arrays()
        assert np.array_equal(ed, self.mo.elem_dof)
        self.xy = xy0 if flat else tgr.bend(xy0)
        self.mo.coords = self.xy
        geom = "hex" if self.m.dim == 3 else "quad"
        self.n = fo.n_dofs(self.mo, fe)
        self.ed, self.nc = ed, fo.ndofs(geom, fe)
        self.A, self.res = tgr.pattern(ctx, ed, self.nc, self.n), ctx.vector(self.n)
        self.opts = opts or {}
        self.asm = None
        for k, v in self.opts.items():
            ctx.set_option(k, v)
        self.asm = self.assembler()
        for k, v in (late or {}).items():                      # options the dispatch reads at every assembly
            ctx.set_option(k, v)

    def assembler(self):
        return capi.Assembler(self.ctx, self.m, self.fe, self.A, order=self.order, elem_dof=self.ed, coords=self.xy)

    def run(self, text, asm=None):
        e = capi.Expr(text, "x,y,z,t")
        try:
            (asm or self.asm).assemble_expr(self.A, self.res, None, e)
        finally:
            e.destroy()
        return self.res.to_numpy().copy()

    def reference(self, dx=0.0, dy=0.0):
        return fo.assemble_poisson(self.mo, self.fe, at_xg(dx, dy), order=self.order)[1]

    def close(self):
        for k, v in TENSOR_DEFAULTS.items():
            self.ctx.set_option(k, v)
        if self.asm is not None:
            self.asm.destroy()
        self.A.destroy(), self.res.destroy(), self.m.destroy()


@pytest.mark.parametrize("case", list(TENSOR))
def test_tensor_product_assembler_kernels(ctx, case):
    c = TENSOR[case]
    s = Tensor(ctx, **c)
    try:
        if case == "hex-Q2-fused-cluster":
            assert s.asm.fused_info()["active"]
        if case == "hex-Q2-affine":
            assert s.asm.affine_count()[0] == s.m.nel
        compare(s.reference, s.run, s.m.dim, case)
        if c["path"] is not None:
            assert s.asm.last_path() == c["path"]
    finally:
        s.close()


def simplex_mesh(case):
    """the smallest meshes of the generic kernels: tri_box(3, 2), cube_Tet.neu, cube_Wedge.neu, square_mixed.neu as read, curved inside"""
    kind, ed_full, xs, own = tga.mesh(case, refinements=0)
    return kind, ed_full, tga.curved(xs), own


class Generic:
    def __init__(self, ctx, case, fe="biquadratic"):
        self.ctx, self.case, self.fe = ctx, case, fe
        self.kind, self.ed_full, self.xs, own = simplex_mesh(case)
        self.ndof = own[tga.FAM[fe]]
        self.geom, self.ed = tga.args_of(self.kind, self.ed_full)
        self.K, _ = tga.pattern(ctx, self.kind, self.ed_full, fe, self.ndof)
        self.K2, _ = tga.pattern(ctx, self.kind, self.ed_full, fe, self.ndof)
        self.RES, self.RES2 = ctx.vector(self.ndof), ctx.vector(self.ndof)
        self.gen = capi.GenericAssembler(ctx, self.geom, fe, self.ed, self.xs, self.K)

    def one_shot(self, text, variables="x,y,z,t"):
        e = capi.Expr(text, variables)
        try:
            tga.one_shot(self.ctx, self.geom, self.fe, self.ed, self.xs, self.K2, self.RES2, source=e)
        finally:
            e.destroy()
        return self.RES2.to_numpy().copy()

    def resident(self, text, gen=None, variables="x,y,z,t"):
        e = capi.Expr(text, variables)
        try:
            (gen or self.gen).assemble(self.K, self.RES, source=e)
        finally:
            e.destroy()
        return self.RES.to_numpy().copy()

    def reference(self, dx=0.0, dy=0.0):
        src = at_point(dx, dy)
        if self.case == "mixed2d":
            return om.assemble(self.kind, self.ed_full, self.xs, self.fe, src)[1] if (dx, dy) == (0.0, 0.0) else \
                om.assemble_batched(self.kind, self.ed_full, self.xs, self.fe, src)[1]
        if (dx, dy) != (0.0, 0.0):                                          # the batched oracle (the same sums, vectorised) for the moved points
            return om.assemble_batched(self.kind, self.ed_full, self.xs, self.fe, src)[1]
        return {"tri": ot, "tet": oq, "wedge": ow}[self.case].assemble(self.ed, self.xs, self.fe, src)[1]

    def close(self):
        self.gen.destroy()
        for o in (self.K, self.K2, self.RES, self.RES2):
            o.destroy()


@pytest.mark.parametrize("case", ["tri", "tet", "wedge", "mixed2d"])
def test_generic_kernels_one_shot_and_resident(ctx, case):
    """assemble_poisson_rows / assemble_poisson_mixed against the oracle's loop; GenericAssembler gives the one-shot call's bits"""
    s = Generic(ctx, case)
    try:
        compare(s.reference, s.one_shot, s.xs.shape[1], case + " one-shot")
        for text in (TEXT, TEXT + SUFFIX[s.xs.shape[1]]):
            assert np.array_equal(s.resident(text).view(np.uint64), s.one_shot(text).view(np.uint64))
    finally:
        s.close()


class Line:
    """eight EDGE3 elements, unevenly spaced"""
    NU, V = 0.01, 1.0

    def __init__(self, ctx):
        self.ctx = ctx
        self.ed, xs, _, _ = o1.box_mesh(8, -0.3, 1.7)
        self.xs = xs + 0.02 * np.sin(3.0 * xs)
        self.ndof = self.xs.size
        self.K, self.RES = tgr.pattern(ctx, self.ed, 3, self.ndof), ctx.vector(self.ndof)

    def run(self, text, variables="x,y,z,t"):
        e = capi.Expr(text, variables)
        try:
            capi.assemble_advdiff_line(self.ctx, "biquadratic", self.ed, self.xs, self.K, self.RES, self.NU, self.V, source=e)
        finally:
            e.destroy()
        return self.RES.to_numpy().copy()

    def reference(self, dx=0.0, dy=0.0):
        return o1.assemble(self.ed, self.xs, "biquadratic", np.zeros(self.ndof), lambda x: f2(x + dx, 0.0), self.NU, self.V)[1]

    def close(self):
        self.K.destroy(), self.RES.destroy()


def test_line_advection_diffusion_kernel(ctx):
    s = Line(ctx)
    try:
        compare(s.reference, s.run, 1, "line, eight EDGE3")
    finally:
        s.close()


class Faces:
    """the flagged boundary faces of a refined box with curved faces, as explicit lists for fh_assemble_neumann_faces_expr"""

    def __init__(self, ctx, args, fe="biquadratic"):
        self.ctx, self.fe = ctx, fe
        self.m = capi.Mesh.box(*args).refine()
        self.mo = fo.build_levels(*args, 2)[-1]
        ed, xy, ff = self.m.arrays()
        self.xy = xy + np.random.default_rng(5).uniform(-0.01, 0.01, xy.shape)
        self.mo.coords = self.xy
        self.dim = self.m.dim
        self.flags = sorted(set(ff[ff < -1].tolist()), reverse=True)
        fn, fl = [], []
        for f in range(self.m.nfaces):
            loc = capi.fe_face_nodes(self.m.geom, fe, f)
            for flag in self.flags:
                els = np.where(ff[:, f] == flag)[0]
                fn.append(ed[els][:, loc])
                fl.append(np.full(els.size, flag))
        self.fn, self.fl = np.concatenate(fn), np.concatenate(fl)
        self.res = ctx.vector(self.m.nnode)

    def run(self, texts_by_flag, order_of_exprs=None, shuffle=None, variables="x,y,z,t"):
        """the faces of flag f carry expression texts_by_flag[f]; order_of_exprs: the order of the expression list; shuffle: a permutation of the faces"""
        flags = list(texts_by_flag) if order_of_exprs is None else order_of_exprs
        sel = np.isin(self.fl, flags)
        fn, fx_ = self.fn[sel], np.array([flags.index(f) for f in self.fl[sel]])
        if shuffle is not None:
            p = np.random.default_rng(shuffle).permutation(fn.shape[0])
            fn, fx_ = fn[p], fx_[p]
        exprs = [capi.Expr(texts_by_flag[f], variables) for f in flags]
        try:
            self.res.fill(0.0)
            if self.dim == 2:
                capi.assemble_neumann_edges(self.ctx, self.fe, fn, fx_, exprs, self.xy, self.res)
            else:
                capi.assemble_neumann_faces_expr(self.ctx, "hex", self.fe, fn, fx_, exprs, self.xy, self.res)
        finally:
            for e in exprs:
                e.destroy()
        return self.res.to_numpy().copy()

    def close(self):
        self.res.destroy(), self.m.destroy()


@pytest.mark.parametrize("args", [(4, 3, 0), (2, 2, 2)])
def test_neumann_kernel(ctx, args):
    s = Faces(ctx, args)
    try:
        flags = s.flags[:2]
        compare(lambda dx, dy: fo.neumann_rhs(s.mo, s.fe, {f: at_point(dx, dy) for f in flags}),
                lambda text: s.run({f: text for f in flags}), s.dim, "neumann %dD" % s.dim)
    finally:
        s.close()


# ---- e. the Neumann program table -------------------------------------------------------------------------------------------------------------------

def test_neumann_table_of_six_programs(ctx):
    """six expressions in one call, one per side of the cube, of 1, 1, 3, 5, 9 and 23 words: `x` has no constants (two equal const_ptr entries), a bare
    constant is one word as well; faces in shuffled order; then the expression list permuted with face_expr remapped: identical bits"""
    s = Faces(ctx, (2, 2, 2))
    try:
        assert len(s.flags) == 6
        table = [("x", lambda p: p[0]),
                 ("0.75", lambda p: 0.75),
                 ("exp(-x)*(y<0.5)+2", lambda p: np.exp(-p[0]) * (1.0 if p[1] < 0.5 else 0.0) + 2),
                 ("y*z", lambda p: p[1] * p[2]),
                 ("0.2+x*y-sin(3*z)+t+cos(2*x)*1.5-0.25*y", lambda p: 0.2 + p[0] * p[1] - np.sin(3 * p[2]) + p[3] + np.cos(2 * p[0]) * 1.5 - 0.25 * p[1]),
                 ("min(x,y)+3.5", lambda p: min(p[0], p[1]) + 3.5)]
        lengths = []
        for text, _ in table:
            e = capi.Expr(text, "x,y,z,t")
            lengths.append(e.program()[0].size)
            assert text != "x" or e.program()[1].size == 0
            e.destroy()
        assert sorted(lengths) == [1, 1, 3, 5, 9, 23]
        texts = {f: t for f, (t, _) in zip(s.flags, table)}
        ref = fo.neumann_rhs(s.mo, s.fe, {f: fn for f, (_, fn) in zip(s.flags, table)})
        got = s.run(texts, shuffle=3)
        assert np.abs(got[:ref.size] - ref).max() <= 1e-12 * np.abs(ref).max()
        order = [s.flags[k] for k in (4, 0, 5, 2, 1, 3)]
        again = s.run(texts, order_of_exprs=order, shuffle=3)
        assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
    finally:
        s.close()


# ---- f. program caches ------------------------------------------------------------------------------------------------------------------------------

CACHE_TEXTS = ["2.5*sin(x)+y", "3.5*sin(x)+y", "2.5*sin(x)+y"]           # the second: the same code, another constant


def test_tensor_product_assembler_reloads_a_program_that_differs_in_constants_only(ctx):
    s = Tensor(ctx, (4, 4, 0), "linear")
    try:
        a, b = (capi.Expr(t) for t in CACHE_TEXTS[:2])
        assert np.array_equal(a.program()[0], b.program()[0]) and not np.array_equal(a.program()[1], b.program()[1])
        a.destroy(), b.destroy()
        reused = [s.run(t) for t in CACHE_TEXTS]
        assert not np.array_equal(reused[0], reused[1])
        for t, r in zip(CACHE_TEXTS, reused):
            fresh = s.assembler()
            try:
                assert np.array_equal(s.run(t, fresh).view(np.uint64), r.view(np.uint64))
            finally:
                fresh.destroy()
    finally:
        s.close()


def test_generic_assembler_reloads_its_program(ctx):
    s = Generic(ctx, "tri")
    try:
        reused = [s.resident(t) for t in CACHE_TEXTS]
        assert not np.array_equal(reused[0], reused[1])
        for t, r in zip(CACHE_TEXTS, reused):
            fresh = capi.GenericAssembler(ctx, s.geom, s.fe, s.ed, s.xs, s.K)
            try:
                assert np.array_equal(s.resident(t, fresh).view(np.uint64), r.view(np.uint64))
            finally:
                fresh.destroy()
    finally:
        s.close()


# ---- g. refusals ------------------------------------------------------------------------------------------------------------------------------------

FIVE = ("x+y+z+t+s", "x,y,z,t,s")


def refused_then_usable(run):
    """run(text, variables=...) refuses a program over five variables and serves the next call as if nothing had happened"""
    before = run(TEXT)
    with pytest.raises(capi.FemusHipError, match="5 variables"):
        run(FIVE[0], variables=FIVE[1])
    assert np.array_equal(run(TEXT).view(np.uint64), before.view(np.uint64))


def test_five_variables_refused_by_the_tensor_product_assembler(ctx):
    s = Tensor(ctx, (4, 4, 0), "linear")

    def run(text, variables="x,y,z,t"):
        e = capi.Expr(text, variables)
        try:
            s.asm.assemble_expr(s.A, s.res, None, e)
        finally:
            e.destroy()
        return s.res.to_numpy().copy()
    try:
        refused_then_usable(run)
    finally:
        s.close()


@pytest.mark.parametrize("args", [(4, 3, 0), (2, 2, 2)])
def test_five_variables_refused_by_the_neumann_entries(ctx, args):
    s = Faces(ctx, args)
    try:
        refused_then_usable(lambda text, variables="x,y,z,t": s.run({f: text for f in s.flags[:2]}, variables=variables))
    finally:
        s.close()


def test_five_variables_refused_by_the_line_assembler(ctx):
    s = Line(ctx)
    try:
        refused_then_usable(s.run)
    finally:
        s.close()


@pytest.mark.parametrize("case", ["tri", "mixed2d"])
def test_five_variables_refused_by_the_generic_kernels(ctx, case):
    """assemble_poisson_rows (tri) / assemble_poisson_mixed (mixed2d) and GenericAssembler.assemble"""
    s = Generic(ctx, case)
    try:
        refused_then_usable(s.one_shot)
        refused_then_usable(lambda text, variables="x,y,z,t": s.resident(text, variables=variables))
    finally:
        s.close()
