"""Every element kernel at every Gauss rule the C-ABI takes, against the oracle at the SAME rule: the generic and the mixed kernels, the tensor-product
assembler under its option sets, face integrals, the batched Jacobian with Hessians, the one-dimensional advection-diffusion and the Navier-Stokes family.  Curved meshes, a
source or flux that oscillates across an element, a non-zero state; 1e-12 of the largest entry for K and residual, 1e-13 for face integrals.  Rules other than the default
put a partial last chunk of Gauss points into the kernels (dead lanes), and a kernel that kept the 64 points of "seventh" whatever the rule would fail:
every case off "seventh" also asserts that the oracle at "seventh" differs from the oracle at its rule by more than 1000 times the tolerance."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from femus_amd import capi
from oracle import femus_oracle as fo
from oracle import femus_oracle_1d as o1
from oracle import femus_oracle_mixed as om
from oracle import femus_oracle_ns as ns
from oracle import femus_oracle_tet as oq
from oracle import femus_oracle_tri as ot
from oracle import femus_oracle_wedge as ow

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RULES = ["first", "third", "fifth", "seventh", "ninth"]
FES = ["linear", "serendipity", "biquadratic"]
SOURCE = "exp(x)*(1+y)*sin(11*x+7*y)-cos(9*z)"


def source(x):
    """SOURCE for points x[d] (arrays of any shape)"""
    return np.exp(x[0]) * (1 + x[1]) * np.sin(11 * x[0] + 7 * x[1]) - np.cos(9 * (x[2] if len(x) > 2 else 0.0))


def source_xg(xg):
    """SOURCE for the tensor-product oracle's Gauss points xg[..., d]"""
    return source(np.moveaxis(xg, -1, 0))


def bend(xs):
    """nodes moved smoothly inside the unit box (curved elements), the boundary kept"""
    return xs + 0.01 * np.sin(5 * xs[:, list(range(1, xs.shape[1])) + [0]]) * (xs * (1 - xs)).prod(axis=1, keepdims=True) * 60


def close(got, want, tol, order, want7=None, norm="max"):
    """got == want to tol of want's size (its largest entry, or with norm="l2" its 2-norm); given want7, the oracle at "seventh", also that want is more than
    1000 tol away from it when order is not "seventh" (the case is not vacuous).  K of linear simplices is the same at every rule: its callers pass no want7"""
    got, want = (np.asarray(a.toarray() if sp.issparse(a) else a) for a in (got, want))
    size = (lambda a: np.abs(a).max()) if norm == "max" else (lambda a: np.linalg.norm(a.ravel()))
    scale = size(want)
    assert size(got - want) <= tol * scale, (size(got - want) / scale, order)
    if want7 is not None and order != "seventh":
        want7 = np.asarray(want7.toarray() if sp.issparse(want7) else want7)
        assert size(want7 - want) > 1000 * tol * scale, ("vacuous", order)


def pattern(ctx, ed, nc, ndof):
    rp, col = capi.pattern_from_elements(np.asarray(ed)[:, :nc], ndof)
    return ctx.matrix_csr(ndof, ndof, rp, col)


_MESHES = {}


def mesh(name):
    """small two-level meshes, curved inside"""
    if name not in _MESHES:
        if name == "tri":
            ed, xs, ff, own = ot.refine(*ot.box_mesh(3, 2)[:3])
            _MESHES[name] = ("tri", ed, bend(xs), ff, own)
        elif name in ("tet", "wedge"):
            m = oq if name == "tet" else ow
            ed, xs, ff, own = m.refine(*m.read_gambit(os.path.join(HERE, "golden", "cube_%s.neu" % name.capitalize()))[:3])
            _MESHES[name] = (name, ed, bend(xs), ff, own)
        elif name == "mixed3d":
            kind, ed, xs, ff, own = om.refine(*om.read_gambit(os.path.join(HERE, "golden", "cube_all_shapes_Six_boundary_groups.neu"))[:4])
            _MESHES[name] = (kind, ed, bend(xs), ff, own)
        else:                                                   # "hex" / "quad": the box generator's meshes, refined once
            args = (2, 2, 2) if name == "hex" else (3, 2, 0)
            mo = fo.build_levels(*args, 2)[-1]
            mo.coords = bend(mo.coords)
            _MESHES[name] = (args, mo)
    return _MESHES[name]


# ---- a. the generic kernel (fh_assemble_poisson_rows) -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("geom", ["tri", "tet", "wedge", "quad", "hex"])
def test_generic_kernel_at_every_rule(ctx, geom, fe, order):
    f = capi.Expr(SOURCE, "x,y,z,t")
    if geom in ("quad", "hex"):
        _, mo = mesh(geom)
        ed, xs, ndof, nc = mo.elem_dof, mo.coords, fo.n_dofs(mo, fe), fo.ndofs(geom, fe)
        u = np.random.default_rng(11).uniform(-1, 1, ndof)
        neg = lambda xg: -source_xg(xg)                         # the tensor-product oracle integrates -f phi, the 001_Poisson callback +f phi
        Ko, Fo = fo.assemble_poisson(mo, fe, neg, sol=u, order=order)
        _, F7 = fo.assemble_poisson(mo, fe, neg, sol=u, order="seventh")
    else:
        kind, ed, xs, ff, own = mesh(geom)
        ndof, nc = om.n_dofs(own, fe), om.NDOF[geom][fe]
        u = np.random.default_rng(11).uniform(-1, 1, ndof)
        Ko, Fo = om.assemble_batched(kind, ed, xs, fe, source, sol=u, order=order)
        _, F7 = om.assemble_batched(kind, ed, xs, fe, source, sol=u, order="seventh")
    K = pattern(ctx, ed, nc, ndof)
    RES, SOL = ctx.vector(ndof), ctx.vector_from(u)
    try:
        capi.assemble_poisson_rows(ctx, geom, fe, ed, xs, K, RES, sol=SOL, source=f, order=order)
        close(K.to_scipy(), Ko, 1e-12, order)
        close(RES.to_numpy(), Fo, 1e-12, order, F7)
    finally:
        f.destroy(), K.destroy(), RES.destroy(), SOL.destroy()


# ---- b. the mixed kernel (fh_assemble_poisson_mixed): each shape its own point count in one launch -----------------------------------------------------

def _square_quad_and_two_triangles():
    """the unit square as one QUAD9 and two TRI7 sharing curved edges (test_mixed_3d.py)"""
    xs = np.array([[0, 0], [.5, 0], [.5, 1], [0, 1], [1, 0], [1, 1], [.25, 0], [.53, .5], [.25, 1], [0, .5], [.75, 0], [.77, .52], [1, .5], [.75, 1],
                   [.26, .51], [.68, .17], [.84, .66]], dtype=float)
    kind = np.array(["quad", "tri", "tri"])
    ed = np.full((3, 9), -1, dtype=np.int64)
    ed[0] = [0, 1, 2, 3, 6, 7, 8, 9, 14]
    ed[1, :7] = [1, 4, 2, 10, 11, 7, 15]
    ed[2, :7] = [4, 5, 2, 12, 13, 11, 16]
    return kind, ed, xs


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("case", ["cube", "square"])
def test_mixed_kernel_at_every_rule(ctx, case, fe, order):
    if case == "cube":
        kind, ed, xs, _, own = mesh("mixed3d")
        ndof = om.n_dofs(own, fe)
    else:
        kind, ed, xs = _square_quad_and_two_triangles()
        ndof = (6, 14, 17)[FES.index(fe)]
    u = np.random.default_rng(11).uniform(-1, 1, ndof)
    Ko, Fo = om.assemble(kind, ed, xs, fe, source, u, order)
    _, F7 = om.assemble(kind, ed, xs, fe, source, u, "seventh")
    Kb, Fb = om.assemble_batched(kind, ed, xs, fe, source, sol=u, order=order)
    assert abs(Kb - Ko).max() <= 1e-14 * abs(Ko).max() and np.abs(Fb - Fo).max() <= 1e-14 * np.abs(Fo).max()
    pat = sp.csr_matrix(Ko)
    pat.sort_indices()
    K = capi.Mat.from_csr(ctx, ndof, ndof, pat.indptr, pat.indices)
    RES, SOL = ctx.vector(ndof), ctx.vector_from(u)
    f = capi.Expr(SOURCE, "x,y,z,t")
    try:
        capi.assemble_poisson_mixed(ctx, fe, kind, ed, xs, K, RES, sol=SOL, source=f, order=order)
        close(K.to_scipy(), Ko, 1e-12, order)
        close(RES.to_numpy(), Fo, 1e-12, order, F7)
    finally:
        f.destroy(), K.destroy(), RES.destroy(), SOL.destroy()


# ---- c. the tensor-product assembler (fh_assembler_create + fh_assemble_poisson) under its option sets -----------------------------------------------------

OPTIONS = {"defaults": {}, "tile": {"assemble_sym": 0}, "emap_scatter": {"assemble_two_pass": 0},
           "search_scatter": {"assemble_two_pass": 0, "assemble_emap": 0}}
DEFAULTS = {"assemble_sym": 1, "assemble_two_pass": 1, "assemble_emap": 1, "assemble_affine": 0}
ELEMENTS = {"HEX27": ("hex", "biquadratic"), "HEX20": ("hex", "serendipity"), "HEX8": ("hex", "linear"),
            "QUAD9": ("quad", "biquadratic"), "QUAD8": ("quad", "serendipity"), "QUAD4": ("quad", "linear")}


def restore_options(ctx):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    ctx.set_option("debug_poison", int(os.environ.get("FEMUS_HIP_POISON", "0")))     # what a context starts with


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("opts", list(OPTIONS))
@pytest.mark.parametrize("elem", list(ELEMENTS))
def test_tensor_product_assembler_at_every_rule(ctx, elem, opts, order):
    geom, fe = ELEMENTS[elem]
    args, mo = mesh(geom)
    m = capi.Mesh.box(*args).refine()
    ed, xy0, _ = m.arrays()
    assert np.array_equal(ed, mo.elem_dof) and np.array_equal(bend(xy0), mo.coords)
    xy = mo.coords
    n, nc = fo.n_dofs(mo, fe), fo.ndofs(geom, fe)
    u = np.random.default_rng(13).uniform(-1, 1, n)
    Ao, bo = fo.assemble_poisson(mo, fe, source_xg, sol=u, order=order)
    _, b7 = fo.assemble_poisson(mo, fe, source_xg, sol=u, order="seventh")
    A = pattern(ctx, ed, nc, n)
    res, sol = ctx.vector(n), ctx.vector_from(u)
    f = capi.Expr(SOURCE, "x,y,z,t")
    asm = None
    try:
        for k, v in OPTIONS[opts].items():
            ctx.set_option(k, v)
        ctx.set_option("debug_poison", 1)
        asm = capi.Assembler(ctx, m, fe, A, order=order, elem_dof=ed, coords=xy)
        if elem == "HEX27" and order != "seventh":             # the fused cluster plan serves 64 points only: it must refuse, not run
            assert not asm.fused_info()["active"]
        if elem == "HEX27" and order == "seventh" and opts == "defaults":
            assert asm.fused_info()["active"]                  # a refined mesh: the sibling groups are there
        asm.assemble_expr(A, res, sol, f)
        close(A.to_scipy(), Ao, 1e-12, order)
        close(res.to_numpy(), bo, 1e-12, order, b7)
        K, F = asm.element_matrices(sol, 1, (2.0, 1.3))         # the closed-form source of the element kernel
        Ko, Fo = fo.elem_poisson_batch(fo.ElemType(geom, fe, order), np.transpose(xy[ed], (0, 2, 1)), u[ed[:, :nc]],
                                       lambda xg: 2.0 * np.prod(np.sin(1.3 * xg), axis=-1))
        assert np.abs(K - Ko).max() <= 1e-12 * np.abs(Ko).max() and np.abs(F - Fo).max() <= 1e-12 * np.abs(Fo).max()
    finally:
        restore_options(ctx)
        if asm is not None:
            asm.destroy()
        f.destroy(), A.destroy(), res.destroy(), sol.destroy()


@pytest.mark.parametrize("order", RULES)
def test_affine_path_runs_at_64_points_only(ctx, order):
    """HEX27 on a flat refined box (every element affine): at "seventh" the affine path takes every element; at any other rule it must take none and the
    quadrature kernels integrate with that rule -- against the oracle at the same rule, with the option on"""
    m = capi.Mesh.box(2, 2, 2).refine()
    mo = fo.build_levels(2, 2, 2, 2)[-1]
    ed, xy, _ = m.arrays()
    assert np.array_equal(ed, mo.elem_dof) and np.array_equal(xy, mo.coords)
    n = m.nnode
    u = np.random.default_rng(17).uniform(-1, 1, n)
    Ao, bo = fo.assemble_poisson(mo, "biquadratic", source_xg, sol=u, order=order)
    _, b7 = fo.assemble_poisson(mo, "biquadratic", source_xg, sol=u, order="seventh")
    A = pattern(ctx, ed, 27, n)
    res, sol = ctx.vector(n), ctx.vector_from(u)
    f = capi.Expr(SOURCE, "x,y,z,t")
    asm = None
    try:
        ctx.set_option("assemble_affine", 1)
        asm = capi.Assembler(ctx, m, "biquadratic", A, order=order)
        assert asm.affine_count()[0] == (m.nel if order == "seventh" else 0)
        asm.assemble_expr(A, res, sol, f)
        close(A.to_scipy(), Ao, 1e-12, order)
        close(res.to_numpy(), bo, 1e-12, order, b7)
    finally:
        restore_options(ctx)
        if asm is not None:
            asm.destroy()
        f.destroy(), A.destroy(), res.destroy(), sol.destroy()


# ---- d. face integrals with a parsed flux (fh_assemble_neumann_faces_expr) ----------------------------------------------------------------------------

def _face_list(kind, ed, ff, fe, flags):
    """flagged faces of the simplex / prism / mixed oracles' meshes, by face shape"""
    out = {}
    for e, fl in zip(*np.nonzero(ff < -1)):
        if ff[e, fl] in flags:
            s = kind if isinstance(kind, str) else kind[e]
            nv = om.NVF[s][fl]
            out.setdefault(nv, []).append(ed[e, om.FACE[s][fl][:om.NFN[nv][fe]]])
    return {nv: np.array(v) for nv, v in out.items()}


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("geom", ["hex", "quad", "tet", "wedge"])
def test_face_integrals_at_every_rule(ctx, geom, fe, order):
    flux = source
    e = capi.Expr(SOURCE, "x,y,z,t")
    try:
        if geom in ("hex", "quad"):                             # QUAD8 / QUAD9 faces of hexahedra, EDGE3 edges of quadrilaterals, through the mesh's flags
            args, mo = mesh(geom)
            m = capi.Mesh.box(*args).refine()
            m.set_coords(mo.coords)
            flags = (-4, -3) if geom == "hex" else (-3, -2)
            res = ctx.vector(m.nnode)
            capi.assemble_neumann(ctx, m, fe, res, {fl: e for fl in flags}, order=order)
            ref, ref7 = (fo.neumann_rhs(mo, fe, {fl: flux for fl in flags}, order=o) for o in (order, "seventh"))
            close(res.to_numpy()[:ref.size], ref, 1e-13, order, ref7)
            assert np.all(res.to_numpy()[ref.size:] == 0.0)      # nothing past the family's dofs
            res.destroy()
        else:                                                   # TRI3 / TRI6 / TRI7 faces of tetrahedra; both kinds of faces of prisms
            kind, ed, xs, ff, own = mesh(geom)
            m = oq if geom == "tet" else ow
            flags = (-4, -6, -7)
            ref, ref7 = (m.neumann(ed, xs, ff, fe, {fl: flux for fl in flags}, order=o) for o in (order, "seventh"))
            res = ctx.vector(ref.size)
            for nv, fn in _face_list(kind, ed, ff, fe, flags).items():
                capi.assemble_neumann_faces_expr(ctx, "triface" if nv == 3 else "quadface", fe, fn, np.zeros(len(fn)), [e], xs, res, order=order)
            close(res.to_numpy(), ref, 1e-13, order, ref7)
            res.destroy()
    finally:
        e.destroy()


# ---- e. the batched Jacobian with Hessians (fh_fe_jacobian) ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("fe", ["linear", "biquadratic"])
@pytest.mark.parametrize("args", [(2, 2, 1), (3, 2, 0)])
def test_jacobian_with_hessians_at_every_rule(ctx, args, fe, order):
    m = capi.Mesh.box(*args)
    ed, xy, _ = m.arrays()
    rng = np.random.default_rng(21)
    xyc = xy + rng.uniform(-0.03, 0.03, xy.shape)
    w, g, h = capi.fe_jacobian(ctx, m, fe, order=order, hessians=True, coords=xyc)
    geom = "hex" if m.dim == 3 else "quad"
    et = fo.ElemType(geom, fe, order)
    assert w.shape == (ed.shape[0], et.ng)
    scale_g, scale_h = abs(g).max(), abs(h).max()
    for e in range(ed.shape[0]):
        vt = [xyc[ed[e, :et.nc], d] for d in range(m.dim)]
        for ig in range(et.ng):
            wo, _, go, ho = et.jacobian(vt, ig, nabla=True)
            assert abs(w[e, ig] - wo) <= 1e-13 * abs(wo)
            assert abs(g[e, ig].ravel() - go).max() <= 1e-12 * scale_g
            assert abs(h[e, ig].ravel() - ho).max() <= 1e-12 * scale_h
    w7, _, _ = capi.fe_jacobian(ctx, m, fe, order="seventh", hessians=True, coords=xyc)
    if order != "seventh":
        assert w7.shape[1] != w.shape[1]
    if fe == "biquadratic":                                     # affine elements: the Hessians reproduce a quadratic's, the weights add up to the volume
        dim = m.dim
        A = np.eye(dim) + 0.2 * rng.standard_normal((dim, dim))
        xa = xy @ A.T + 0.3
        w, g, h = capi.fe_jacobian(ctx, m, fe, order=order, hessians=True, coords=xa)
        Q = rng.standard_normal((dim, dim))
        Q = Q + Q.T
        q = 0.5 * np.einsum("ni,ij,nj->n", xa, Q, xa)
        got = np.einsum("egjk,ej->egk", h, q[ed])
        pairs = [(0, 0), (1, 1), (0, 1)] if dim == 2 else [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0)]
        assert abs(got - np.array([Q[a, b] for a, b in pairs])).max() <= 1e-10 * abs(Q).max()
        assert abs(w.sum() - abs(np.linalg.det(A))) <= 1e-12


# ---- f. one-dimensional advection-diffusion (fh_assemble_advdiff_line) --------------------------------------------------------------------------------

@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("fe", ["linear", "biquadratic"])
def test_line_advdiff_at_every_rule(ctx, fe, order):
    NU, V = 0.01, 1.0
    line_source = lambda x: 10. * np.exp(-5. * x) - 4. * np.exp(-x)
    ed, xs, _, nv = o1.box_mesh(13, -0.3, 1.7)
    xs = xs + 0.02 * np.sin(3.0 * xs)
    nc = 2 if fe == "linear" else 3
    ndof = nv if fe == "linear" else xs.size
    u = np.random.default_rng(3).uniform(-1, 1, ndof)
    Ko, Fo = o1.assemble(ed, xs, fe, u, line_source, NU, V, order=order)
    _, F7 = o1.assemble(ed, xs, fe, u, line_source, NU, V, order="seventh")
    K = pattern(ctx, ed, nc, ndof)
    RES, SOL = ctx.vector(ndof), ctx.vector_from(u)
    src = capi.Expr("10.*exp(-5.*x) - 4.*exp(-x)", "x,y,z,t")
    try:
        capi.assemble_advdiff_line(ctx, fe, ed, xs, K, RES, NU, V, sol=SOL, source=src, order=order)
        close(K.to_scipy(), Ko, 1e-12, order)
        close(RES.to_numpy(), Fo, 1e-12, order, F7)
    finally:
        src.destroy(), K.destroy(), RES.destroy(), SOL.destroy()


# ---- g. the Navier-Stokes family: Taylor-Hood, piecewise-linear pressure, stabilised equal order, advection-diffusion, open-boundary pressure ----------

NS_LO, NS_HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)


def ns_box(box, lo, seed):
    """a distorted box mesh (the full Jacobian path) on both sides"""
    mo = fo.build_levels(*box, 1, lo, NS_HI)[0]
    mh = capi.Mesh.box(*box, lo, NS_HI)
    rng = np.random.default_rng(seed)
    mo.coords = mo.coords + 0.02 * rng.standard_normal(mo.coords.shape)
    mh.set_coords(mo.coords)
    return mo, mh, rng


def nsbenc():
    """the known-answer test's QUAD9 mesh around the cylinder, as read"""
    mh = capi.Mesh.read_gambit(os.path.join(HERE, "golden", "nsbenc.neu"))
    ed, xy, ff = mh.arrays()
    return fo.Mesh("quad", ed, xy, ff, level=0), mh


def ns_check(asm, A, res, sol, extra, Ao, bo, b7, order, objects):
    """run asm.assemble, compare with the oracle at the rule (the existing tests' tolerances: K to the largest entry, the residual in 2-norm), free"""
    try:
        asm.assemble(A, res, sol, *extra)
        close(A.to_scipy(), Ao, 1e-12, order)
        close(res.to_numpy(), bo, 1e-12, order, b7, norm="l2")
    finally:
        for o in [asm, A, res, sol] + objects:
            o.destroy()


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("box", [(3, 2, 0), (2, 1, 2)])
def test_navier_stokes_taylor_hood_at_every_rule(ctx, box, order):
    """NSAssembler (Q2 / Q1) in two and three dimensions against femus_oracle_ns.assemble_ns"""
    mo, mh, rng = ns_box(box, NS_LO, 3)
    lay = ns.NSLayout(mo)
    es = capi.system_elem_dofs(mh, ["biquadratic"] * mo.dim + ["linear"])[2]
    u = 0.5 * rng.standard_normal(lay.n)
    Ao, bo = ns.assemble_ns(mo, lay, u, 0.03, order)
    _, b7 = ns.assemble_ns(mo, lay, u, 0.03, "seventh")
    A = pattern(ctx, es, es.shape[1], lay.n)
    ns_check(capi.NSAssembler(ctx, mh, A, order), A, ctx.vector(lay.n), ctx.vector_from(u), (0.03,), Ao, bo, b7, order, [mh])


@pytest.mark.parametrize("order", RULES)
def test_navier_stokes_piecewise_linear_pressure_at_every_rule(ctx, order):
    """NSPwAssembler (Q2 / discontinuous P1) on the known-answer test's mesh against assemble_ns with the piecewise-linear pressure at the same rule"""
    mo, mh = nsbenc()
    lay = ns.NSLayoutPwLinear(mo)
    x = np.random.default_rng(11).uniform(-1, 1, lay.n)
    Ao, bo = ns.assemble_ns(mo, lay, x, 0.001, order, etp=ns.PwLinearPressure("quad", order))
    _, b7 = ns.assemble_ns(mo, lay, x, 0.001, "seventh", etp=ns.PwLinearPressure("quad", "seventh"))
    A = ctx.matrix_from_elements(capi.NSPwAssembler.elem_sys(mh), lay.n)
    ns_check(capi.NSPwAssembler(ctx, mh, A, order), A, ctx.vector(lay.n), ctx.vector_from(x), (0.001,), Ao, bo, b7, order, [mh])


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("box", [(4, 3, 0), (2, 2, 2)])
def test_navier_stokes_stabilised_at_every_rule(ctx, box, order):
    """NSStabAssembler (equal-order Q1, Franca-Frey) against assemble_ns_stab"""
    mo, mh, rng = ns_box(box, (-0.5, -0.5, 0.0), 3)
    lay = ns.NSLayoutEqualOrder(mo)
    es = capi.system_elem_dofs(mh, ["linear"] * (mo.dim + 1))[2]
    u = 0.5 * rng.standard_normal(lay.n)
    Ao, bo = ns.assemble_ns_stab(mo, lay, u, 1e-2, order)
    _, b7 = ns.assemble_ns_stab(mo, lay, u, 1e-2, "seventh")
    A = pattern(ctx, es, es.shape[1], lay.n)
    ns_check(capi.NSStabAssembler(ctx, mh, A, order), A, ctx.vector(lay.n), ctx.vector_from(u), (1e-2,), Ao, bo, b7, order, [mh])


@pytest.mark.parametrize("order", RULES)
def test_advection_diffusion_at_every_rule(ctx, order):
    """AdvDiffAssembler (the temperature callback of the known-answer test) in a random velocity field against assemble_advdiff"""
    mo, mh = nsbenc()
    rng = np.random.default_rng(21)
    t0, v0 = rng.uniform(-1, 1, mh.nnode), rng.uniform(-1, 1, 2 * mh.nnode)
    Ao, bo = ns.assemble_advdiff(mo, t0, v0, 1e-3, order)
    _, b7 = ns.assemble_advdiff(mo, t0, v0, 1e-3, "seventh")
    A = ctx.matrix_from_mesh(mh, "biquadratic")
    V = ctx.vector_from(v0)
    ns_check(capi.AdvDiffAssembler(ctx, mh, A, order), A, ctx.vector(mh.nnode), ctx.vector_from(t0), (V, 1e-3), Ao, bo, b7, order, [V, mh])


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("box", [(3, 2, 0), (2, 2, 2)])
def test_open_boundary_pressure_at_every_rule(ctx, box, order):
    """fh_assemble_pressure_faces: a number on the inlet, an oscillating parsed function on the outlet, curved faces in planar sides, against
    pressure_boundary_residual at the same rule (RES = -aRes)"""
    from femus_amd.navier_stokes import open_boundary_faces
    dim = 2 if box[2] == 0 else 3
    mo = fo.build_levels(*box, 2, NS_LO, NS_HI)[-1]
    mh = capi.Mesh.box(*box, NS_LO, NS_HI).refine()
    x0 = mo.coords.copy()
    mo.coords = mo.coords + 0.01 * np.random.default_rng(8).standard_normal(mo.coords.shape)
    on_side = np.isclose(abs(x0), 0.5)
    mo.coords[on_side] = x0[on_side]
    mh.set_coords(mo.coords)
    lay = ns.NSLayout(mo)
    inlet, outlet = (4, 2) if dim == 2 else (5, 3)

    def bc(x, name, face):
        if name == "P":
            return False, (1.25 if face == inlet else np.sin(7 * x[1] + 5 * x[dim - 1]) * np.exp(x[0]) if face == outlet else 0.0)
        return (face not in (inlet, outlet), 0.0) if name == "U" else (True, 0.0)
    faces, fnames = open_boundary_faces(mh, ["U", "V", "W"][:dim] + ["P"], bc)
    assert faces.shape[0] > 0 and set(fnames.tolist()) == {inlet, outlet}
    e_out = capi.Expr("sin(7*y + 5*%s)*exp(x)" % ("y" if dim == 2 else "z"), "x,y,z,t")
    off = capi.system_elem_dofs(mh, ["biquadratic"] * dim + ["linear"])[1]
    res = ctx.vector(lay.n)
    try:
        sel = fnames == inlet
        capi.assemble_pressure_faces(ctx, mh, res, faces[sel], 1.25, off[:dim], order=order)
        capi.assemble_pressure_faces(ctx, mh, res, faces[~sel], [(e_out, np.ones((~sel).sum(), bool))], off[:dim], order=order)
        ref, ref7 = (-ns.pressure_boundary_residual(mo, lay, bc, order=o) for o in (order, "seventh"))
        close(res.to_numpy(), ref, 1e-13, order, ref7)
    finally:
        e_out.destroy(), res.destroy(), mh.destroy()
