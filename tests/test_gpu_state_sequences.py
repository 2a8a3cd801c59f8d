"""GPU sequences: an object is REUSED after its inputs were changed through some other entry point.  The library keeps state derived from a matrix's
values (the macro rows and the partial-row buffer of a fused assembly, the element-row buffer, the cached explicit transpose, plans, factors, colourings,
coarse inverses and the captured cycle of a multigrid, NavierStokesMG.mg[ig]); each piece is right only while every writer of the values tells it so.

Every case compares the reused object with (a) the oracle / scipy on the new inputs, at the tolerance the existing test of the same quantity uses
(1e-13 of the largest entry for coarse operators, 1e-11 relative for one cycle, 1e-14 scaled for the transposed product), and where a second object
can be made (b) with the same library calls on objects made fresh from the new inputs, bit for bit.  Every case also shows that it can fail: the answer a
stale cache would give is computed with the oracle alone and must differ from the right one by more than 1000 times the tolerance.  Meshes are curved
(the nodes of every level moved independently): on flat boxes the rediscretised and the Galerkin operators agree to rounding and nothing could be seen."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import femus_amd
from femus_amd import capi
from femus_amd.poisson import PoissonMG
from oracle import femus_oracle as fo

pytestmark = pytest.mark.gpu
FE = "biquadratic"
ONE = lambda xg: np.ones(xg.shape[:2])
TOL_COARSE = 1e-13          # of the largest entry: test_elementwise_galerkin_after_a_fused_assembly
TOL_CYCLE = 1e-11           # relative: test_vcycle_matches_oracle
TOL_SPMV = 1e-14            # scaled by |A|^T |x|


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ---- curved hierarchies: the device meshes and the oracle's, with the same coordinates ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def curved_coords(nl, seed):
    rng = np.random.default_rng(seed)
    return [m.coords + rng.uniform(-0.01, 0.01, m.coords.shape) / 2 ** l for l, m in enumerate(fo.build_levels(2, 2, 2, nl))]


def device_meshes(nl, seed):
    ms = [capi.Mesh.box(2, 2, 2)]
    for _ in range(nl - 1):
        ms.append(ms[-1].refine())
    for m, xy in zip(ms, curved_coords(nl, seed)):       # after the refinement: every level has displacements of its own
        m.set_coords(xy)
    return ms


@functools.lru_cache(maxsize=None)
def oracle_levels(nl, seed):
    """per level: the oracle's assembled (rediscretised) operator; the interpolations with the Dirichlet rows / columns zeroed; the Dirichlet sets"""
    oms = fo.build_levels(2, 2, 2, nl)
    for m, xy in zip(oms, curved_coords(nl, seed)):
        m.coords = xy.copy()
    bdc = [fo.dirichlet_dofs(m, FE) for m in oms]
    P = [None] + [fo.zero_interpolator_dirichlet(fo.build_prolongator(oms[l - 1], oms[l], FE), bdc[l], bdc[l - 1]) for l in range(1, nl)]
    A = [fo.assemble_poisson(m, FE, ONE)[0] for m in oms]
    return oms, A, P, bdc


def chain(A_top, P, bdc, top=None):
    """Galerkin chain below A_top (un-penalised), then SetPenalty on every level: what PoissonMG.level_operators leaves in A[0 .. top]"""
    top = len(P) - 1 if top is None else top
    raw = {top: A_top.tocsr()}
    for l in range(top, 0, -1):
        raw[l - 1] = (P[l].T @ raw[l] @ P[l]).tocsr()
    return [fo.zero_rows(raw[l], bdc[l], 1.0) for l in range(top + 1)]


def assert_operators(pb, want, levels, what=""):
    for l in levels:
        got = pb.A[l].to_scipy()
        err = abs(got - want[l]).max() / abs(want[l]).max()
        print("%s level %d: |device - oracle| / max = %.2e" % (what, l, err))
        assert err <= TOL_COARSE, (what, l, err)


def assert_distinguishable(right, stale, levels, tol, what=""):
    for l in levels:
        d = abs(right[l] - stale[l]).max() / abs(right[l]).max()
        assert d > 1000 * tol, (what, l, d)


# ---- 1. macro rows versus every writer of the matrix's values --------------------------------------------------------------------------------------
# A writer gets the environment E (ctx, pb, A = the finest matrix after a fused assembly, its assembled values v0, the pattern, the mesh arrays) and
# returns (A_now as scipy, device objects to destroy).  The matrix is left holding A_now; the assembly was A_asm.
def _interior_rows(E, k):
    inner = np.setdiff1d(np.arange(E["n"]), E["pb"].bdc[-1])
    return inner[:: max(1, inner.size // k)][:k].astype(np.int32)


def w_zero(E):
    E["A"].zero()
    return 0.0 * E["asm_sp"], []


def w_set_values(E):
    E["A"].set_values(2.0 * E["v0"])
    return 2.0 * E["asm_sp"], []


def _block(E):
    dofs = E["ed"][E["ed"].shape[0] // 2]                  # the 27 nodes of one element: every pair is in the pattern
    vals = np.random.default_rng(5).uniform(1.0, 2.0, (27, 27)) * abs(E["v0"]).max()
    add = sp.coo_matrix((vals.ravel(), (np.repeat(dofs, 27), np.tile(dofs, 27))), shape=(E["n"], E["n"])).tocsr()
    return dofs, vals, add


def w_add_matrix_blocked(E):
    dofs, vals, add = _block(E)
    E["A"].add_matrix_blocked(vals, dofs, dofs)
    return (E["asm_sp"] + add).tocsr(), []


def w_stage_flush(E):
    dofs, vals, add = _block(E)
    E["A"].stage_matrix_blocked(vals, dofs, dofs)
    E["A"].flush()
    return (E["asm_sp"] + add).tocsr(), []


def w_insert_row(E):
    now = E["asm_sp"].copy()
    for r in _interior_rows(E, 40):
        cols, vals = E["A"].get_row(r)
        E["A"].insert_row(r, cols, 3.0 * vals)
        now.data[now.indptr[r]:now.indptr[r + 1]] *= 3.0
    return now, []


def w_zero_cols(E):
    idx = _interior_rows(E, 200)
    E["A"].zero_cols(idx)
    mask = np.ones(E["n"])
    mask[idx] = 0.0
    return (E["asm_sp"] @ sp.diags(mask)).tocsr(), []


def w_gather_values(E):
    src = E["ctx"].matrix_csr(E["n"], E["n"], E["rp"], E["col"], 0.5 * E["v0"][::-1].copy())
    ident = capi.Index(E["ctx"], np.arange(E["v0"].size, dtype=np.int32))
    ident.gather_matrix_values(E["A"], src)
    now = E["asm_sp"].copy()
    now.data = 0.5 * E["v0"][::-1].copy()
    return now, [src, ident]


def _second_assembler(E, order="seventh", options=()):
    """another assembler of the same matrix on OTHER coordinates, through the path the options select"""
    ctx = E["ctx"]
    xy2 = E["xy"] * np.array([1.0, 1.3, 0.8])                     # a stretched mesh: another operator on the same pattern
    for name, value, _ in options:
        ctx.set_option(name, value)
    try:
        asm2 = capi.Assembler(ctx, None, FE, E["A"], order=order, elem_dof=E["ed"], coords=xy2)
        res = ctx.vector(E["n"])
        asm2.assemble(E["A"], res, None, 0, (1.0,))
        path, fused = asm2.last_path(), asm2.fused_info()["active"]
    finally:
        for name, _, back in options:
            ctx.set_option(name, back)
    om = fo.Mesh("hex", E["ed"], xy2, None)
    om.own_size = None
    now = fo.assemble_poisson(om, FE, ONE, order=order)[0]
    return now, [asm2, res], path, fused


def w_two_pass_ninth(E):
    now, objs, path, fused = _second_assembler(E, order="ninth")
    assert path == "two-pass" and not fused
    return now, objs


def w_two_pass_option(E):
    now, objs, path, fused = _second_assembler(E, options=(("assemble_fused", 0, 1),))
    assert path == "two-pass" and not fused
    return now, objs


def w_coloured(E):
    now, objs, path, fused = _second_assembler(E, options=(("assemble_two_pass", 0, 1),))
    assert path is None                                           # neither of the row-gather paths: the coloured scatter
    return now, objs


def w_fused_other_assembler(E):
    now, objs, path, fused = _second_assembler(E)
    assert path == "fused" and fused
    return now, objs


class _TwoEqualRanks:
    """the transport of a one-rank host halo that answers as if a second rank had contributed the same values: the sum is twice the input"""

    def alltoallv(self, parts, dtype):
        return parts

    def allreduce_sum(self, a):
        return 2.0 * a


def w_halo_allreduce_mat(E):
    z = np.zeros(1, np.int32)
    halo = capi.Halo.host(E["ctx"], 0, 1, _TwoEqualRanks(), z, np.zeros(1, np.int32)[:0], z)
    halo.allreduce_mat(E["A"])
    return 2.0 * E["asm_sp"], [halo]


WRITERS = {"halo_allreduce_mat": w_halo_allreduce_mat, "zero": w_zero, "set_values": w_set_values, "add_matrix_blocked": w_add_matrix_blocked, "insert_row": w_insert_row, "stage_flush": w_stage_flush,
           "zero_cols": w_zero_cols, "gather_values": w_gather_values, "two_pass_ninth": w_two_pass_ninth, "two_pass_option": w_two_pass_option,
           "coloured": w_coloured, "fused_other_assembler": w_fused_other_assembler}


def environment(ctx, nl=3, seed=7):
    pb = PoissonMG(ctx, 2, 2, 2, nl, meshes=device_meshes(nl, seed)).init()
    assert pb.gal_elem and pb.asm[-1].fused_info()["active"]
    pb.assemble()
    assert pb.asm[-1].last_path() == "fused"
    A = pb.A[-1]
    rp, col = A.pattern()
    ed, xy, _ = pb.meshes[-1].arrays()
    oms, Ao, P, bdc = oracle_levels(nl, seed)
    # positive control: with no writer in between the product IS made from the macro rows (all the further conditions of fh_assembler_galerkin hold on these
    # meshes) -- nobody asks for the element rows, so assemble_fused 1 keeps the fused path at the next assembly; after a writer it does not (checked per row)
    pb.level_operators()
    pb.assemble()
    assert pb.asm[-1].last_path() == "fused", "the macro rows are not the source of the product here: the writer rows would prove nothing"
    v0 = A.values()
    asm_sp = sp.csr_matrix((v0, col, rp), shape=(A.m(), A.n()))
    assert abs(asm_sp - Ao[-1]).max() <= 1e-12 * abs(Ao[-1]).max()
    return {"ctx": ctx, "pb": pb, "A": A, "v0": v0, "rp": rp, "col": col, "ed": ed, "xy": xy, "n": A.m(), "asm_sp": asm_sp, "Ao": Ao, "P": P, "bdc": bdc}


def finish(E, objs):
    for o in objs:
        o.destroy()
    E["pb"].destroy()


@pytest.mark.parametrize("writer", sorted(WRITERS))
def test_galerkin_product_after_every_writer_of_the_fine_matrix(ctx, writer):
    """fused assembly into A, then a writer of A's values that is not the assembler, then the Galerkin chain: the coarse operators are P^T A_asm P of the
    ASSEMBLED operator (fh_assembler_galerkin goes back to the element rows of the assembly), whoever wrote A since -- not a mixture of the partial-row
    buffer with what the matrix holds now.  The stale answer (the chain of what the matrix holds now: the limit of reading every macro row from it) differs
    by more than 1000 tolerances.  (fh_mat_restrict and the sparse products create the matrices they write; a product into A by fh_assembler_galerkin is the
    PoissonMG sequence below; the Navier-Stokes and the generic assemblers cannot target a scalar Q2 matrix of a fused plan: part 2.)"""
    E = environment(ctx)
    objs = []
    try:
        now, objs = WRITERS[writer](E)
        got_now = E["A"].to_scipy()
        assert abs(got_now - now).max() <= 1e-12 * max(abs(E["v0"]).max(), abs(now).max()), "the writer did not leave what this test thinks it left"
        right = chain(E["Ao"][-1], E["P"], E["bdc"])
        stale = chain(now, E["P"], E["bdc"])
        assert_distinguishable(right, stale, range(2), TOL_COARSE, writer)
        E["pb"].level_operators()
        assert_operators(E["pb"], right, range(2), writer)
        E["pb"].assemble()
        assert E["pb"].asm[-1].last_path() == "two-pass"       # the product had to go back to the element rows: the writer was seen
    finally:
        finish(E, objs)


@pytest.mark.parametrize("how", ["mat_zero_rows", "index_zero_rows"])
def test_dirichlet_row_replacement_keeps_the_macro_rows(ctx, how):
    """the documented exception (SetPenalty between assembly and preparation, the flow of every MGsolve): the macro rows stay the source -- the assembler stays on
    the fused path at the next assembly -- and the coarse operators are those of the assembled operator.  (No stale answer to tell apart here: the
    interpolation has zero rows at the Dirichlet nodes, so the replaced rows cannot reach a coarse operator; what the case pins is the path.)"""
    E = environment(ctx)
    try:
        pb = E["pb"]
        if how == "mat_zero_rows":
            E["A"].mat_zero_rows(pb.bdc[-1], 1.0)
        else:
            pb.bdc_dev[-1].zero_rows(E["A"], 1.0)
        right = chain(E["Ao"][-1], E["P"], E["bdc"])
        pb.level_operators()
        assert_operators(pb, right, range(2), how)
        pb.assemble()
        assert pb.asm[-1].last_path() == "fused"              # nobody had to ask for the element rows
    finally:
        finish(E, [])


@pytest.mark.parametrize("nl", [3, 4])
def test_poisson_mg_coarse_levels_assembled_before_a_galerkin_preparation(ctx, nl):
    """assemble(l) on every coarse level (fused: macro rows of the REDISCRETISED operator in A[l] and in asm[l]'s partial-row buffer), then assemble() and
    prepare() with the Galerkin chain: the product for level l - 1 has asm[l] as its fine assembler and must read the Galerkin element rows the product for
    level l has just written, not the macro rows of the rediscretisation.  Again after a second prepare(), and after assemble(1) alone + prepare()."""
    oms, Ao, P, bdc = oracle_levels(nl, 7)
    right = chain(Ao[-1], P, bdc)
    # what the stale macro rows would give: level l - 1 from the rediscretised level l
    stale = [fo.zero_rows((P[l + 1].T @ Ao[l + 1] @ P[l + 1]).tocsr(), bdc[l], 1.0) for l in range(nl - 1)]
    assert_distinguishable(right, stale, range(nl - 2), TOL_COARSE, "rediscretised level below the top")
    pb = PoissonMG(ctx, 2, 2, 2, nl, meshes=device_meshes(nl, 7)).init()
    try:
        assert pb.gal_elem
        for l in range(nl - 1):
            pb.assemble(l)
            assert l == 0 or (pb.asm[l].fused_info()["active"] and pb.asm[l].last_path() == "fused")      # the levels that are the fine side of a product
        pb.assemble()
        assert pb.asm[-1].last_path() == "fused"
        pb.prepare()
        assert_operators(pb, right, range(nl - 1), "first prepare")
        pb.prepare()
        assert_operators(pb, right, range(nl - 1), "second prepare")
        pb.assemble(1)
        assert pb.asm[1].last_path() == "two-pass"      # by design: the product for level 0 has asked asm[1] for its element rows, the next assembly keeps them
        pb.prepare()
        assert_operators(pb, right, range(nl - 1), "after assemble(1)")
    finally:
        pb.destroy()


# ---- 2. the cached explicit transpose versus every writer ----------------------------------------------------------------------------------------
def w_mat_zero_rows(E):
    E["A"].mat_zero_rows(E["pb"].bdc[-1], 1.0)
    return fo.zero_rows(E["asm_sp"], E["bdc"][-1], 1.0), []


def w_index_zero_rows(E):
    E["pb"].bdc_dev[-1].zero_rows(E["A"], 1.0)
    return fo.zero_rows(E["asm_sp"], E["bdc"][-1], 1.0), []


T_WRITERS = dict(WRITERS, mat_zero_rows=w_mat_zero_rows, index_zero_rows=w_index_zero_rows)


def check_transpose(ctx, A, x, now, old, what):
    n_in, n_out = A.m(), A.n()
    xv, y = ctx.vector_from(x), ctx.vector(n_out)
    y.matrix_mult_transpose(xv, A)
    got = y.to_numpy()[:n_out].copy()
    xv.destroy(), y.destroy()
    ref = now.T @ x
    scale = max((abs(M).T @ abs(x)).max() for M in (now, old) if M is not None)       # (a zeroed matrix: the scale of what the cache may still hold)
    err = abs(got - ref).max() / scale
    print("%s: |A^T x - scipy| / max(|A|^T |x|) = %.2e" % (what, err))
    assert err <= TOL_SPMV, (what, err)
    if old is not None:
        assert abs(old.T @ x - ref).max() / scale > 1000 * TOL_SPMV, what
    At = A.get_transpose()
    T, want = At.to_scipy(), now.T.tocsr()
    At.destroy()
    want.sort_indices()
    assert T.shape == want.shape and abs(T - want).max() == 0.0, what


@pytest.mark.parametrize("writer", sorted(T_WRITERS))
def test_transposed_product_after_every_writer(ctx, writer):
    """matrix_mult_transpose caches the explicit transpose: after any writer of the values -- the Dirichlet-row replacement included -- the next product
    and get_transpose() follow the new values"""
    E = environment(ctx)
    objs = []
    try:
        x = fo.lcg_fill(E["n"], 17)
        check_transpose(ctx, E["A"], x, E["asm_sp"], None, "before")
        now, objs = T_WRITERS[writer](E)
        check_transpose(ctx, E["A"], x, E["A"].to_scipy(), E["asm_sp"], writer)
        assert abs(E["A"].to_scipy() - now).max() <= 1e-12 * max(abs(E["v0"]).max(), abs(now).max())
    finally:
        finish(E, objs)


@pytest.mark.parametrize("product", ["galerkin_from", "ptap_numeric", "abc_numeric"])
def test_transposed_product_after_a_product_is_made_again(ctx, product):
    """the coarse matrix of a product (element-wise Galerkin, sparse P^T A P, sparse A B C) after the product was repeated with other fine values"""
    E = environment(ctx)
    objs = []
    try:
        pb, top = E["pb"], 2
        Pd = ctx.matrix_scipy(E["P"][top])
        objs.append(Pd)
        if product == "galerkin_from":
            pb.level_operators()
            C, again = pb.A[top - 1], pb.level_operators
        elif product == "ptap_numeric":
            C = capi.Mat.ptap(Pd, E["A"])
            objs.append(C)
            again = lambda: C.ptap_numeric(Pd, E["A"])
        else:
            R = ctx.matrix_scipy(E["P"][top].T.tocsr())
            objs.append(R)
            C = capi.Mat.abc(R, E["A"], Pd)
            objs.append(C)
            again = lambda: C.abc_numeric(R, E["A"], Pd)
        x = fo.lcg_fill(C.m(), 23)
        old = C.to_scipy()
        check_transpose(ctx, C, x, old, None, "before")
        # other fine values: through the assembler for the element-wise product (it reads the assembler's rows), in the matrix for the sparse ones
        if product == "galerkin_from":
            objs.append(pb.asm[-1])
            pb.asm[-1] = capi.Assembler(ctx, None, FE, E["A"], elem_dof=E["ed"], coords=E["xy"] * np.array([1.0, 1.3, 0.8]))
            pb.assemble()
        else:
            E["A"].set_values(E["v0"] * (1.0 + 0.5 * fo.lcg_fill(E["v0"].size, 3)))
        again()
        check_transpose(ctx, C, x, C.to_scipy(), old, product)
    finally:
        finish(E, objs)


def _own_shape(ctx, kind):
    """(matrix, assemble(k) for two different inputs k = 0, 1, objects to destroy) for the assemblers that cannot target a scalar Q2 hex matrix"""
    m = capi.Mesh.box(3, 2, 0).refine()
    ed, xy, _ = m.arrays()
    xy = xy + np.random.default_rng(2).uniform(-0.01, 0.01, xy.shape)
    m.set_coords(xy)
    if kind in ("navier_stokes", "navier_stokes_stab"):
        nd, off, es = capi.system_elem_dofs(m, ["biquadratic", "biquadratic", "linear"] if kind == "navier_stokes" else ["linear"] * 3)
        n = int(off[-1])
        A = ctx.matrix_csr(n, n, *capi.pattern_from_elements(es, n))
        asm = (capi.NSAssembler if kind == "navier_stokes" else capi.NSStabAssembler)(ctx, m, A)
        res, sols = ctx.vector(n), [ctx.vector_from(0.3 * fo.lcg_fill(n, 50 + k)) for k in range(2)]
        return A, (lambda k: asm.assemble(A, res, sols[k], 0.05)), [asm, res] + sols + [m]
    n = m.nnode
    A = ctx.matrix_from_mesh(m, FE)
    res = ctx.vector(n)
    if kind == "advection_diffusion":
        asm = capi.AdvDiffAssembler(ctx, m, A)
        vel = [ctx.vector_from(fo.lcg_fill(2 * n, 60 + k)) for k in range(2)]
        return A, (lambda k: asm.assemble(A, res, None, vel[k], 0.1)), [asm, res] + vel + [m]
    xs = [xy, xy * np.array([1.0, 1.4])]
    if kind == "poisson_rows":
        return A, (lambda k: capi.assemble_poisson_rows(ctx, "quad", FE, ed, xs[k], A, res)), [res, m]
    if kind == "poisson_mixed":
        return A, (lambda k: capi.assemble_poisson_mixed(ctx, FE, ["quad"] * m.nel, ed, xs[k], A, res)), [res, m]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["navier_stokes", "navier_stokes_stab", "advection_diffusion", "poisson_rows", "poisson_mixed"])
def test_transposed_product_after_the_other_assemblers(ctx, kind):
    """the assemblers that write a matrix of their own shape (Taylor-Hood and stabilised Navier-Stokes, advection-diffusion, the generic Poisson rows on one
    and on mixed shapes): assemble, cache the transpose, assemble from other inputs -- the transposed product and get_transpose() follow what the matrix
    holds (that the assemblers leave the oracle's operator there is the subject of their own files)"""
    A, assemble, objs = _own_shape(ctx, kind)
    try:
        x = fo.lcg_fill(A.m(), 29)
        assemble(0)
        old = A.to_scipy()
        check_transpose(ctx, A, x, old, None, kind + " first")
        assemble(1)
        now = A.to_scipy()
        assert abs(now - old).max() > 1e-3 * abs(old).max()
        check_transpose(ctx, A, x, now, old, kind)
    finally:
        A.destroy()
        for o in objs:
            o.destroy()


def test_transposed_product_after_the_line_assembler(ctx):
    """fh_assemble_advdiff_line on a one-dimensional EDGE3 mesh"""
    nel = 12
    ed = np.array([[e, e + 1, nel + 1 + e] for e in range(nel)], np.int32)
    xs = np.concatenate([np.linspace(0, 1, nel + 1), (np.arange(nel) + 0.5) / nel])
    n = 2 * nel + 1
    A = ctx.matrix_csr(n, n, *capi.pattern_from_elements(ed, n))
    res = ctx.vector(n)
    try:
        x = fo.lcg_fill(n, 29)
        capi.assemble_advdiff_line(ctx, FE, ed, xs, A, res, 0.1, 1.0)
        old = A.to_scipy()
        check_transpose(ctx, A, x, old, None, "line first")
        capi.assemble_advdiff_line(ctx, FE, ed, xs, A, res, 0.3, -2.0)
        now = A.to_scipy()
        assert abs(now - old).max() > 1e-3 * abs(old).max()
        check_transpose(ctx, A, x, now, old, "line")
    finally:
        A.destroy(), res.destroy()


# ---- 3. a destroyed matrix -------------------------------------------------------------------------------------------------------------------------
def test_galerkin_product_after_the_assembled_matrix_was_destroyed(ctx):
    """fused assembly into A; A destroyed; B of the same pattern with other values created (it may get A's address): the product from the old assembler gives
    the operators of the ASSEMBLY (element rows made again) and touches neither the freed array nor B; after an assembly into B the product follows B"""
    E = environment(ctx)
    objs = []
    try:
        pb = E["pb"]
        right = chain(E["Ao"][-1], E["P"], E["bdc"])
        assert_distinguishable(right, chain(3.0 * E["Ao"][-1], E["P"], E["bdc"]), range(2), TOL_COARSE, "B")
        E["A"].destroy()
        B = ctx.matrix_csr(E["n"], E["n"], E["rp"], E["col"], 3.0 * E["v0"])
        pb.A[-1] = B
        pb.level_operators()
        assert_operators(pb, right, range(2), "after destroy")
        # now an assembly into B on other coordinates: the product follows it
        xy2 = E["xy"] * np.array([1.0, 1.3, 0.8])
        asm2 = capi.Assembler(ctx, None, FE, B, elem_dof=E["ed"], coords=xy2)
        objs.append(pb.asm[-1])
        pb.asm[-1] = asm2
        pb.assemble()
        assert asm2.last_path() == "fused"
        om = fo.Mesh("hex", E["ed"], xy2, None)
        right2 = chain(fo.assemble_poisson(om, FE, ONE)[0], E["P"], E["bdc"])
        assert_distinguishable(right2, right, range(2), TOL_COARSE, "second assembly")
        pb.level_operators()
        assert_operators(pb, right2, range(2), "after the assembly into B")
    finally:
        finish(E, objs)


# ---- 4. repeated fh_mg_setup with values that really change ----------------------------------------------------------------------------------------
class _H:
    pass


@functools.lru_cache(maxsize=None)
def hierarchy(which, nl=3):
    """"old": the curved hierarchy of seed 7; "new": the one of seed 11 with a non-constant coefficient by the row / column scaling D A D on every level --
    the same patterns, no common factor between the two.  nl = 2: its two finest levels (a coarsest level of 729 unknowns, 343 of them coupled)"""
    oms, Ao, P, bdc = oracle_levels(3, 7 if which == "old" else 11)
    H = _H()
    H.P = list(oracle_levels(3, 7)[2])
    H.A = chain(Ao[-1], P, bdc)
    if which == "new":
        for l, a in enumerate(H.A):
            d = sp.diags(1.0 + 0.5 * np.abs(fo.lcg_fill(a.shape[0], 40 + l)))
            H.A[l] = (d @ a @ d).tocsr()
    for a in H.A:
        a.sort_indices()
    if nl == 2:
        H.A, H.P = H.A[1:], [None, H.P[2]]
    H.coords0 = curved_coords(3, 7)[3 - nl]
    return H


OMEGA, NPRE, NPOST = 0.8, 2, 1


def ref_cycle(H, rhs, smoother, solver):
    """the oracle's cycle; for the exact level solve (LU_PRECOND) the same cycle with B = A^-1 by scipy's LU"""
    top = len(H.A) - 1
    if smoother != "lu":
        Hc = _H()
        Hc.A, Hc.P = H.A, H.P                    # (fo.vcycle keeps factors on the object it is given)
        return fo.vcycle(Hc, top, rhs, omega=OMEGA, npre=NPRE, npost=NPOST, smoother=smoother, level_solver=solver)
    import scipy.sparse.linalg as spla

    def cyc(l, b):
        lu = spla.splu(H.A[l].tocsc())
        if l == 0:
            return lu.solve(b)
        if solver == "gmres":
            sm = lambda xx, n, zg: fo.smooth_gmres(H.A[l], b, xx, n, zg, lu.solve)
        else:
            sm = lambda xx, n, zg: fo.smooth_precond(H.A[l], b, xx, OMEGA, n, zg, lu.solve)
        x = sm(np.zeros_like(b), NPRE, True)
        x = x + H.P[l] @ cyc(l - 1, H.P[l].T @ (b - H.A[l] @ x))
        return sm(x, NPOST, False)
    return cyc(top, rhs)


@functools.lru_cache(maxsize=None)
def oracle_cycle(which, nl, smoother, solver):
    H = hierarchy(which, nl)
    return ref_cycle(H, fo.lcg_fill(H.A[-1].shape[0], 9), smoother, solver)


SMOOTHERS = {"jacobi": capi.SMOOTH_JACOBI, "gs_color": capi.SMOOTH_GS_COLOR, "sor": capi.SMOOTH_SOR, "ilu0": capi.SMOOTH_ILU0, "identity": capi.SMOOTH_IDENTITY,
             "lu": capi.SMOOTH_LU}
COARSE_OPTIONS = {"dense": (), "dissected": (("coarse_nd_min", 16, 1024), ("coarse_direct", 0, 1)), "direct": (("coarse_direct", 2, 1),)}


class Solver:
    """a Multigrid over device copies of a hierarchy, with everything it made in one place to destroy"""

    def __init__(self, ctx, H, smoother, solver, coarse):
        self.ctx, self.nl, self.smoother, self.solver = ctx, len(H.A), smoother, solver
        self.mg = capi.Multigrid(ctx, self.nl)
        self.objs = [self.mg]
        if coarse != "dense":
            self.mg.set_coarse_coords(H.coords0)
        self.A, self.P = [None] * self.nl, [None] * self.nl
        for l in range(self.nl):
            self.install(l, H.A[l], H.P[l])
        self.mg.setup()

    def install(self, l, A, P):
        self.A[l] = self.ctx.matrix_scipy(A)
        self.P[l] = self.ctx.matrix_scipy(P) if P is not None else None
        self.objs += [o for o in (self.A[l], self.P[l]) if o is not None]
        self.mg.set_level(l, self.A[l], self.P[l], None, SMOOTHERS[self.smoother], OMEGA, NPRE, NPOST)
        if l > 0 and self.solver == "gmres":
            self.mg.set_level_solver(l, "gmres", 30)

    def cycle(self, rhs):
        b, x = self.ctx.vector_from(rhs), self.ctx.vector(rhs.size)
        self.objs += [b, x]
        self.mg.vcycle(b, x)
        return x.to_numpy().copy()

    def coarse_path(self):
        nden, nblk = self.mg.coarse_info()[:2]
        return nden, ("direct" if nblk < 0 else "dissected" if nblk >= 2 else "dense")

    def destroy(self):
        for o in self.objs:
            o.destroy()


def options(ctx, graph, reuse, coarse, restore=False):
    ctx.set_option("use_graph", 1 if restore else graph)
    ctx.set_option("mg_reuse_graph", 1 if restore else reuse)
    for name, value, back in COARSE_OPTIONS[coarse]:
        ctx.set_option(name, back if restore else value)


GRAPHS = [(1, 1), (1, 0), (0, 1), (0, 0)]
CASES = [("jacobi", "richardson", "dense"), ("gs_color", "richardson", "dense"), ("sor", "richardson", "dense"), ("ilu0", "richardson", "dense"),
         ("identity", "richardson", "dense"), ("lu", "richardson", "dense"), ("jacobi", "gmres", "dense"), ("sor", "gmres", "dense"), ("ilu0", "gmres", "dense"),
         ("lu", "gmres", "dense"), ("jacobi", "richardson", "dissected"), ("jacobi", "richardson", "direct"), ("ilu0", "gmres", "direct")]


@pytest.mark.parametrize("graph,reuse", GRAPHS)
@pytest.mark.parametrize("smoother,solver,coarse", CASES)
def test_second_setup_follows_operator_values_that_really_changed(ctx, smoother, solver, coarse, graph, reuse):
    """set up, cycle, replace the values of EVERY level operator by those of another hierarchy of the same pattern (no common factor: a stale diagonal,
    factor, coarse inverse or captured argument shows), set up again, cycle: bit for bit the cycle of a fresh solver on the new values, the oracle's
    cycle to 1e-11 -- and the old hierarchy's cycle is further than 1e-8 from it.  The dense inverse on the three-level hierarchy (27 coupled unknowns);
    the dissected inverse and the sparse exact solve on its two finest levels (343 coupled unknowns)"""
    nl = 3 if coarse == "dense" else 2
    ncoupled = 27 if nl == 3 else 343
    Ho, Hn = hierarchy("old", nl), hierarchy("new", nl)
    for a, b in zip(Ho.A, Hn.A):
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    ref_old, ref_new = oracle_cycle("old", nl, smoother, solver), oracle_cycle("new", nl, smoother, solver)
    assert rel(ref_old, ref_new) > 1000 * TOL_CYCLE
    rhs = fo.lcg_fill(Hn.A[-1].shape[0], 9)
    made = []
    options(ctx, graph, reuse, coarse)
    try:
        S = Solver(ctx, Ho, smoother, solver, coarse)
        made.append(S)
        assert S.coarse_path() == (ncoupled, coarse), S.mg.coarse_info()
        e0 = rel(S.cycle(rhs), ref_old)
        for l in range(nl):
            S.A[l].set_values(Hn.A[l].data)
        S.mg.setup()
        assert S.coarse_path() == (ncoupled, coarse), S.mg.coarse_info()
        again = S.cycle(rhs)
        F = Solver(ctx, Hn, smoother, solver, coarse)
        made.append(F)
        fresh = F.cycle(rhs)
        e1 = rel(again, ref_new)
        print("first setup %.2e, second setup %.2e from the oracle's cycle; bits equal to a fresh solver: %s" % (e0, e1, np.array_equal(again, fresh)))
        assert e0 < TOL_CYCLE
        assert np.array_equal(again, fresh)
        assert e1 < TOL_CYCLE
    finally:
        options(ctx, graph, reuse, coarse, restore=True)
        for S in made:
            S.destroy()


def on_pattern(M, A0):
    """M with the (larger) stored pattern of A0, zeros included: a fresh solver must get the pattern the reused one has"""
    M = M.tocsr()
    M.sort_indices()
    full = sp.csr_matrix((np.zeros(A0.nnz), A0.indices.copy(), A0.indptr.copy()), shape=A0.shape)
    pos = fo._csr_positions(A0.indptr, A0.indices, np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), M.indices)
    full.data[pos] = M.data
    return full


@pytest.mark.parametrize("coarse", ["dense", "dissected", "direct"])
def test_second_setup_follows_a_changed_dirichlet_set_on_the_coarsest_level(ctx, coarse):
    """between the setups more unknowns of level 0 are penalised (rows and columns zeroed, diagonal 1), then the first set again: the list of coupled
    unknowns, the size of the dense inverse and the dissection change under an unchanged matrix (same uid, same pattern)"""
    H = hierarchy("old", 2)
    A0 = H.A[0]
    offdiag = np.asarray(abs(A0).sum(axis=1)).ravel() - abs(A0.diagonal())
    coupled = np.where(offdiag > 0)[0]
    assert coupled.size == 343
    extra = coupled[::5].astype(np.int32)
    keep = np.ones(A0.shape[0])
    keep[extra] = 0.0
    big = on_pattern(sp.diags(keep) @ A0 @ sp.diags(keep) + sp.diags(1.0 - keep), A0)       # the larger Dirichlet set
    rhs = fo.lcg_fill(H.A[-1].shape[0], 9)
    Hs = {}
    for name, a0 in (("first", A0), ("larger", big)):
        Hs[name] = _H()
        Hs[name].A, Hs[name].P, Hs[name].coords0 = [a0, H.A[1]], H.P, H.coords0
    refs = {name: ref_cycle(Hs[name], rhs, "jacobi", "richardson") for name in Hs}
    assert rel(refs["first"], refs["larger"]) > 1000 * TOL_CYCLE
    made = []
    options(ctx, 1, 1, coarse)
    try:
        S = Solver(ctx, H, "jacobi", "richardson", coarse)
        made.append(S)
        for step, name, n_coupled in ((0, "first", 343), (1, "larger", 343 - extra.size), (2, "first", 343)):
            if step == 1:
                S.A[0].zero_cols(extra)
                S.A[0].mat_zero_rows(extra, 1.0)
                assert abs(S.A[0].to_scipy() - big).max() == 0.0
            elif step == 2:
                S.A[0].set_values(A0.data)
            if step:
                S.mg.setup()
            assert S.coarse_path() == (n_coupled, coarse), (name, S.mg.coarse_info())
            got = S.cycle(rhs)
            F = Solver(ctx, Hs[name], "jacobi", "richardson", coarse)
            made.append(F)
            fresh = F.cycle(rhs)
            err = rel(got, refs[name])
            print("%s (%d coupled): %.2e from the oracle's cycle; bits equal to a fresh solver: %s" % (name, n_coupled, err, np.array_equal(got, fresh)))
            assert np.array_equal(got, fresh), name
            assert err < TOL_CYCLE, name
    finally:
        options(ctx, 1, 1, coarse, restore=True)
        for S in made:
            S.destroy()


@pytest.mark.parametrize("smoother,solver", [("gs_color", "richardson"), ("sor", "richardson"), ("ilu0", "richardson"), ("ilu0", "gmres"), ("lu", "richardson")])
def test_second_setup_follows_another_pattern_installed_with_set_level(ctx, smoother, solver):
    """orderings, sweep schedules, the ILU(0) plan and the exact level solve's fronts belong to the pattern they were made for: another matrix of the same size
    and another pattern in the same solver object (the colouring test, widened to the natural-order sweeps, ILU(0) and the exact solve)"""
    Ha, Hnew = hierarchy("old", 2), hierarchy("new", 2)
    Ab = Hnew.A[1].tolil(copy=True)
    for r in range(0, Ab.shape[0], 3):                    # drop the couplings of every third row: another graph
        d = Ab[r, r]
        Ab[r, :] = 0.0
        Ab[r, r] = d
    Hb = _H()
    Hb.A, Hb.P, Hb.coords0 = [Hnew.A[0], Ab.tocsr()], Ha.P, Ha.coords0
    Hb.A[1].eliminate_zeros()
    Hb.A[1].sort_indices()
    assert Hb.A[1].nnz < Ha.A[1].nnz
    rhs = fo.lcg_fill(Ha.A[1].shape[0], 9)
    ref_a, ref_b = ref_cycle(Ha, rhs, smoother, solver), ref_cycle(Hb, rhs, smoother, solver)
    assert rel(ref_a, ref_b) > 1000 * TOL_CYCLE
    made = []
    try:
        S = Solver(ctx, Ha, smoother, solver, "dense")
        made.append(S)
        assert rel(S.cycle(rhs), ref_a) < TOL_CYCLE
        for l in range(2):
            S.install(l, Hb.A[l], Hb.P[l])
        S.mg.setup()
        got = S.cycle(rhs)
        F = Solver(ctx, Hb, smoother, solver, "dense")
        made.append(F)
        fresh = F.cycle(rhs)
        err = rel(got, ref_b)
        print("%s %s: %.2e from the oracle's cycle; bits equal to a fresh solver: %s" % (smoother, solver, err, np.array_equal(got, fresh)))
        assert np.array_equal(got, fresh)
        assert err < TOL_CYCLE
    finally:
        for S in made:
            S.destroy()


def _ns_setting(nl=3):
    """the small cavity of the block-smoother cases: oracle levels, boundary sets, two states of the finest level, a right-hand side"""
    from oracle import femus_oracle_ns as ns
    LO, HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
    ms, lays = ns.build_ns_levels(4, 4, 0, nl, LO, HI)
    bcs = [ns.cavity_bc(m, l) for m, l in zip(ms, lays)]
    top = nl - 1
    n = lays[top].n
    rng = np.random.default_rng(5)
    states = []
    for k in range(2):
        st = (0.3 + 0.4 * k) * rng.standard_normal(n)
        st[bcs[top][0]] = bcs[top][1]
        states.append(st)
    b = rng.standard_normal(n)
    b[bcs[top][0]] = 0.0
    return ns, ms, lays, bcs, states, b


def _cycle_of(ctx, mg, b):
    bv, x = ctx.vector_from(b), ctx.vector(b.size)
    try:
        mg.vcycle(bv, x)
        return x.to_numpy().copy()
    finally:
        bv.destroy(), x.destroy()


@pytest.mark.parametrize("smoother,coarse_level,graph,reuse", [("vanka", 0, 1, 1), ("asm", 0, 1, 1), ("vanka", 1, 1, 1), ("vanka", 0, 0, 0), ("vanka", 0, 1, 0),
                                                              ("asm", 0, 0, 0)])
def test_block_smoothers_follow_a_jacobian_that_really_changed(ctx, smoother, coarse_level, graph, reuse):
    """the patch inverses (Vanka), the ILU(0) factors of the blocks (PCASM) and the sparse LU of a raised coarsest level are made from the values: prepare the
    Navier-Stokes cycle at one state, cycle, prepare at another state (the assembler and the sparse Galerkin products rewrite every level operator of the
    same solver object), cycle: the bits of a fresh object at the second state, and -- full hierarchy -- the oracle's cycle at the tolerance of the existing
    tests of these smoothers (1e-9); the first state's cycle is more than 1000 tolerances away.  Also without the captured graph, and with a graph that is
    captured again at every setup"""
    from femus_amd.navier_stokes import NavierStokesMG
    nu, nl, top = 0.01, 3, 2
    ns, ms, lays, bcs, states, b = _ns_setting(nl)

    def new():
        pb = NavierStokesMG(ctx, 4, 4, 0, nl, nu).init()
        pb.smoother = capi.SMOOTH_VANKA if smoother == "vanka" else capi.SMOOTH_ASM
        pb.coarse_level = coarse_level
        return pb

    def cycle(pb, st):
        pb.SOL[top].upload(st)
        return _cycle_of(ctx, pb.prepare(top), b)

    made = []
    options(ctx, graph, reuse, "dense")
    try:
        pb, fresh = new(), new()
        made += [pb, fresh]
        first = cycle(pb, states[0])
        second = cycle(pb, states[1])
        want = cycle(fresh, states[1])
        assert np.isfinite(second).all() and rel(first, second) > 1000 * 1e-9
        assert np.array_equal(second, want)
        if coarse_level == 0:
            # (ILU(0) fills the allocated pattern: taken from the device operators, the values are the oracle's)
            pat = [pb.A[(top, l)].pattern() for l in range(nl)] if smoother == "asm" else None
            H = ns.newton_step_operators(ms, lays, bcs, top, states[1], nu, omega=pb.omega, npre=pb.npre, npost=pb.npost, smoother=smoother, patterns=pat)
            err = rel(second, ns.vcycle(H, top, b))
            print("%s: second preparation %.2e from the oracle's cycle" % (smoother, err))
            assert err < 1e-9
    finally:
        options(ctx, graph, reuse, "dense", restore=True)
        for o in made:
            o.destroy()


def padded(M):
    """M on a larger stored pattern (one more position in every row that lacks it, holding an explicit zero): the same operator, other CSR positions"""
    n = M.shape[0]
    ones = sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    extra = sp.coo_matrix((np.ones(n), (np.arange(n), (np.arange(n) * 7 + 3) % n)), shape=M.shape).tocsr()
    pat = (ones + extra).tocsr()
    pat.sort_indices()
    assert pat.nnz > M.nnz
    return on_pattern(M, pat)


@pytest.mark.parametrize("smoother", ["vanka", "asm"])
def test_block_smoothers_follow_another_pattern_installed_with_set_level(ctx, smoother):
    """the block smoothers keep the most pattern-derived state of all: per patch dof the positions {row, first, end} into A's CSR arrays, the patch descriptors
    and masks, the patch colouring, the masks of the block ILU(0).  Prepare the Navier-Stokes cycle at one state and cycle; then install, with set_level on the
    SAME Multigrid (its patches kept), the level operators of another state, the finest and the middle one on a PADDED pattern (another matrix, other CSR
    positions for every entry behind the first padding); set up and cycle: the bits of a fresh Multigrid given the same matrices and patches, and the
    oracle's cycle at the second state to 1e-9 (the padding holds zeros: the same operator; the block ILU(0) of PCASM fills the allocated pattern and the
    patch colouring of Vanka follows the stored graph, so the oracle is given the padded patterns for both)"""
    from femus_amd.navier_stokes import NavierStokesMG
    nu, nl, top = 0.01, 3, 2
    ns, ms, lays, bcs, states, b = _ns_setting(nl)
    code = capi.SMOOTH_VANKA if smoother == "vanka" else capi.SMOOTH_ASM
    made = []
    try:
        pbs = []
        for st in states:
            pb = NavierStokesMG(ctx, 4, 4, 0, nl, nu).init()
            made.append(pb)
            pb.smoother = code
            pb.SOL[top].upload(st)
            pb.prepare(top)
            pbs.append(pb)
        pb = pbs[0]
        mg = pb.mg[top]
        first = _cycle_of(ctx, mg, b)
        # the operators of the second state, levels 1 and 2 on padded patterns
        ops = [pbs[1].A[(top, l)].to_scipy() for l in range(nl)]
        ops = [ops[0]] + [padded(a) for a in ops[1:]]
        for l in range(1, nl):
            assert ops[l].nnz > pb.A[(top, l)].nnz
        dev = [ctx.matrix_scipy(a) for a in ops]
        made += dev

        def install(m):
            for l in range(nl):
                m.set_level(l, dev[l], pb.P[l] if l else None, None, code, pb.omega, pb.npre if l else 1, pb.npost if l else 0)
            m.setup()

        install(mg)
        got = _cycle_of(ctx, mg, b)
        fresh = capi.Multigrid(ctx, nl)
        made.append(fresh)
        for l in range(1, nl):
            fresh.set_level_patches(l, *pb.patches[l])
        install(fresh)
        want = _cycle_of(ctx, fresh, b)
        H = ns.newton_step_operators(ms, lays, bcs, top, states[1], nu, omega=pb.omega, npre=pb.npre, npost=pb.npost, smoother=smoother,
                                     patterns=[(a.indptr, a.indices) for a in ops] if smoother == "asm" else None)
        if smoother == "vanka":      # the order of the multiplicative sweep is the greedy patch colouring of the STORED graph: the oracle colours the padded one too
            for l in range(1, nl):
                sm = H.smoother[l]
                H.smoother[l] = ns.VankaSmoother(H.A[l], sm.patches, ns.color_patches(sm.patches, ops[l]), pb.omega)
        ref = ns.vcycle(H, top, b)
        err = rel(got, ref)
        print("%s: %.2e from the oracle's cycle; bits equal to a fresh solver: %s; first state's cycle %.2e away" % (smoother, err, np.array_equal(got, want), rel(first, ref)))
        assert rel(first, ref) > 1000 * 1e-9
        assert np.array_equal(got, want)
        assert err < 1e-9
    finally:
        for kind in (capi.Multigrid, NavierStokesMG, capi.Mat):      # solvers before the matrices they point to
            for o in made:
                if isinstance(o, kind):
                    o.destroy()


# ---- 5. NavierStokesMG.coarse_level changed between two preparations ------------------------------------------------------------------------------
def test_navier_stokes_coarse_level_changed_between_prepares(ctx):
    """mg[ig] is built for one coarse_level (its level count, the patch slots): prepare with 0, then 1, then 0 again on ONE object -- each cycle has the bits of
    the cycle of a fresh object prepared with that value, and the two values give different cycles"""
    from femus_amd.navier_stokes import NavierStokesMG
    ig = 2

    def cycle(ns):
        mg = ns.prepare(ig)
        rhs = fo.lcg_fill(ns.n[ig], 31)
        rhs[ns.bdc[ig]] = 0.0
        return _cycle_of(ctx, mg, rhs)

    fresh = {}
    for c in (0, 1):
        ns = NavierStokesMG(ctx, 2, 2, 0, 3, 0.1).init()
        ns.coarse_level = c
        fresh[c] = cycle(ns)
        ns.destroy()
    assert np.isfinite(fresh[0]).all() and rel(fresh[0], fresh[1]) > 1e-8
    ns = NavierStokesMG(ctx, 2, 2, 0, 3, 0.1).init()
    try:
        for c in (0, 1, 0):
            ns.coarse_level = c
            got = cycle(ns)
            assert np.array_equal(got, fresh[c]), (c, rel(got, fresh[c]))
    finally:
        ns.destroy()
