"""The fused cluster assembly reads ONE 16-byte plan word per thread and cluster (k_cluster_maps: the slot's informative byte m, a class bit per slot,
the flags of the carried entries); the cluster kernel and k_galerkin_macro decode entry = class ? p : m, position = class ? m : p.  Checked at the
smallest shapes where that decode can go wrong: one cluster (complete rows only), one super-cluster of 64 clusters, 512 clusters in several
super-clusters (complete, carried and partial rows in one cluster), and the last mesh with its dofs renumbered at random, so that neither the entry nor
the position of a slot equals p anywhere.  Tolerances: the ones of test_gpu_fused_assembly.py."""
import concurrent.futures
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from femus_amd import capi
from oracle import femus_oracle as fo

pytestmark = pytest.mark.gpu

SRC = 1.5                     # constant source: the instantiation that reads the geometry cache (the flagship's)
MESHES = {"one": ((1, 1, 1), 2), "super": ((1, 1, 1), 4), "many": ((2, 2, 2), 4), "permuted": ((2, 2, 2), 4)}


@functools.lru_cache(maxsize=None)
def hierarchy(args, nl):
    ms = [capi.Mesh.box(*args)]
    for _ in range(nl - 1):
        ms.append(ms[-1].refine())
    return ms


@functools.lru_cache(maxsize=None)
def geometry(args, nl):
    """curved fine mesh, solution vector and the oracle's operator in the mesh's own numbering (made once per mesh, never written to)"""
    m = hierarchy(args, nl)[-1]
    ed, xy, _ = m.arrays()
    rng = np.random.default_rng(17)
    xy = xy + rng.uniform(-0.01, 0.01, xy.shape) / 2 ** (nl - 1)
    n = m.nnode
    u = rng.uniform(-1, 1, n)
    et = fo.ElemType("hex", "biquadratic", "seventh")
    X, U = np.transpose(xy[ed], (0, 2, 1)), u[ed]
    chunks = [slice(k, k + 512) for k in range(0, ed.shape[0], 512)]         # elements are independent: the oracle's loop, a few chunks side by side
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        parts = list(pool.map(lambda s: fo.elem_poisson_batch(et, X[s], U[s], lambda xg: SRC * np.ones(xg.shape[:2])), chunks))
    Ko, Fo = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return m, ed, xy, u, Ko, Fo


@functools.lru_cache(maxsize=None)
def case(name):
    """(mesh, element dofs, coordinates, n, rowptr, col, u, oracle matrix, oracle residual, permutation) of a named mesh"""
    args, nl = MESHES[name]
    m, ed, xy, u, Ko, Fo = geometry(args, nl)
    n = m.nnode
    perm = np.arange(n)
    if name == "permuted":        # new number of node k = perm[k]: the mesh as arrays, nothing about the numbering left
        perm = np.random.default_rng(23).permutation(n)
        ed = perm[ed].astype(np.int32)
        xy2, u2 = np.empty_like(xy), np.empty_like(u)
        xy2[perm], u2[perm] = xy, u
        xy, u = xy2, u2
    rp, col = capi.pattern_from_elements(ed, n)
    Ao = sp.coo_matrix((Ko.ravel(), (np.repeat(ed, 27, axis=1).ravel(), np.tile(ed, (1, 27)).ravel())), shape=(n, n)).tocsr()
    Ao.sort_indices()
    bo = np.zeros(n)
    np.add.at(bo, ed.ravel(), Fo.ravel())
    assert np.array_equal(Ao.indptr, rp) and np.array_equal(Ao.indices, col)
    for a in (ed, xy, u, rp, col, Ao.data, bo, perm):
        a.setflags(write=False)
    return m, ed, xy, n, rp, col, u, Ao, bo, perm


def assemble_twice(ctx, name, fused=1, carry=0, geom_cache=1):
    """two assemblies from NaN-poisoned value, residual and partial-row buffers; returns (values, residual, fused_info, plan_info)"""
    m, ed, xy, n, rp, col, u, _, _, _ = case(name)
    ctx.set_option("assemble_fused", fused)
    ctx.set_option("assemble_carry", carry)
    ctx.set_option("assemble_geom_cache", geom_cache)
    ctx.set_option("debug_poison", 1)
    try:
        A = ctx.matrix_csr(n, n, rp, col, np.full(col.size, np.nan))
        res = ctx.vector_from(np.full(n, np.nan))
        asm = capi.Assembler(ctx, m, "biquadratic", A, elem_dof=ed, coords=xy)
        fi, pi = asm.fused_info(), asm.plan_info()
        sol = ctx.vector_from(u)
        asm.assemble(A, res, sol, 0, (SRC,))
        v, f = A.values().copy(), res.to_numpy().copy()
        A.set_values(np.full(col.size, np.nan))
        res.upload(np.full(n, np.nan))
        asm.assemble(A, res, sol, 0, (SRC,))
        v2, f2 = A.values(), res.to_numpy()
        assert np.array_equal(v.view(np.uint64), v2.view(np.uint64)) and np.array_equal(f.view(np.uint64), f2.view(np.uint64))
        assert asm.last_path() == ("fused" if fused else "two-pass")
        asm.destroy(), A.destroy()
    finally:
        ctx.set_option("debug_poison", 0)
        ctx.set_option("assemble_geom_cache", 1)
        ctx.set_option("assemble_carry", -1)
        ctx.set_option("assemble_fused", 1)
    return v, f, fi, pi


@pytest.mark.parametrize("name,carry", [("one", 3), ("super", 6), ("many", 6), ("permuted", 3), ("permuted", 6)])
def test_one_plan_word_assembles_the_bits_of_the_plan_without_carried_rows(ctx, name, carry):
    """matrix and residual with carried rows are bitwise equal to those with assemble_carry off and to a second assembly; both equal the two-pass path and
    the oracle at the tolerances of test_gpu_fused_assembly.py; every plan, carried or not, holds clusters x 512 x 16 bytes of plan words"""
    m, ed, xy, n, rp, col, u, Ao, bo, _ = case(name)
    ncl = ed.shape[0] // 8
    vc, fc, fic, pic = assemble_twice(ctx, name, carry=carry)
    v0, f0, fi0, pi0 = assemble_twice(ctx, name, carry=0)
    v2, f2, fi2, _ = assemble_twice(ctx, name, fused=0)
    assert fic["active"] and fi0["active"] and not fi2["active"]
    assert fic["clusters"] == ncl and fi0["clusters"] == ncl
    for pi in (pic, pi0):
        assert pi == {"map_bytes": ncl * 512 * 16, "bytes_per_cluster": 512 * 16}
    assert fi0["clusters_per_super"] == 1 and fi0["carried_entries"] == 0
    if name == "one":         # a single cluster cannot be grouped: every row is complete, no class bit is set
        assert fic["clusters_per_super"] == 1 and fic["partial_entries"] == 0
    else:
        assert fic["clusters_per_super"] == (1 << carry) and fic["carried_entries"] > 0
        assert (fic["partial_entries"] > 0) == (name != "super")        # one super-cluster: nothing is left for the partial-row buffer
        assert fic["partial_entries"] < fi0["partial_entries"]
    assert np.isfinite(vc).all() and np.isfinite(fc).all()
    assert np.array_equal(vc.view(np.uint64), v0.view(np.uint64)) and np.array_equal(fc.view(np.uint64), f0.view(np.uint64))
    if name == "permuted":    # the instantiation that computes phase A itself reads the same word
        vg, fg, _, pig = assemble_twice(ctx, name, carry=carry, geom_cache=0)
        assert pig == pic
        assert np.array_equal(vc.view(np.uint64), vg.view(np.uint64)) and np.array_equal(fc.view(np.uint64), fg.view(np.uint64))
    if name == "many":        # assemble_carry 200 + k (measurement aid): the CARRY kernel walks 2^k clusters on a plan WITHOUT carried rows -- no class bit to decode
        va, fa, fia, pia = assemble_twice(ctx, name, carry=206)
        assert fia["active"] and fia["clusters_per_super"] == 1 and fia["carried_entries"] == 0 and pia == pi0
        assert np.array_equal(va.view(np.uint64), v0.view(np.uint64)) and np.array_equal(fa.view(np.uint64), f0.view(np.uint64))
    row_scale = np.repeat(np.maximum.reduceat(abs(Ao.data), rp[:-1]), np.diff(rp))
    for v, f in ((vc, fc), (v2, f2)):
        err_v, err_f = (abs(v - Ao.data) / row_scale).max(), abs(f - bo).max() / abs(bo).max()
        print("%s carry %d: against the oracle, matrix %.2e (row-scaled), residual %.2e" % (name, carry, err_v, err_f))
        assert err_v <= 1e-12
        assert err_f <= 1e-12
    d_v, d_f = abs(vc - v2).max() / abs(Ao.data).max(), abs(fc - f2).max() / abs(bo).max()
    print("%s carry %d: against the two-pass path, matrix %.2e, residual %.2e" % (name, carry, d_v, d_f))
    assert d_v <= 4e-16
    assert d_f <= 1e-15


def test_galerkin_from_one_plan_word_on_a_renumbered_mesh(ctx):
    """fh_assembler_galerkin from the macro rows (k_galerkin_macro: entry and position of every slot from the one word, a carried entry read in the cluster
    that made the last contribution) equals the element-wise product from the element rows, on the renumbered mesh, with and without carried rows"""
    m, ed, xy, n, rp, col, u, _, _, perm = case("permuted")
    mc = hierarchy(*MESHES["permuted"])[-2]
    child = mc.child_elems()
    fb = perm[m.dirichlet_dofs("biquadratic")].astype(np.int32)
    cb = mc.dirichlet_dofs("biquadratic")
    got = {}
    for macro, carry in ((0, 0), (1, 0), (1, 3), (1, 6)):
        ctx.set_option("galerkin_macro", macro)
        ctx.set_option("assemble_carry", carry)
        try:
            A = ctx.matrix_csr(n, n, rp, col)
            res = ctx.vector(n)
            fas = capi.Assembler(ctx, m, "biquadratic", A, elem_dof=ed, coords=xy)
            Ac = ctx.matrix_from_mesh(mc, "biquadratic")
            cas = capi.Assembler(ctx, mc, "biquadratic", Ac)
            fi = fas.fused_info()
            assert fi["active"] and fi["clusters_per_super"] == (1 << carry)
            sol = ctx.vector_from(u)
            fas.assemble(A, res, sol, 0, (SRC,))
            assert fas.last_path() == "fused"
            cas.galerkin_from(fas, child, fb, cb, Ac)
            got[(macro, carry)] = Ac.to_scipy()
            fas.assemble(A, res, sol, 0, (SRC,))
            # the macro rows served the product: nobody asked for the element rows, the assembler stays on the fused path
            assert fas.last_path() == ("fused" if macro else "two-pass")
            cas.destroy(), fas.destroy(), Ac.destroy(), A.destroy()
        finally:
            ctx.set_option("galerkin_macro", 1)
            ctx.set_option("assemble_carry", -1)
    ref = got[(0, 0)]
    assert abs(ref).max() > 0
    for key in ((1, 0), (1, 3), (1, 6)):
        d = abs(got[key] - ref).max() / abs(ref).max()
        print("galerkin macro rows, carry %d: against the element-wise product %.2e" % (key[1], d))
        assert d <= 1e-13
