"""Geometry cache of the fused cluster assembly (option assemble_geom_cache; k_geom_cache + the cached instantiation of k_cluster_q2hex_sf): with a constant
source the cluster kernel reads D_q and det * w at the Gauss points from a cache the assembler makes at its first such assembly instead of computing them in
phase A.  The cached factors are what phase A returns, so matrix and residual must have the BITS of the in-kernel path -- on one cluster, on boundary and
interior clusters, with and without carried rows, with and without a solution vector -- and the oracle's values to 1e-12; the cache belongs to the assembler,
holds nothing of the source, and follows the option from one assembly to the next."""
import numpy as np
import pytest
import scipy.sparse as sp

from femus_amd import capi
from oracle import femus_oracle as fo

pytestmark = pytest.mark.gpu

# curved refined meshes: 1 cluster (every row complete), 2, 12 clusters (boundary clusters), 64 clusters (interior clusters)
MESHES = [((1, 1, 1), 2), ((2, 1, 1), 2), ((3, 2, 2), 2), ((2, 2, 2), 3)]
CARRY = [0, 1, 2]       # clusters per super-cluster 1, 2, 4 (fewer where the cluster count is no multiple): the kernel without and with carried rows
P0 = 1.5

_setup, _runs = {}, {}


def setup(args, nl, seed=3):
    key = (args, nl, seed)
    if key not in _setup:
        m = capi.Mesh.box(*args)
        for _ in range(nl - 1):
            m = m.refine()
        ed, xy, _ = m.arrays()
        rng = np.random.default_rng(seed)
        xy = xy + rng.uniform(-0.01, 0.01, xy.shape) / 2 ** (nl - 1)
        rp, col = capi.pattern_from_elements(ed, m.nnode)
        u = rng.uniform(-1, 1, m.nnode)
        _setup[key] = (m, ed, xy, rp, col, u)
    return _setup[key]


def run(ctx, s, calls, carry=-1, with_sol=True, order="seventh", xy=None):
    """One assembler; calls = [(assemble_geom_cache, source kind, params)], each from NaN-filled arrays with debug_poison 1.
    Returns [(values, residual, geom_cache_info after the call)]."""
    m, ed, xy0, rp, col, u = s
    xy = xy0 if xy is None else xy
    n = m.nnode
    out = []
    ctx.set_option("assemble_carry", carry)
    ctx.set_option("debug_poison", 1)
    try:
        A = ctx.matrix_csr(n, n, rp, col, np.full(col.size, np.nan))
        res = ctx.vector_from(np.full(n, np.nan))
        asm = capi.Assembler(ctx, m, "biquadratic", A, order=order, elem_dof=ed, coords=xy)
        assert asm.fused_info()["active"] == (order == "seventh")
        assert asm.geom_cache_info() == {"active": False, "bytes": 0}          # nothing is made at create
        sol = ctx.vector_from(u) if with_sol else None
        for geom, kind, params in calls:
            ctx.set_option("assemble_geom_cache", geom)
            A.set_values(np.full(col.size, np.nan))
            res.upload(np.full(n, np.nan))
            asm.assemble(A, res, sol, kind, params)
            out.append((A.values().copy(), res.to_numpy().copy(), asm.geom_cache_info()))
        asm.destroy(), A.destroy()
    finally:
        ctx.set_option("assemble_geom_cache", 1)
        ctx.set_option("debug_poison", 0)
        ctx.set_option("assemble_carry", -1)
    return out


def twice(ctx, args, nl, carry, with_sol, geom):
    """constant source, assembled twice with one setting of the option (shared by the tests below)"""
    key = (args, nl, carry, with_sol, geom)
    if key not in _runs:
        _runs[key] = run(ctx, setup(args, nl), [(geom, 0, (P0,))] * 2, carry, with_sol)
    return _runs[key]


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("with_sol", [True, False])
@pytest.mark.parametrize("carry", CARRY)
@pytest.mark.parametrize("args,nl", MESHES)
def test_cached_assembly_has_the_bits_of_the_in_kernel_phase_a(ctx, args, nl, carry, with_sol):
    m = setup(args, nl)[0]
    cached, plain = twice(ctx, args, nl, carry, with_sol, 1), twice(ctx, args, nl, carry, with_sol, 0)
    for v, f, _ in cached + plain:
        assert np.isfinite(v).all() and np.isfinite(f).all()
    assert same_bits(cached[0], plain[0])
    assert same_bits(cached[1], cached[0]) and same_bits(plain[1], plain[0])         # again, from poisoned buffers
    for _, _, info in cached:
        assert info == {"active": True, "bytes": m.nel * 7 * 64 * 8}
    for _, _, info in plain:
        assert info == {"active": False, "bytes": 0}


_oracle = {}


def oracle_global(args, nl, with_sol):
    key = (args, nl, with_sol)
    if key not in _oracle:
        m, ed, xy, rp, col, u = setup(args, nl)
        n = m.nnode
        uu = u if with_sol else np.zeros(n)
        et = fo.ElemType("hex", "biquadratic", "seventh")
        Ko, Fo = fo.elem_poisson_batch(et, np.transpose(xy[ed], (0, 2, 1)), uu[ed], lambda xg: P0 * np.ones(xg.shape[:2]))
        rows = np.repeat(ed, 27, axis=1).ravel()
        cols = np.tile(ed, (1, 27)).ravel()
        Ao = sp.coo_matrix((Ko.ravel(), (rows, cols)), shape=(n, n)).tocsr()
        Ao.sort_indices()
        bo = np.zeros(n)
        np.add.at(bo, ed.ravel(), Fo.ravel())
        assert np.array_equal(Ao.indptr, rp) and np.array_equal(Ao.indices, col)
        _oracle[key] = (Ao, bo)
    return _oracle[key]


@pytest.mark.parametrize("with_sol", [True, False])
@pytest.mark.parametrize("carry", CARRY)
@pytest.mark.parametrize("args,nl", MESHES)
def test_cached_assembly_matches_the_oracle(ctx, args, nl, carry, with_sol):
    """the oracle's element loop; bounds of the fused test: 1e-12 of each row's largest entry, 1e-12 of the largest residual entry"""
    rp = setup(args, nl)[3]
    Ao, bo = oracle_global(args, nl, with_sol)
    v, f, info = twice(ctx, args, nl, carry, with_sol, 1)[0]
    assert info["active"]
    row_scale = np.repeat(np.maximum.reduceat(abs(Ao.data), rp[:-1]), np.diff(rp))
    assert (abs(v - Ao.data) / row_scale).max() <= 1e-12
    assert abs(f - bo).max() <= 1e-12 * abs(bo).max()


def test_cache_belongs_to_the_assembler_not_the_mesh(ctx):
    """two assemblers on one mesh with different coordinates, assembled alternately: each has the bits of its own uncached twin"""
    s = setup((3, 2, 2), 2)
    m, ed, xy, rp, col, u = s
    n = m.nnode
    xyB = xy + np.random.default_rng(11).uniform(-0.01, 0.01, xy.shape) / 2
    ref = {k: run(ctx, s, [(0, 0, (P0,))], xy=c)[0] for k, c in (("A", xy), ("B", xyB))}
    assert not same_bits(ref["A"], ref["B"])
    ctx.set_option("debug_poison", 1)
    try:
        objs = {}
        for k, c in (("A", xy), ("B", xyB)):
            A = ctx.matrix_csr(n, n, rp, col, np.full(col.size, np.nan))
            objs[k] = (capi.Assembler(ctx, m, "biquadratic", A, elem_dof=ed, coords=c), A, ctx.vector_from(np.full(n, np.nan)))
        sol = ctx.vector_from(u)
        for k in ("A", "B", "A", "B", "B", "A"):
            asm, A, res = objs[k]
            A.set_values(np.full(col.size, np.nan))
            res.upload(np.full(n, np.nan))
            asm.assemble(A, res, sol, 0, (P0,))
            assert asm.geom_cache_info()["active"]
            assert same_bits((A.values(), res.to_numpy()), ref[k])
        for asm, A, _ in objs.values():
            asm.destroy(), A.destroy()
    finally:
        ctx.set_option("debug_poison", 0)


def test_source_parameters_are_not_cached(ctx):
    """constant 1.5, then a source that depends on x (in-kernel path), then constant -0.75 on ONE assembler: each call has the bits of the uncached call"""
    s = setup((3, 2, 2), 2)
    seq = [(0, (1.5,)), (1, (2.0, 1.3)), (0, (-0.75,))]
    cached = run(ctx, s, [(1, k, p) for k, p in seq])
    plain = run(ctx, s, [(0, k, p) for k, p in seq])
    for a, b in zip(cached, plain):
        assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all() and same_bits(a, b)
    assert not same_bits(cached[0], cached[2])
    assert all(info["active"] for _, _, info in cached) and not any(info["active"] for _, _, info in plain)


def test_option_toggled_between_assemblies(ctx):
    """1, 0, 1 on one assembler: every result has the reference bits; the cache, once made, stays with the assembler while the option is off"""
    s = setup((2, 2, 2), 3)
    ref = twice(ctx, (2, 2, 2), 3, -1, True, 0)[0]
    got = run(ctx, s, [(1, 0, (P0,)), (0, 0, (P0,)), (1, 0, (P0,))])
    for g in got:
        assert same_bits(g, ref)
        assert g[2] == {"active": True, "bytes": s[0].nel * 7 * 64 * 8}


def test_assembler_without_a_fused_plan_has_no_cache(ctx):
    """125 Gauss points: no fused plan, so no cache is made, and the assembly is what it is with the option off"""
    s = setup((2, 1, 1), 2)
    on = run(ctx, s, [(1, 0, (P0,))], order="ninth")[0]
    off = run(ctx, s, [(0, 0, (P0,))], order="ninth")[0]
    assert on[2] == {"active": False, "bytes": 0}
    assert np.isfinite(on[0]).all() and np.isfinite(on[1]).all() and same_bits(on, off)
