"""mixed_mesh.refine_flagged / flag_elements and app_poisson._prolongator_from_links: the host statement of the selective refinement of an element mesh of any
shape and of the transfer into the flagged level -- the yardsticks of the device side (tests/test_gpu_element_mesh_flagged.py, which imports the chains from
here).  On boxes of quadrilaterals and hexahedra the rule is held against oracle/femus_oracle_amr.py (refine_flagged, build_prolongator); on the meshes of
tests/golden against its own edge cases (all flagged == refine, none flagged == the input), conservation, and what the transfer must reproduce.  No device;
the FE tables come from the built library, as for mixed_mesh itself.  Chains are computed once per mesh and shared, read-only.

Bound on coordinates and transfers, DERIVED: a new node's coordinate is a sum of at most 27 products w * x with |w| <= 1; two correctly rounded evaluations of
it in different orders differ by at most 2 * 27 * eps * max|x| < 64 * eps * max|x|."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from femus_amd import app_poisson as app
from femus_amd import capi, mixed_mesh
from oracle import femus_oracle as fo
from oracle import femus_oracle_amr as foa
from test_element_transfer_host import FAM, _Builder, groups_of
from test_gpu_element_mesh import MESHES, THREE_D, coarse

EPS = np.finfo(np.float64).eps
BOXES = [(3, 2, 0), (2, 2, 2)]


def ex4(x, level):
    """SetRefinementFlag of applications/MGAMR/ex4/ex4.cpp:49-62"""
    if level == 0:
        return x[0] > 0
    if level == 1:
        return x[0] > 0 and x[1] > -0.25
    return False


EX4 = "if(level<0.5, x>0, if(level<1.5, (x>0)&(y>-0.25), 0))"          # the same over x,y,z,level for capi.Expr


def level_flags(mesh, lev, level, fn=ex4, seed=0):
    """fn where it separates the elements of the level, otherwise a seeded random half of them; on a level above 0 some elements of older levels are named
    as well (the rule must leave them alone)"""
    kind, ed, xs = mesh[0], mesh[1], mesh[2]
    flags = mixed_mesh.flag_elements(kind, ed, xs, lev, level, fn)
    cur = lev == level
    if flags[cur].all() or not flags.any():
        flags = np.zeros(kind.shape[0], dtype=np.uint8)
        pick = np.random.default_rng(seed + level).permutation(np.nonzero(cur)[0])
        flags[pick[:max(1, pick.size // 2)]] = 1
    assert flags[cur].any() and not flags[cur].all() and not flags[~cur].any()
    old = np.nonzero(~cur)[0]
    flags[old[::2]] = 1
    return flags


def frozen(level):
    for a in level:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return level


def flagged_chain_of(mesh, n=2, fn=ex4):
    """[(kind, ed, xs, ff, own, lev, father, child, flags used to get here)] of levels 0 .. n"""
    nel = mesh[0].shape[0]
    out = [frozen(tuple(mesh[:4]) + (list(mesh[4]), np.zeros(nel, dtype=np.int64), np.full(nel, -1), np.full(nel, -1), None))]
    for level in range(n):
        c = out[-1]
        flags = level_flags(c, c[5], level, fn)
        f = mixed_mesh.refine_flagged(c[0], c[1], c[2], c[3], flags, c[5], level)
        out.append(frozen(f[:4] + (list(f[4]),) + f[5:] + (flags,)))
    return out


@functools.lru_cache(maxsize=None)
def flagged_chain(name, distorted):
    return flagged_chain_of(coarse(name, distorted))


def off_the_chords(mesh):
    """the largest distance of an edge node from the middle of its two vertices"""
    kind, ed, xs = mesh[0], mesh[1], mesh[2]
    d = 0.0
    for s in sorted(set(kind.tolist())):
        nv, E, rows = mixed_mesh.CLASSES[s][0], np.array(mixed_mesh.tables(s)["edges"]), ed[kind == s]
        d = max(d, float(np.abs(xs[rows[:, nv:nv + len(E)]] - 0.5 * (xs[rows[:, E[:, 0]]] + xs[rows[:, E[:, 1]]])).max()))
    return d


@functools.lru_cache(maxsize=None)
def straight_chain(name):
    """the flagged chain of a mesh as read whose edge nodes are the middles of their chords in double precision -- where the linear family must reproduce the
    coordinates.  The files with short decimals are; cube_Tet.neu stores 12 digits and its middles lie 5.0e-13 off the chords, which is all the linear transfer
    then misses: for it the middles are put on the chords and the nodes the reader adds (faces, centres) are summed again with the reader's weights"""
    mesh = coarse(name, False)
    d0 = off_the_chords(mesh)
    if d0 == 0.0:
        return flagged_chain(name, False)
    kind, ed, xs, ff, own = mesh
    assert d0 < 1e-12 and set(kind.tolist()) <= set(mixed_mesh.ADDED)
    xs = np.array(xs)
    for e in range(kind.shape[0]):
        s = kind[e]
        nv, W = mixed_mesh.CLASSES[s][0], mixed_mesh.ADDED[s]
        for m, (a, b) in enumerate(mixed_mesh.tables(s)["edges"]):
            xs[ed[e, nv + m]] = 0.5 * (xs[ed[e, a]] + xs[ed[e, b]])
        j0 = mixed_mesh.NLOC[s] - W.shape[0]
        for j in range(W.shape[0]):
            acc = np.zeros(xs.shape[1])
            for i in range(j0):
                acc += xs[ed[e, i]] * W[j][i]
            xs[ed[e, j0 + j]] = acc
    xs.setflags(write=False)
    assert off_the_chords((kind, ed, xs)) == 0.0
    return flagged_chain_of((kind, ed, xs, ff, own))


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def host_prolongator_links(fe, c, f):
    """(rowptr, col, val) of app_poisson._prolongator_from_links between two levels of a flagged chain, caught on its way to capi.Mat.from_csr"""
    got = []
    keep = capi.Mat.__dict__["from_csr"]
    capi.Mat.from_csr = classmethod(lambda cls, ctx, m, n, rowptr, col, val=None: got.append((int(m), int(n), np.array(rowptr), np.array(col), np.array(val))))
    try:
        app.Poisson001._prolongator_from_links(_Builder(fe), groups_of(c[0], fe), c[1], f[1], c[4][FAM[fe]], f[4][FAM[fe]], f[6], f[7])
    finally:
        capi.Mat.from_csr = keep
    (m, n, rowptr, col, val), = got
    assert (m, n) == (f[4][FAM[fe]], c[4][FAM[fe]]) and rowptr.shape == (m + 1,) and rowptr[-1] == col.size == val.size
    return rowptr.astype(np.int64), col.astype(np.int64), val.astype(np.float64)


# ---- 1. against the oracle on boxes ---------------------------------------------------------------------------------------------------------------------
def as_mixed(mo):
    ed = np.full((mo.nel, 27), -1, dtype=np.int64)
    ed[:, :mo.elem_dof.shape[1]] = mo.elem_dof
    ff = np.full((mo.nel, 6), -1, dtype=np.int64)
    ff[:, :mo.face_flag.shape[1]] = mo.face_flag
    return np.full(mo.nel, mo.geom), ed, mo.coords.copy(), ff


def box_flags(mo, step):
    """level 0: the right part of the box; level 1: every second element, older ones among them"""
    if step == 0:
        return foa.elem_centroids(mo)[:, 0] > 0.4
    flags = np.zeros(mo.nel, dtype=bool)
    flags[::2] = True
    lev = foa.elem_levels(mo)
    assert (flags & (lev < mo.level)).any() and (flags & (lev == mo.level)).any() and not flags[lev == mo.level].all()
    return flags


@functools.lru_cache(maxsize=None)
def box_chains(box):
    mo = fo.coarse_box_mesh(*box)
    mo.elem_level = np.zeros(mo.nel, dtype=np.int64)
    ours = [as_mixed(mo) + (list(mo.own_size), mo.elem_level.copy(), None, None)]
    theirs = [mo]
    for step in range(2):
        flags = box_flags(theirs[-1], step)
        theirs.append(foa.refine_flagged(theirs[-1], flags))
        c = ours[-1]
        ours.append(mixed_mesh.refine_flagged(c[0], c[1], c[2], c[3], flags, c[5], step))
    return ours, theirs


@pytest.mark.parametrize("box", BOXES, ids=["quad_3x2", "hex_2x2x2"])
def test_two_flagged_levels_equal_the_oracle_on_boxes(box):
    ours, theirs = box_chains(box)
    for level, (m, mo) in enumerate(zip(ours, theirs)):
        w, nf = mo.elem_dof.shape[1], mo.face_flag.shape[1]
        print("%s level %d: %d elements, %d nodes, own %s" % (mo.geom, level, mo.nel, mo.nnode, list(m[4])))
        assert np.array_equal(m[1][:, :w], mo.elem_dof) and (m[1][:, w:] == -1).all()
        assert np.array_equal(m[3][:, :nf], mo.face_flag) and (m[3][:, nf:] == -1).all()
        assert list(m[4]) == [int(k) for k in mo.own_size]
        assert np.array_equal(m[5], foa.elem_levels(mo))
        assert m[2].shape == mo.coords.shape and np.abs(m[2] - mo.coords).max() <= 64 * EPS * np.abs(mo.coords).max()
    assert 0 < (ours[1][7] < 0).sum() < ours[1][0].shape[0] and (ours[2][5] == 0).any() and (ours[2][5] == 2).any()


def test_the_quadrilateral_box_counts():
    """figures of the oracle side alone, stated in the issue: all 6 flagged -> 24 elements, 117 nodes, own [35, 93, 117]; 4 of 6 -> 18 elements, 93 nodes"""
    mo = fo.coarse_box_mesh(3, 2, 0)
    kind, ed, xs, ff = as_mixed(mo)
    a = mixed_mesh.refine_flagged(kind, ed, xs, ff, np.ones(6, dtype=np.uint8))
    assert (a[0].shape[0], a[2].shape[0], list(a[4])) == (24, 117, [35, 93, 117])
    four = np.array([1, 1, 1, 0, 1, 0], dtype=bool)            # the lower row and the middle of the upper one: three edges between flagged elements
    b = mixed_mesh.refine_flagged(kind, ed, xs, ff, four)
    assert (b[0].shape[0], b[2].shape[0]) == (18, 93)
    fo_b = foa.refine_flagged(mo, four)
    assert (fo_b.nel, fo_b.nnode) == (18, 93)


@pytest.mark.parametrize("fe", ["linear", "biquadratic"])
@pytest.mark.parametrize("box", BOXES, ids=["quad_3x2", "hex_2x2x2"])
def test_the_transfer_equals_the_oracle_s_on_boxes(box, fe):
    ours, theirs = box_chains(box)
    for l in (1, 2):
        rp, col, val = host_prolongator_links(fe, ours[l - 1], ours[l])
        P = sp.csr_matrix((val, col, rp), shape=(ours[l][4][FAM[fe]], ours[l - 1][4][FAM[fe]]))
        Q = foa.build_prolongator(theirs[l - 1], theirs[l], fe)
        assert P.shape == Q.shape
        D = (P - Q).tocoo()
        assert (np.abs(D.data).max() if D.nnz else 0.0) <= 4 * EPS
        assert np.array_equal(rp, Q.indptr) and np.array_equal(col, Q.indices)


# ---- 2. the edge cases on every mesh ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distorted", [False, True], ids=["as_read", "distorted"])
@pytest.mark.parametrize("name", MESHES)
def test_all_flagged_is_refine_and_none_flagged_is_the_input(name, distorted):
    kind, ed, xs, ff, own = coarse(name, distorted)
    nel = kind.shape[0]
    a, want = mixed_mesh.refine_flagged(kind, ed, xs, ff, np.ones(nel, dtype=bool)), mixed_mesh.refine(kind, ed, xs, ff)
    nch = want[0].shape[0] // nel
    assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1]) and np.array_equal(a[3], want[3]) and list(a[4]) == list(want[4])
    assert a[2].shape == want[2].shape and np.array_equal(bits(a[2]), bits(want[2]))
    assert (a[5] == 1).all() and np.array_equal(a[6], np.arange(nch * nel) // nch) and np.array_equal(a[7], np.arange(nch * nel) % nch)
    b = mixed_mesh.refine_flagged(kind, ed, xs, ff, np.zeros(nel, dtype=np.uint8))
    assert np.array_equal(b[0], kind) and np.array_equal(b[1], ed) and np.array_equal(b[3], ff) and list(b[4]) == list(own)
    assert np.array_equal(bits(b[2]), bits(xs))
    assert (b[5] == 0).all() and np.array_equal(b[6], np.arange(nel)) and (b[7] == -1).all()
    with pytest.raises(ValueError):
        mixed_mesh.refine_flagged(kind, ed, xs, ff, np.ones(nel + 1, dtype=bool))


# ---- 3. conservation --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distorted", [False, True], ids=["as_read", "distorted"])
@pytest.mark.parametrize("name", MESHES)
def test_conservation_on_two_flagged_levels(name, distorted):
    chain = flagged_chain(name, distorted)
    nch = 8 if chain[0][2].shape[1] == 3 else 4
    for level in (1, 2):
        c, f = chain[level - 1], chain[level]
        flags, lev_c = f[8], c[5]
        split = (flags != 0) & (lev_c == level - 1)
        kind, ed, xs, ff, own, lev, father, child = f[:8]
        copies = child < 0
        assert 0 < split.sum() < split.size and (level == 1 or (flags != 0)[lev_c < level - 1].any())
        assert kind.shape[0] == (~split).sum() + nch * split.sum() == copies.sum() + nch * split.sum()
        assert np.array_equal(father[copies], np.nonzero(~split)[0]) and np.array_equal(lev[copies], lev_c[~split]) and (lev[~copies] == level).all()
        assert np.array_equal(kind, c[0][father]) and (ed[:, 0] >= 0).all() and own[2] == xs.shape[0] == np.unique(ed[ed >= 0]).size
        for j in range(nch):
            assert np.array_equal(father[child == j], np.nonzero(split)[0])
        # a copy's row is its father's up to the renumbering: one old -> new map serves all copies and the children's vertices, and it keeps the coordinate bits
        new = np.full(c[2].shape[0], -1, dtype=np.int64)
        rows_c, rows_f = c[1][father[copies]], ed[copies]
        assert np.array_equal(rows_c < 0, rows_f < 0) and np.array_equal(ff[copies], c[3][father[copies]])
        new[rows_c[rows_c >= 0]] = rows_f[rows_f >= 0]
        assert np.array_equal(new[rows_c[rows_c >= 0]], rows_f[rows_f >= 0])               # one image per old node
        for s in sorted(set(kind.tolist())):
            T, nv = mixed_mesh.tables(s), mixed_mesh.CLASSES[s][0]
            for j in range(nch):
                m = (kind == s) & (child == j)
                old, img = c[1][father[m]][:, T["f2c"][j]].ravel(), ed[m][:, :nv].ravel()
                known = new[old] >= 0
                assert np.array_equal(new[old][known], img[known])
                new[old] = img
        kept = np.nonzero(new >= 0)[0]
        assert np.unique(new[kept]).size == kept.size and np.array_equal(bits(xs[new[kept]]), bits(c[2][kept]))


# ---- 4. the host transfer rule ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distorted", [False, True], ids=["as_read", "distorted"])
@pytest.mark.parametrize("fe", ["linear", "biquadratic"])
@pytest.mark.parametrize("name", MESHES)
def test_the_transfer_into_a_flagged_level(name, fe, distorted):
    chain = flagged_chain(name, distorted) if distorted or fe != "linear" else straight_chain(name)
    for level in (1, 2):
        c, f = chain[level - 1], chain[level]
        rp, col, val = host_prolongator_links(fe, c, f)
        m, n = f[4][FAM[fe]], c[4][FAM[fe]]
        P = sp.csr_matrix((val, col, rp), shape=(m, n))
        assert (np.diff(rp) > 0).all() and np.abs(P @ np.ones(n) - 1.0).max() <= 64 * EPS
        # the family's dofs are reproduced: by the biquadratic family always (it is the map the coordinates were made with), by the linear family where the
        # edge nodes are the middles of their chords, the meshes as read (straight_chain; on a distorted mesh the middles were moved: nothing linear
        # reproduces them)
        if fe == "biquadratic" or not distorted:
            err = np.abs(P @ c[2][:n] - f[2][:m]).max()
            print("%s %s level %d: max |P xs_c - xs_f| = %.3e, bound %.3e" % (name, fe, level, err, 64 * EPS * np.abs(c[2]).max()))
            assert err <= 64 * EPS * np.abs(c[2]).max()
        # dofs of copies that no child holds: a single exact 1.0
        kind, ed, child = f[0], f[1], f[7]
        nc = np.array([mixed_mesh.CLASSES[s][FAM[fe]] for s in kind])
        inside = np.arange(27)[None, :] < nc[:, None]
        of_children = np.zeros(m, dtype=bool)
        of_children[ed[(child >= 0)[:, None] & inside]] = True
        only = np.zeros(m, dtype=bool)
        only[ed[(child < 0)[:, None] & inside]] = True
        only &= ~of_children
        assert only.any()
        assert (np.diff(rp)[only] == 1).all() and np.array_equal(bits(val[rp[:-1][only]]), bits(np.ones(only.sum())))
        # and a node a copy shares with children holds the exact 1.0 too (the copies' insertions are the last)
        shared = np.zeros(m, dtype=bool)
        shared[ed[(child < 0)[:, None] & inside]] = True
        shared &= of_children
        assert shared.any() and (np.diff(rp)[shared] == 1).all() and (val[rp[:-1][shared]] == 1.0).all()


# ---- 5. flags ---------------------------------------------------------------------------------------------------------------------------------------------
def test_ex4_flags_on_triAMR():
    chain = flagged_chain("triAMR.neu", False)
    for level in (0, 1):
        kind, ed, xs, lev = chain[level][0], chain[level][1], chain[level][2], chain[level][5]
        flags = mixed_mesh.flag_elements(kind, ed, xs, lev, level, ex4)
        assert flags.dtype == np.uint8 and 0 < flags.sum() < flags.size
        assert not flags[lev < level].any()
        assert np.array_equal(flags != 0, (chain[level + 1][8] != 0) & (lev == level))           # the chain was flagged by ex4 here
        e = capi.Expr(EX4, "x,y,z,level")
        assert np.array_equal(flags, mixed_mesh.flag_elements(kind, ed, xs, lev, level, lambda x, l: e(np.array([x[0], x[1], x[2], float(l)])) != 0.0))
        e.destroy()
    assert (chain[1][5] < 1).any()


# ---- 6. control -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", THREE_D)
def test_the_coordinate_comparison_tells_the_creating_child_of_a_flagged_refinement(name):
    """control on the oracle alone: with the coarse elements in reversed order a distorted three-dimensional mesh gets other last bits in some nodes of a
    flagged refinement -- other children create them -- so the bit comparisons of the device test can fail"""
    kind, ed, xs, ff, _ = coarse(name, True)
    flags = level_flags((kind, ed, xs), np.zeros(kind.shape[0], dtype=np.int64), 0)
    rows = lambda x: set(map(bytes, np.ascontiguousarray(x)))
    a = rows(mixed_mesh.refine_flagged(kind, ed, xs, ff, flags)[2])
    b = rows(mixed_mesh.refine_flagged(kind[::-1], ed[::-1], xs, ff[::-1], flags[::-1])[2])
    print("%s: %d of %d coordinate rows differ in bits" % (name, len(a - b), len(a)))
    assert len(a) == len(b) and len(a - b) > 0
