"""capi.ElementMesh.flag / refine(flags) / prolongator into a flagged level (fh_elem_mesh_flag, fh_elem_mesh_refine_flagged, fh_elem_mesh_prolongator): the
selective refinement of a resident element mesh of any shape against the host statement of the rule, mixed_mesh.refine_flagged / flag_elements and
app_poisson._prolongator_from_links (pinned by tests/test_element_refine_flagged_host.py, whose chains are used here) -- names, integers (padding included),
class ends, levels, fathers and children equal, coordinates and transfer values equal as bits.  Two flagged levels from one upload; the flags of the second
level name elements of the older level too, which the rule leaves alone."""
import functools

import numpy as np
import pytest

from femus_amd import capi, mixed_mesh
from oracle import femus_oracle as fo
from test_element_refine_flagged_host import EX4, as_mixed, bits, ex4, flagged_chain, flagged_chain_of, host_prolongator_links
from test_element_transfer_host import FAM, FAMILIES
from test_gpu_element_mesh import MESHES, MIXED_CUBE, coarse, same
from test_gpu_element_transfer import DEFAULT_CAP, OPTION, csr, destroy, host_boundary_sets, same_bits

pytestmark = pytest.mark.gpu


def resident_flagged_chain(ctx, chain):
    """the levels of a host chain as resident meshes: level 0 goes up, every further level is refined on the device with the host chain's flags"""
    dev = [capi.ElementMesh.from_arrays(ctx, *chain[0][:5])]
    try:
        for h in chain[1:]:
            dev.append(dev[-1].refine(h[8]))
    except Exception:
        destroy(dev)
        raise
    return dev


def same_level(m, h, level):
    same(m.arrays(), h[:5])
    lev, father, child = m.elem_levels()
    assert np.array_equal(lev, h[5]) and np.array_equal(father, h[6]) and np.array_equal(child, h[7])
    assert (m.nel, m.nnode, m.dim, m.level, m.own) == (h[0].shape[0], h[2].shape[0], h[2].shape[1], level, list(h[4]))
    assert m.homogeneous == bool((h[5] == level).all())


# ---- 1. two flagged levels -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distorted", [False, True], ids=["as_read", "distorted"])
@pytest.mark.parametrize("name", MESHES)
def test_two_flagged_device_levels_equal_the_host_rule(ctx, name, distorted):
    chain = flagged_chain(name, distorted)
    assert (chain[2][8] != 0)[chain[1][5] < 1].any() and len({0, 1, 2} & set(chain[2][5].tolist())) == 3
    dev = resident_flagged_chain(ctx, chain)
    try:
        for level, (m, h) in enumerate(zip(dev, chain)):
            same_level(m, h, level)
        assert dev[0].homogeneous and not dev[1].homogeneous and not dev[2].homogeneous
    finally:
        destroy(dev)


@pytest.mark.parametrize("name", MESHES)
def test_all_flagged_is_the_uniform_refinement_and_none_flagged_the_input(ctx, name):
    mesh = coarse(name, True)
    c = capi.ElementMesh.from_arrays(ctx, *mesh)
    u = c.refine()
    a = c.refine(np.ones(c.nel, dtype=bool))
    b = c.refine(np.zeros(c.nel, dtype=np.uint8))
    try:
        same(a.arrays(), u.arrays())
        for x, y in zip(a.elem_levels(), u.elem_levels()):
            assert np.array_equal(x, y)
        nch = u.nel // c.nel
        lev, father, child = u.elem_levels()
        assert (lev == 1).all() and np.array_equal(father, np.arange(u.nel) // nch) and np.array_equal(child, np.arange(u.nel) % nch)
        assert (a.level, a.homogeneous, u.homogeneous, a.own, a.nnode) == (1, True, True, u.own, u.nnode)
        same(b.arrays(), mesh)
        lev, father, child = b.elem_levels()
        assert (lev == 0).all() and np.array_equal(father, np.arange(c.nel)) and (child == -1).all()
        assert (b.level, b.homogeneous, b.nel, b.nnode) == (1, False, c.nel, c.nnode)
        lev, father, child = c.elem_levels()
        assert (lev == 0).all() and (father == -1).all() and (child == -1).all() and c.homogeneous
    finally:
        destroy(c, u, a, b)


@pytest.mark.parametrize("name", [MIXED_CUBE, "square_mixed.neu"])
def test_shapes_interleaved(ctx, name):
    kind, ed, xs, ff, own = coarse(name, True)
    perm = np.random.default_rng(7).permutation(kind.shape[0])
    kp = kind[perm]
    assert (kp[1:] != kp[:-1]).sum() > (kind[1:] != kind[:-1]).sum()
    chain = flagged_chain_of((kp, ed[perm], xs, ff[perm], own))
    dev = resident_flagged_chain(ctx, chain)
    try:
        for level, (m, h) in enumerate(zip(dev, chain)):
            same_level(m, h, level)
    finally:
        destroy(dev)


def test_set_levels_makes_an_uploaded_mesh_non_homogeneous(ctx):
    """level 1 of a host chain uploaded as it is: with its levels set, the second flagged refinement is the chain's"""
    chain = flagged_chain(MIXED_CUBE, True)
    m = capi.ElementMesh.from_arrays(ctx, *chain[1][:5])
    assert m.level == 0 and m.homogeneous
    m.set_levels(chain[1][5])
    f = m.refine(chain[2][8])
    try:
        assert (m.level, m.homogeneous) == (1, False) and np.array_equal(m.elem_levels()[0], chain[1][5])
        same_level(f, chain[2], 2)
    finally:
        destroy(m, f)


# ---- 2. flags --------------------------------------------------------------------------------------------------------------------------------------------
def _host_flags(level_arrays, level, text):
    e = capi.Expr(text, "x,y,z,level")
    try:
        return mixed_mesh.flag_elements(level_arrays[0], level_arrays[1], level_arrays[2], level_arrays[5], level,
                                        lambda x, l: abs(e(np.array([x[0], x[1], x[2], float(l)]))) >= 0.5)
    finally:
        e.destroy()


@pytest.mark.parametrize("name", MESHES)
def test_device_flags_equal_the_host_flags(ctx, name):
    chain = flagged_chain(name, True)
    dev = resident_flagged_chain(ctx, chain)
    try:
        for level, (m, h) in enumerate(zip(dev, chain)):
            for text in (EX4, "x>0 & y>-0.25", "x*x+y*y+z*z < 0.3 + 0.1*level"):
                got = m.flag(text)
                assert got.dtype == np.uint8 and got.shape == (m.nel,) and np.array_equal(got, _host_flags(h, level, text)), (level, text)
                assert not got[h[5] < level].any()
            want = mixed_mesh.flag_elements(h[0], h[1], h[2], h[5], level, ex4)
            assert np.array_equal(m.flag(EX4), want)
    finally:
        destroy(dev)


@functools.lru_cache(maxsize=None)
def threshold_meshes():
    """(mesh, expression, host flags, elements on the threshold): a box of quadrilaterals whose middle column has the centroid x = 0 exactly, under x>0 and
    x>=0 (exact in any order of summation); the tetrahedra with the threshold AT the centroid of one of their elements as the rule sums it, under > and >=
    -- five elements of the distorted mesh, each alone on its threshold, and one of the mesh as read, where other elements share its centroid's x"""
    out = []
    mo = fo.coarse_box_mesh(3, 2, 0, lo=(-1.5, -1.0, 0.0), hi=(1.5, 1.0, 0.0))
    quads = as_mixed(mo) + (list(mo.own_size),)
    tets = coarse("cube_Tet.neu", True)
    cases = [(quads, 0.0, 1), (coarse("cube_Tet.neu", False), None, 11)] + [(tets, None, e0) for e0 in (3, 11, 40, 77, 100)]
    for mesh, c, e0 in cases:
        zero = np.zeros(mesh[0].shape[0], dtype=np.int64)
        cx = []
        mixed_mesh.flag_elements(mesh[0], mesh[1], mesh[2], zero, 0, lambda x, l: cx.append(float(x[0])) or False)
        cx = np.array(cx)
        c = float(cx[e0]) if c is None else c
        on = cx == c
        assert on[e0] and (cx > c).any() and (cx < c).any()
        for op in (">", ">="):
            text = "x %s %s" % (op, repr(c))
            want = (cx > c) if op == ">" else (cx >= c)
            out.append((mesh, text, want.astype(np.uint8), on))
    assert out[0][3].sum() == 2 and out[2][3].sum() > 1
    return out


def test_a_centroid_on_the_threshold_flags_the_same_on_both_sides(ctx):
    for mesh, text, want, on in threshold_meshes():
        m = capi.ElementMesh.from_arrays(ctx, *mesh)
        try:
            got = m.flag(text)
            assert np.array_equal(got, want), text
            assert np.array_equal(got, _host_flags(mesh[:5] + (np.zeros(m.nel, dtype=np.int64),), 0, text))
            assert (got[on] == (1 if ">=" in text else 0)).all()
        finally:
            m.destroy()


@pytest.mark.parametrize("name,text", [(MIXED_CUBE, "x>0.5 | z>0.8"), ("triAMR.neu", EX4)])
def test_resident_flags_refine_like_flags_from_the_host(ctx, name, text):
    chain = flagged_chain(name, True)
    c = capi.ElementMesh.from_arrays(ctx, *chain[0][:5])
    flags = c.flag(text)
    assert 0 < flags.sum() < flags.size
    a, b = c.refine("resident"), c.refine(flags)
    try:
        same(a.arrays(), b.arrays())
        for x, y in zip(a.elem_levels(), b.elem_levels()):
            assert np.array_equal(x, y)
        h = mixed_mesh.refine_flagged(*chain[0][:4], flags)
        same(a.arrays(), h[:5])
        # the fine mesh has no flags of its own yet; its own flags then refine it
        with pytest.raises(capi.FemusHipError) as err:
            a.refine("resident")
        assert "none resident" in str(err.value), str(err.value)
        f2 = a.flag(text)
        assert 0 < f2.sum() < f2.size and not f2[h[5] < 1].any()
        g = a.refine("resident")
        h2 = mixed_mesh.refine_flagged(*h[:4], f2, h[5], 1)
        same(g.arrays(), h2[:5])
        g.destroy()
    finally:
        destroy(c, a, b)


# ---- 3. the transfer into a flagged level ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_transfer_links(name, fe, level):
    chain = flagged_chain(name, True)
    out = host_prolongator_links(fe, chain[level - 1], chain[level])
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", MESHES)
def test_the_transfer_into_a_flagged_level_has_the_host_rule_s_bits(ctx, name):
    """three families x levels 0 -> 1 and 1 -> 2, rows in the wave's LDS and, with the capacity at one element's slots, in the workgroup's scratch"""
    chain = flagged_chain(name, True)
    dev = resident_flagged_chain(ctx, chain)
    try:
        for cap in (DEFAULT_CAP, 27):
            ctx.set_option(OPTION, cap)
            for fe in FAMILIES:
                for level in (1, 2):
                    P = dev[level - 1].prolongator(dev[level], fe)
                    assert (P.m_, P.n_) == (chain[level][4][FAM[fe]], chain[level - 1][4][FAM[fe]])
                    got = csr(P)
                    P.destroy()
                    same_bits(got, host_transfer_links(name, fe, level))
    finally:
        ctx.set_option(OPTION, DEFAULT_CAP)
        destroy(dev)


@pytest.mark.parametrize("name", [MIXED_CUBE, "square_mixed.neu", "triAMR.neu"])
def test_boundary_dofs_of_a_flagged_level(ctx, name):
    chain = flagged_chain(name, True)
    dev = resident_flagged_chain(ctx, chain)
    try:
        for m, h in zip(dev[1:], chain[1:]):
            for fe in FAMILIES:
                by_flag = host_boundary_sets(h[:5], fe)
                flags = sorted(by_flag)
                assert flags
                for sub in [flags] + [[f] for f in flags]:
                    want = np.array(sorted(set().union(*(by_flag[f] for f in sub))), dtype=np.int32)
                    assert np.array_equal(m.boundary_dofs(fe, sub), want), (fe, sub)
    finally:
        destroy(dev)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    tri = resident_flagged_chain(ctx, flagged_chain("triAMR.neu", True))
    two = capi.ElementMesh.from_arrays(ctx, *coarse("tri2.neu", False))
    sq = resident_flagged_chain(ctx, flagged_chain("square_mixed.neu", True)[:2])

    def refused(call, words):
        with pytest.raises(capi.FemusHipError) as err:
            call()
        assert words in str(err.value), str(err.value)

    try:
        refused(lambda: two.prolongator(tri[1], "biquadratic"), "not its refinement")            # fathers the coarse mesh does not have
        refused(lambda: sq[0].prolongator(tri[1], "biquadratic"), "not its refinement")           # fathers the coarse mesh does not have either
        refused(lambda: tri[0].prolongator(sq[1], "biquadratic"), "neither children nor a copy")  # fathers in range, two coarse elements without fine ones
        refused(lambda: tri[1].refine(), "holds elements of older levels")                          # the uniform refinement of a flagged level
        refused(lambda: tri[0].prolongator(tri[2], "linear"), "not its refinement")
        refused(lambda: tri[0].refine(np.ones(tri[0].nel + 1, dtype=np.uint8)), "flags for %d elements" % tri[0].nel)
        refused(lambda: tri[0].refine(np.ones((tri[0].nel, 1), dtype=np.uint8)), "flags for %d elements" % tri[0].nel)
        refused(lambda: two.refine("resident"), "none resident")
        refused(lambda: two.refine("all"), "resident")
        refused(lambda: two.flag("x > q"), "q")                                                     # the parser's message names what it cannot read
        refused(lambda: two.flag(capi.Expr("a+b+c+d+e", "a,b,c,d,e")), "has 5 variables, at most 4")
        refused(lambda: two.set_levels(np.zeros(two.nel + 1, dtype=np.int32)), "levels for %d elements" % two.nel)
        # and the context goes on working
        chain = flagged_chain("tri2.neu", True)
        dev = resident_flagged_chain(ctx, chain)
        same_level(dev[2], chain[2], 2)
        destroy(dev)
    finally:
        destroy(tri, two, sq)
