"""mixed_mesh.amr_constraints (fh_elem_amr_constraints_host): the hanging-node constraints of a flagged level of an element mesh of any shape, on the host -- the
yardstick of the device search (tests/test_gpu_element_constraints.py, which imports the chains from here).  On boxes of quadrilaterals and hexahedra the rule
is held against oracle/femus_oracle_amr.py: amr_restriction; on the meshes of tests/golden against what a constraint must do: reproduce the polynomials of its
family at every hanging dof, and not depend on the geometry.  No device.  Chains are computed once per mesh and shared, read-only.

Bounds.  Both Newton iterations (ours, the oracle's) stop below 1e-14 * scale and the basis gradients are O(10): weights agree to about 1e-13, asserted at 1e-12.
A hanging node's row reproduces a polynomial of degree <= 2 up to the same error times the polynomial's size, max(1, |x|^2)."""
import functools
import itertools

import numpy as np
import pytest

from femus_amd import capi, mixed_mesh
from oracle import femus_oracle_amr as foa
from test_element_refine_flagged_host import BOXES, box_chains, flagged_chain, flagged_chain_of, straight_chain
from test_element_transfer_host import FAM
from test_gpu_element_mesh import MESHES, MIXED_CUBE, THREE_D, coarse

FAMILIES3 = ["linear", "serendipity", "biquadratic"]
MODES = ["reference", "coarsest"]
# the number of hanging dofs (it does not depend on the mode): {mesh: {level: {family: n}}}
COUNTS = {"triAMR.neu": {1: {"linear": 2, "biquadratic": 4}, 2: {"linear": 7, "biquadratic": 14}},
          "tri_box": {1: {"linear": 8, "biquadratic": 16}, 2: {"linear": 29, "biquadratic": 58}},
          "square_mixed.neu": {1: {"linear": 2, "biquadratic": 4}, 2: {"linear": 7, "biquadratic": 14}},
          "cube_Wedge.neu": {1: {"linear": 33, "biquadratic": 138}, 2: {"linear": 231, "biquadratic": 993}},
          MIXED_CUBE: {1: {"linear": 44, "biquadratic": 207}, 2: {"linear": 246, "biquadratic": 1209}},
          "cube_Tet.neu": {1: {"linear": 131, "serendipity": 565, "biquadratic": 969}, 2: {"linear": 805, "serendipity": 3419, "biquadratic": 5633}}}


def constraints(level, fe, mode):
    """(hanging, ptr, master, weight) of one level of a chain"""
    return mixed_mesh.amr_constraints(level[0], level[1], level[2], level[3], level[5], fe, mode)


def rows_of(c):
    hang, ptr, master, w = c
    return {int(h): (master[ptr[i]:ptr[i + 1]].astype(np.int64), w[ptr[i]:ptr[i + 1]]) for i, h in enumerate(hang)}


def well_formed(c, ndof):
    hang, ptr, master, w = c
    assert hang.dtype == np.int32 and ptr.shape == (hang.size + 1,) and ptr[0] == 0 and ptr[-1] == master.size == w.size
    assert (np.diff(hang) > 0).all() and (np.diff(ptr) > 0).all() and np.isfinite(w).all()
    assert hang.size == 0 or (0 <= hang.min() and hang.max() < ndof and 0 <= master.min() and master.max() < ndof)
    for i in range(hang.size):
        assert (np.diff(master[ptr[i]:ptr[i + 1]]) > 0).all()               # masters ascending within a row


def warp(xs):
    c = xs - xs.min(axis=0)
    L = float(c.max())
    return xs + 0.04 * L * np.sin(np.pi * np.roll(c, 1, axis=1) / L) * np.cos(0.7 * np.pi * np.roll(c, -1, axis=1) / L + 0.3)


@functools.lru_cache(maxsize=None)
def warped_chain(name):
    """the flagged chain of the mesh as read with its level-0 nodes moved smoothly (curved elements whose biquadratic maps still invert); the flags are the
    unwarped chain's, so that the two chains are the same mesh in two geometries"""
    kind, ed, xs, ff, own = coarse(name, False)
    xw = warp(xs)
    xw.setflags(write=False)
    chain = flagged_chain_of((kind, ed, xw, ff, own))
    for a, b in zip(chain[1:], flagged_chain(name, False)[1:]):
        assert np.array_equal(a[8], b[8]) and np.array_equal(a[1], b[1]) and np.array_equal(a[5], b[5])
    return chain


# ---- 1. against the independent oracle on boxes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fe", ["linear", "biquadratic"])
@pytest.mark.parametrize("box", BOXES, ids=["quad_3x2", "hex_2x2x2"])
def test_the_rows_equal_the_oracle_s_on_boxes(box, fe, mode):
    ours, theirs = box_chains(box)
    for level in (1, 2):
        c = constraints(ours[level], fe, mode)
        well_formed(c, ours[level][4][FAM[fe]])
        got, want = rows_of(c), foa.amr_restriction(theirs[level], fe, mode)
        assert sorted(got) == sorted(want) and len(got) > 0
        err = 0.0
        for h, (m, w) in got.items():
            assert m.tolist() == sorted(want[h])
            err = max(err, max(abs(want[h][int(j)] - v) for j, v in zip(m, w)))
        print("%s level %d %s %s: %d hanging dofs, max |w - oracle| = %.2e" % (theirs[level].geom, level, fe, mode, len(got), err))
        assert err <= 1e-12


# ---- 2. polynomial reproduction ------------------------------------------------------------------------------------------------------------------------------
def monomials(dim, degree):
    return [p for p in itertools.product(range(degree + 1), repeat=dim) if sum(p) <= degree]


@pytest.mark.parametrize("fe", FAMILIES3)
@pytest.mark.parametrize("name", MESHES)
def test_a_row_reproduces_the_polynomials_of_its_family(name, fe):
    chain = straight_chain(name)
    for level in (1, 2):
        lv = chain[level]
        xs, dim = lv[2], lv[2].shape[1]
        c = constraints(lv, fe, "coarsest")
        well_formed(c, lv[4][FAM[fe]])
        hang, ptr, master, w = c
        want = COUNTS.get(name, {}).get(level, {}).get(fe)
        print("%s level %d %s: %d hanging dofs, %d entries" % (name, level, fe, hang.size, master.size))
        assert hang.size > 0 and (want is None or hang.size == want)
        for f2 in MODES:                                    # the number of hanging dofs does not depend on the mode
            assert np.array_equal(constraints(lv, fe, f2)[0], hang)
        sums = np.add.reduceat(w, ptr[:-1])
        assert np.abs(sums - 1.0).max() <= 1e-12
        bound = 1e-12 * max(1.0, float(np.abs(xs).max()) ** 2)
        worst = 0.0
        for p in monomials(dim, 1 if fe == "linear" else 2):
            val = np.prod(xs ** np.array(p), axis=1)
            err = np.abs(np.add.reduceat(w * val[master], ptr[:-1]) - val[hang]).max()
            worst = max(worst, err)
            assert err <= bound, (p, err, bound)
        print("    max |sum w p(x_m) - p(x_h)| = %.2e (bound %.2e), max |row sum - 1| = %.2e" % (worst, bound, np.abs(sums - 1.0).max()))


# ---- 3. geometry independence --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fe", FAMILIES3)
@pytest.mark.parametrize("name", MESHES)
def test_the_rows_do_not_depend_on_the_geometry(name, fe):
    """a hanging node sits at the same reference point of its coarse element whatever the geometry: the lists of the warped chain are the unwarped one's, the
    weights equal to rounding"""
    flat, curved = flagged_chain(name, False), warped_chain(name)
    assert np.abs(curved[0][2] - flat[0][2]).max() > 0.01 * np.ptp(flat[0][2])
    for level in (1, 2):
        for mode in MODES:
            a, b = constraints(flat[level], fe, mode), constraints(curved[level], fe, mode)
            assert all(np.array_equal(a[k], b[k]) for k in range(3)) and a[0].size > 0
            err = np.abs(a[3] - b[3]).max()
            print("%s level %d %s %s: %d entries, max |w_warped - w| = %.2e" % (name, level, fe, mode, a[3].size, err))
            assert err <= 1e-12


# ---- 4. the two modes ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fe", FAMILIES3)
@pytest.mark.parametrize("name", MESHES)
def test_the_modes_agree_where_every_jump_is_single(name, fe):
    lv = straight_chain(name)[1]
    a, b = constraints(lv, fe, "reference"), constraints(lv, fe, "coarsest")
    assert all(np.array_equal(a[k], b[k]) for k in range(3)) and np.abs(a[3] - b[3]).max() <= 1e-15


@pytest.mark.parametrize("name", THREE_D)
def test_the_reference_mode_on_a_double_jump(name):
    """level 2 of the three-dimensional meshes holds nodes on the interfaces with two coarser levels at once.  There the reference's resolution keeps the direct
    entry and drops the path through the intermediate hanging node: rows of mode "reference" need not sum to one (only mode "coarsest" is held to that, in test 2).
    What this records, with the chains of this file, biquadratic: rows off one by more than 1e-12 -- cube_Tet.neu 1828 of 5633, cube_Wedge.neu 236 of 993, the mixed
    cube 318 of 1209 (printed again below).  The hanging dofs themselves are the same in both modes."""
    lv = straight_chain(name)[2]
    a, b = constraints(lv, "biquadratic", "reference"), constraints(lv, "biquadratic", "coarsest")
    assert np.array_equal(a[0], b[0])
    off = np.abs(np.add.reduceat(a[3], a[1][:-1]) - 1.0) > 1e-12
    print("%s level 2 biquadratic, mode reference: %d of %d rows do not sum to one" % (name, int(off.sum()), off.size))
    assert np.abs(np.add.reduceat(b[3], b[1][:-1]) - 1.0).max() <= 1e-12


# ---- 5. control: what a patch test on these meshes may be assembled with ---------------------------------------------------------------------------------------
def test_the_seventh_order_rule_of_the_tetrahedron_does_not_sum_to_its_volume():
    """the reference's Gauss tables are kept digit for digit; its 31-point rule of the tetrahedron ("seventh", the default order of the assemblers) sums to
    1/6 - 1.07e-9.  A patch test on a mesh with tetrahedra assembled with it misses by about 1e-8 whatever the constraints do, so the one of
    tests/test_gpu_element_constraints.py assembles with "fifth", exact to rounding on every shape"""
    import ctypes
    L = capi.load_library()
    total = {}
    for order in ("fifth", "seventh"):
        for geom, volume in (("tet", 1.0 / 6.0), ("wedge", 1.0), ("tri", 0.5), ("hex", 8.0), ("quad", 4.0)):
            ng, w, x = ctypes.c_int(), np.zeros(256), np.zeros(1024)
            capi._chk(L.fh_fe_gauss(capi.GEOM[geom], capi.GAUSS_ORDER[order], ctypes.byref(ng), capi._p(w), capi._p(x)))
            total[order, geom] = w[:ng.value].sum() - volume
            print("%s %s: %d points, sum of the weights - volume = %.3e" % (geom, order, ng.value, total[order, geom]))
    assert all(abs(total["fifth", g]) <= 1e-13 for g in ("tet", "wedge", "tri", "hex", "quad"))
    assert all(abs(total["seventh", g]) <= 1e-13 for g in ("wedge", "tri", "hex", "quad"))
    assert 1.0e-9 < -total["seventh", "tet"] < 1.2e-9
