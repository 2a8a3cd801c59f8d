"""tests/system_families_reference.py, the restatement of a coupled system whose variables are of different families (the yardstick of the block matrices
Mat.block_system(m, sizes=) now, of an element body for such systems when there is one), checked on the host before anything is measured with it:
(a) with every variable of the mesh's family it is tests/system_reference.py, to 1e-14 of the largest entry;
(b) its Jacobian is the derivative of its residual for the mixed-order form and for Stokes: K delta against the five-point central difference of -RES;
(c) the prefix property the device path rests on: with S the pattern of the highest family, S[:n_k, :n_l] IS the pattern of the pairs (function of family
    f_k, function of family f_l) on a uniform level, and CONTAINS it on a flagged level (the extras are counted and printed);
and the argument refusals that need no device."""
import numpy as np
import pytest

import quasilinear_reference as qr
import system_families_reference as fr
import system_reference as sr
from femus_amd import mixed_mesh
from test_gpu_generic_assembler import CASES, FES, curved, mesh

_MESH = {}


def setup(case, refinements=0):
    if (case, refinements) not in _MESH:
        kind, ed, xs, own = mesh(case, refinements=refinements)
        _MESH[(case, refinements)] = (kind, ed, curved(xs), own)
    return _MESH[(case, refinements)]


def lists(dim):
    """lists of families, each with the family of the mesh's table: Taylor-Hood by dimension among them"""
    return [("biquadratic", ("biquadratic", "linear")), ("biquadratic", ("biquadratic",) * dim + ("linear",)), ("serendipity", ("serendipity", "linear")),
            ("biquadratic", ("biquadratic", "serendipity", "linear"))]


@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("case", CASES)
def test_equal_families_are_the_restatement_of_one_family(case, fe):
    kind, ed, xs, own = setup(case)
    dim = xs.shape[1]
    form = sr.form_s(dim)[1]
    m = form["m"]
    u = np.random.default_rng(11).uniform(-1, 1, m * own[qr.FAM[fe]])
    K, F = fr.assemble(kind, ed, xs, fe, [fe] * m, form, own, u)
    Ks, Fs = sr.assemble(kind, ed, xs, fe, form, u)
    assert K.shape == Ks.shape
    assert abs(K - Ks).max() <= 1e-14 * abs(Ks).max()
    assert np.abs(F - Fs).max() <= 1e-14 * max(np.abs(Fs).max(), abs(Ks).max())


JACOBIAN_TOL = 4.4e-12     # the bound of tests/test_quasilinear_reference_host.py


@pytest.mark.parametrize("name", ["mixed", "stokes"])
@pytest.mark.parametrize("case", CASES)
def test_the_jacobian_is_the_derivative_of_the_residual(case, name):
    """K(U) delta = d(-RES)(U + t delta)/dt at t = 0 by (R(-2h) - 8 R(-h) + 8 R(h) - R(2h)) / 12h at h = 2^-3: the mixed-order form makes RES a cubic in U and
    Stokes a linear function, so the formula has no truncation error"""
    kind, ed, xs, own = setup(case)
    dim = xs.shape[1]
    for fe, fes in lists(dim):
        if name == "stokes":
            if len(fes) != dim + 1:
                continue
            form = fr.form_flow(dim, convection=False)[1]
        else:
            form = fr.form_m(len(fes), dim)[1]
        N = sum(fr.sizes(own, fes)[0])
        rng = np.random.default_rng(11)
        u, delta = rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)
        h = 2.0 ** -3
        K, _ = fr.assemble(kind, ed, xs, fe, fes, form, own, u)
        R = {t: fr.assemble(kind, ed, xs, fe, fes, form, own, u + t * h * delta)[1] for t in (-2, -1, 1, 2)}
        dR = (R[-2] - 8 * R[-1] + 8 * R[1] - R[2]) / (12 * h)
        Kd = K @ delta
        defect = np.abs(Kd + dR).max() / np.abs(Kd).max()
        print("%s %s form %s: |K delta + dRES| = %.3e of max |K delta|" % (case, "/".join(f[:3] for f in fes), name, defect))
        assert defect <= JACOBIAN_TOL
        assert K.shape == (N, N)
        if name == "stokes":
            n, off = fr.sizes(own, fes)
            assert abs(K[off[dim]:, off[dim]:]).max() == 0.0                       # the pressure block: the program 0


def top_pattern(kind, ed, own):
    return fr.pair_pattern(kind, ed, "biquadratic", "biquadratic", own[2], own[2])


@pytest.mark.parametrize("case", CASES)
def test_the_prefix_property_on_a_uniform_level(case):
    """the golden meshes refined once: for every pair of families the rows and columns below n_k, n_l of the biquadratic pattern ARE the pattern of the pairs,
    and the columns < n_l of every row are a prefix of the row"""
    kind, ed, xs, own = setup(case, 1)
    S = top_pattern(kind, ed, own)
    for fk in FES:
        for fl in FES:
            nk, nl = own[qr.FAM[fk]], own[qr.FAM[fl]]
            B, Pp = S[:nk, :nl].tocsr(), fr.pair_pattern(kind, ed, fk, fl, nk, nl)
            B.sort_indices()
            assert B.nnz == Pp.nnz and np.array_equal(B.indptr, Pp.indptr) and np.array_equal(B.indices, Pp.indices), (case, fk, fl)
    for i in range(0, own[2], 7):
        c = S.indices[S.indptr[i]:S.indptr[i + 1]]
        assert np.all(np.diff(c) > 0)


def flagged_level(case):
    """the refined golden mesh with about a third of its elements refined once more (the hanging nodes stay in the numbering)"""
    lv = mixed_mesh.tri_box(3, 2, (0., 0.), (1.5, 1.)) if case == "tri" else None
    if lv is None:
        import os
        from test_gpu_generic_assembler import GOLDEN
        lv = mixed_mesh.read_gambit(os.path.join(GOLDEN, {"tet": "cube_Tet.neu", "wedge": "cube_Wedge.neu", "mixed3d": "cube_all_shapes_Six_boundary_groups.neu",
                                                          "mixed2d": "square_mixed.neu"}[case]))
    lv = mixed_mesh.refine(*lv[:4])
    flags = np.zeros(lv[1].shape[0], dtype=np.uint8)
    flags[::3] = 1
    return mixed_mesh.refine_flagged(*lv[:4], flags)


@pytest.mark.parametrize("case", CASES)
def test_the_prefix_property_on_a_flagged_level(case):
    """S[:n_k, :n_l] contains the pattern of the pairs; the extras (a copy's edge node that a refined neighbour owns as a vertex) are counted"""
    lv = flagged_level(case)
    kind, ed, own = lv[0], lv[1], lv[4]
    extras = 0
    S = top_pattern(kind, ed, own)
    for fk in FES:
        for fl in FES:
            nk, nl = own[qr.FAM[fk]], own[qr.FAM[fl]]
            B, Pp = S[:nk, :nl].tocsr(), fr.pair_pattern(kind, ed, fk, fl, nk, nl)
            B.data[:] = 1.0
            missing = (Pp - Pp.multiply(B)).count_nonzero()
            print("%s %s x %s: %d entries of the block, %d of them no pair of an element" % (case, fk, fl, B.nnz, B.nnz - Pp.nnz))
            assert missing == 0 and B.nnz >= Pp.nnz
            extras += B.nnz - Pp.nnz
    assert extras > 0, "no copy's edge node is a neighbour's vertex: the level tests nothing"


def test_block_system_of_the_restatement():
    """fr.block_system, the expectation of the device tests, on a small pattern: equal sizes give kron(ones, S)"""
    import scipy.sparse as sp
    S = sp.random(9, 9, density=0.4, random_state=2, format="csr")
    S.sort_indices()
    B = fr.block_system(S, [9, 9])
    want = sp.kron(np.ones((2, 2)), S, format="csr")
    want.sort_indices()
    assert np.array_equal(B.indptr, want.indptr) and np.array_equal(B.indices, want.indices) and not B.data.any()
    B = fr.block_system(S, [9, 4])
    assert B.shape == (13, 13) and B.nnz == S.nnz + S[:, :4].nnz + S[:4, :].nnz + S[:4, :4].nnz


def test_argument_refusals_that_need_no_device():
    from femus_amd import capi
    with pytest.raises(ValueError, match="5 variables"):
        capi.SystemForm(5)
    form = capi.SystemForm(**fr.form_flow(2)[0])
    assert form.m == 3
    form.destroy()
    form = capi.SystemForm(**fr.form_m(4, 3)[0])
    assert form.m == 4
    form.destroy()
    with pytest.raises(ValueError, match="no matrices"):
        capi.Mat.block_diagonal_of([])
    with pytest.raises(ValueError, match="no matrices"):
        capi.Mat.block_diagonal_of([None, None])
