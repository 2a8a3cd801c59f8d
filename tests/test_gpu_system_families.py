"""The block matrices of systems whose variables are of different families: Mat.block_system(m, sizes=) (fh_mat_block_system_families) and
Mat.block_diagonal_of (fh_mat_block_diagonal_of), against scipy for integers and value bits, and on element meshes against the pattern of the pairs
(function of family f_k, function of family f_l) that tests/system_families_reference.py states and tests/test_system_families_reference_host.py holds
against the numbering.  Meshes are those of tests/test_gpu_system.py (test_gpu_generic_assembler.mesh refined once)."""
import numpy as np
import pytest
import scipy.sparse as sp

import quasilinear_reference as qr
import system_families_reference as fr
from test_gpu_generic_assembler import CASES, Setup
from test_gpu_quasilinear import level

pytestmark = pytest.mark.gpu
L, S_, B = "linear", "serendipity", "biquadratic"


def equal_patterns(Bm, want):
    rp, col = Bm.pattern()
    assert (Bm.m(), Bm.n(), Bm.nnz) == (want.shape[0], want.shape[1], want.nnz)
    assert np.array_equal(rp, want.indptr) and np.array_equal(col, want.indices)
    assert all(np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0) for r in range(Bm.m()))


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_block_matrices_against_scipy(ctx, m):
    """integers and value bits: sizes (own[2], own[0]), (own[1], own[1], own[0]) and all equal, cut to m, and sizes of 1, 2 and 3; equal sizes and equal P give
    the integers and bits of block_system / block_diagonal; a product with a rectangular block diagonal"""
    from femus_amd import capi
    rng = np.random.default_rng(5)
    s = Setup(ctx, "mixed2d", B, lv=level("mixed2d"))
    own = level("mixed2d")[3]
    S = s.pat.copy()
    S.data = rng.uniform(-1, 1, S.nnz)
    s.K.set_values(S.data)
    Ps = [sp.random(r, c, density=0.3, random_state=3 + i, format="csr") for i, (r, c) in enumerate([(37, 11), (23, 23), (5, 19), (41, 7)])]
    for P in Ps:
        P.sort_indices()
    dPs = [capi.Mat.from_csr(ctx, P.shape[0], P.shape[1], P.indptr, P.indices, P.data) for P in Ps]
    made = []
    try:
        for sizes in ([own[2], own[0], own[1], own[0]][:m], [own[1], own[1], own[0], own[2]][:m], [own[2]] * m, [1, own[2], 2, 3][:m]):
            Bm = s.K.block_system(m, sizes=sizes)
            made.append(Bm)
            equal_patterns(Bm, fr.block_system(S, sizes))
            assert not Bm.values().any() and Bm.built_on() == "device"
        old = s.K.block_system(m)
        made.append(old)
        rp, col = made[2].pattern()
        rpo, colo = old.pattern()
        assert np.array_equal(rp, rpo) and np.array_equal(col, colo)
        # block diagonals: different rectangular matrices, then m times the same
        D = capi.Mat.block_diagonal_of(dPs[:m])
        made.append(D)
        want = sp.block_diag(Ps[:m], format="csr")
        want.sort_indices()
        equal_patterns(D, want)
        assert np.array_equal(D.values().view(np.uint64), want.data.view(np.uint64)) and D.built_on() == "device"
        same, oldd = capi.Mat.block_diagonal_of([dPs[0]] * m), dPs[0].block_diagonal(m)
        made += [same, oldd]
        assert np.array_equal(same.pattern()[0], oldd.pattern()[0]) and np.array_equal(same.pattern()[1], oldd.pattern()[1])
        assert np.array_equal(same.values().view(np.uint64), oldd.values().view(np.uint64))
        x = rng.uniform(-1, 1, want.shape[1])
        X, Y = ctx.vector_from(x), ctx.vector(want.shape[0])
        Y.matrix_mult(X, D)
        assert np.abs(Y.to_numpy() - want @ x).max() <= 1e-14 * 23
    finally:
        for M in made + dPs:
            M.destroy()
        s.close()


@pytest.mark.parametrize("case", CASES)
def test_on_a_uniform_level_the_blocks_are_the_patterns_of_the_pairs(ctx, case):
    """Taylor-Hood by dimension and (biquadratic, serendipity, linear) on the biquadratic pattern of the case's mesh: block (k, l) of the device's matrix is the
    pattern of the pairs of families (f_k, f_l) of every element, built from the element table alone"""
    kind, ed, xs, own = level(case)
    dim = xs.shape[1]
    s = Setup(ctx, case, B, lv=level(case))
    made = []
    try:
        for fes in ((B,) * dim + (L,), (B, S_, L), (S_, L)):
            n, off = fr.sizes(own, fes)
            Bm = s.K.block_system(len(fes), sizes=n)
            made.append(Bm)
            want = sp.bmat([[fr.pair_pattern(kind, ed, fk, fl, nk, nl) for fl, nl in zip(fes, n)] for fk, nk in zip(fes, n)], format="csr")
            want.sort_indices()
            equal_patterns(Bm, want)
            assert not Bm.values().any()
    finally:
        for M in made:
            M.destroy()
        s.close()


def test_block_matrix_refusals(ctx):
    from femus_amd import capi
    small = capi.Mat.from_csr(ctx, 2, 2, np.array([0, 1, 2]), np.array([0, 1]))
    try:
        with pytest.raises(capi.FemusHipError, match="fh_mat_block_system_families: 5 variables"):
            small.block_system(5, sizes=[1] * 5)
        with pytest.raises(capi.FemusHipError, match="fh_mat_block_system_families: 0 variables"):
            small.block_system(0, sizes=[])
        with pytest.raises(capi.FemusHipError, match="fh_mat_block_system_families: variable 1 has 3 unknowns, 1 .. 2"):
            small.block_system(2, sizes=[2, 3])
        with pytest.raises(capi.FemusHipError, match="fh_mat_block_system_families: variable 0 has 0 unknowns"):
            small.block_system(2, sizes=[0, 1])
        with pytest.raises(ValueError, match="sizes has 1 entries, 2 are expected"):
            small.block_system(2, sizes=[1])
        with pytest.raises(capi.FemusHipError, match="fh_mat_block_diagonal_of: 5 variables"):
            capi.Mat.block_diagonal_of([small] * 5)
        with pytest.raises(capi.FemusHipError, match="fh_mat_block_diagonal_of: matrix 1 is null"):
            capi.Mat.block_diagonal_of([small, None])
        ok = capi.Mat.block_diagonal_of([small, small])           # the matrix is usable after the refusals
        assert (ok.m(), ok.n(), ok.nnz) == (4, 4, 4)
        ok.destroy()
    finally:
        small.destroy()
