"""The designed inputs of tests/matrix_structure_cases.py, checked without a GPU: every design is what it claims (the candidate count of the marked row, the
column lengths, the row lengths, which lists are unsorted and repeat), and the plain numpy references agree with scipy where scipy has the operation
(A.T.tocsr(), sp.kron, fancy indexing).  tests/test_gpu_matrix_structure.py then holds the device to the same references, exactly."""
import numpy as np
import pytest
import scipy.sparse as sp

import matrix_structure_cases as mc


def scipy_of(A, val=None):
    return sp.csr_matrix((A.val if val is None else val, A.col, A.rowptr), shape=(A.m, A.n))


def sorted_csr(M):
    M = M.tocsr()
    M.sort_indices()
    return M


def test_padded_sizes():
    assert [mc.padded(n) for n in (0, 1, 64, 65, 128, 129, 1020, 1024)] == [64, 64, 64, 128, 128, 256, 1024, 1024]


# ---- element tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,nloc,count,np_,built", [
    ("star_16", 16, 4, 64, 64, "device"), ("star_17", 17, 4, 68, 128, "device"), ("star_255", 255, 4, 1020, 1024, "device"),
    ("star_256", 256, 4, 1024, 1024, "device"), ("star_257", 257, 4, 1028, None, "host_fallback"),
    ("star27_37", 37, 27, 999, 1024, "device"), ("star27_38", 38, 27, 1026, None, "host_fallback")])
def test_star_tables(name, K, nloc, count, np_, built):
    t = mc.table(name)
    c = mc.candidates(t)
    assert t.elem_dof.shape == (K, nloc) and t.m == t.n == (nloc - 1) * K + 1 < 1100
    assert t.design == {"row": 0, "candidates": count} and c[0] == count == c.max() and np.all(c[1:] == nloc)
    assert (count > mc.PE_CAP) == (built == "host_fallback") == (name in mc.OVER_CAP) and mc.built_on_expected(t) == built
    if np_:
        assert mc.padded(count) == np_
    assert np.all(np.diff(t.elem_dof, axis=1) < 0)                       # nothing arrives sorted
    shared = set(t.elem_dof[0])
    for e in t.elem_dof[1:]:
        shared &= set(e)
    assert shared == {0}
    rp, col = mc.pattern_reference(t)
    assert rp[1] == t.n and np.array_equal(col[:t.n], np.arange(t.n)) and np.all(np.diff(rp)[1:] == nloc)


def test_identical_256():
    t = mc.table("identical_256")
    c = mc.candidates(t)
    assert t.elem_dof.shape == (256, 4) and c[2] == c[4] == c[7] == c[9] == 1024 == mc.PE_CAP and c.sum() == 4 * 1024
    rp, col = mc.pattern_reference(t)
    assert np.array_equal(np.diff(rp), [0, 0, 4, 0, 4, 0, 0, 4, 0, 4]) and np.array_equal(col, [2, 4, 7, 9] * 4)
    # sorted, the 1024 keys are four runs of 256: with 16 keys per lane, every lane-chunk edge but three lies inside a run of equal keys
    assert mc.padded(1024) // mc.LANES == 16 and 256 % 16 == 0


def test_repeated_dof():
    t = mc.table("repeated_dof")
    assert [list(e).count(3) for e in t.elem_dof][0] == 2 and list(t.elem_dof[2]).count(0) == 2 and list(t.elem_dof[1]).count(5) == 3
    c = mc.candidates(t)
    assert c[5] == 4 * 4 and c[3] == 3 * 4 and c[0] == 3 * 4          # 5: three times in one element and once in another
    rp, col = mc.pattern_reference(t)
    assert list(col[rp[5]:rp[6]]) == [2, 3, 4, 5, 6] and list(col[rp[2]:rp[3]]) == [2, 5]


def test_rect_hole_empty_tables():
    t = mc.table("rect")
    assert t.m == 8 < t.n == 13 and set(range(8, 13)) <= set(t.elem_dof.ravel())
    rp, col = mc.pattern_reference(t)
    assert rp.size == 9 and col.max() == 12 and set(col[rp[0]:rp[1]]) == {0, 1, 6, 8, 10, 12}
    t0 = mc.table("rect_m0")
    assert t0.m == 0 and np.array_equal(t0.elem_dof, t.elem_dof)
    rp, col = mc.pattern_reference(t0)
    assert list(rp) == [0] and col.size == 0
    h = mc.table("hole")
    assert 3 not in h.elem_dof and h.design["empty_row"] == 3
    assert list(np.diff(mc.pattern_reference(h)[0])) == [3, 3, 5, 0, 4, 4, 3]
    e = mc.table("no_elements")
    assert e.elem_dof.shape == (0, 4) and e.m == 5 and list(mc.pattern_reference(e)[0]) == [0] * 6
    o = mc.table("nloc1")
    assert o.elem_dof.shape[1] == 1 and list(mc.candidates(o)) == [1, 1, 1, 0, 2, 0]
    rp, col = mc.pattern_reference(o)
    assert list(np.diff(rp)) == [1, 1, 1, 0, 1, 0] and list(col) == [0, 1, 2, 4]


def test_mixed_rows():
    t = mc.table("mixed_rows")
    assert tuple(mc.candidates(t)) == mc.MIXED_COUNTS == (1, 63, 64, 65, 127, 128, 129, 512, 513)
    assert sorted(set(mc.padded(c) for c in mc.MIXED_COUNTS)) == [64, 128, 256, 512, 1024]
    first = [np.flatnonzero(t.elem_dof[:, 0] == d) for d in range(t.m)]
    assert all(np.any(np.diff(f) > 1) for f in first[1:])                # no list stands in one piece
    rp, col = mc.pattern_reference(t)
    assert np.array_equal(col, np.arange(t.m)) and np.array_equal(rp, np.arange(t.m + 1))


@pytest.mark.parametrize("name", mc.TABLE_NAMES)
def test_pattern_reference_against_scipy(name):
    """the pattern of B^T B for the dof-by-element incidence B, cut to the owned rows"""
    t = mc.table(name)
    assert mc.built_on_expected(t) == ("host_fallback" if name in mc.OVER_CAP else "device")
    rp, col = mc.pattern_reference(t)
    nel, nloc = t.elem_dof.shape
    B = sp.csr_matrix((np.ones(nel * nloc), (np.repeat(np.arange(nel), nloc), t.elem_dof.ravel())), shape=(nel, t.n))
    P = sorted_csr((B.T @ B).tocsr()[:t.m])
    assert np.array_equal(P.indptr, rp) and np.array_equal(P.indices, col)
    assert all(np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0) for r in range(t.m))


def test_refused_tables():
    a, b = mc.REFUSED_TABLES["dof_equal_n"], mc.REFUSED_TABLES["dof_minus_one"]
    assert a.elem_dof.max() == a.n and a.elem_dof.min() >= 0
    assert b.elem_dof.min() == -1 and b.elem_dof.max() < b.n


# ---- transposes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,top", [("ladder", 1024), ("ladder_1025", 1025)])
def test_ladder(name, top):
    A = mc.transpose_case(name)
    cl, rl = A.col_lengths(), A.row_lengths()
    counts = A.design["counts"]
    assert np.array_equal(cl[:len(counts)], counts) and set(cl[len(counts):]) == {1, 2}
    assert set(mc.LADDER_COUNTS) <= set(cl) and all(counts.count(c) == 2 for c in mc.LADDER_COUNTS)
    assert cl.max() == top and A.design["built_on"] == ("device" if top <= mc.TR_CAP else "host_fallback")
    assert counts != sorted(counts) and counts != sorted(counts, reverse=True)
    assert rl[5] > 64 and rl[700] > 128 and rl[5] <= 128                 # k_tr_fill strides by 64: two and three trips
    assert 4500 < A.nnz < 7000 and np.array_equal(A.val, np.arange(1, A.nnz + 1))


@pytest.mark.parametrize("name", mc.TRANSPOSE_NAMES)
def test_transpose_reference_against_scipy(name):
    A = mc.transpose_case(name)
    for val in (A.val, 2.0 * np.arange(A.nnz) + 7.0):
        rp, col, v = mc.transpose_reference(A, val)
        T = sorted_csr(scipy_of(A, val).T)
        assert T.shape == (A.n, A.m) and np.array_equal(T.indptr, rp) and np.array_equal(T.indices, col) and np.array_equal(T.data, v)
    x = np.arange(1.0, A.n + 1)
    assert np.array_equal(mc.spmv_reference(A.rowptr, A.col, A.val, x), scipy_of(A) @ x)


def test_transpose_shapes():
    w, t, z, e = (mc.transpose_case(n) for n in ("wide", "tall", "nnz0", "m0"))
    assert w.m < w.n and t.m > t.n and w.nnz > 0 and t.col_lengths().max() < 128 and t.col_lengths().min() > 64
    assert z.nnz == 0 and z.m == 5 and z.n == 4 and e.m == 0 and e.n == 6 and e.nnz == 0
    assert z.design["built_on"] == e.design["built_on"] == "host_fallback"


# ---- row, column and diagonal operations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(mc.SHAPES))
def test_rowop_design(shape):
    R = mc.rowop_case(shape)
    A = R.A
    lens = A.row_lengths()
    assert (A.m < A.n) == (shape == "wide") and (A.m > A.n) == (shape == "tall")
    for L in mc.ROW_LENS:
        assert np.any(lens == L)
        if L:
            assert np.any((lens == L) & R.with_diag) and np.any((lens == L) & ~R.with_diag)
    assert np.array_equal(R.with_diag, [i in A.row(i) for i in range(A.m)])
    assert sorted(R.row_lists) == [1, 7, 8, 9]
    seen = set()
    for n, rows in R.row_lists.items():
        assert len(rows) == n and A.m - 1 in rows and all(0 <= r < A.m for r in rows)
        if n > 1:
            assert rows != sorted(rows) and len(set(rows)) < n          # unsorted, a row repeated
        seen |= set((int(lens[r]), bool(R.with_diag[r])) for r in rows)
    assert set(L for L, _ in seen) == set(mc.ROW_LENS) and {(200, True), (200, False), (33, True), (65, False), (1, False)} <= seen
    cl = A.col_lengths()
    assert cl[R.empty_col] == 0 and R.empty_col in R.col_lists["empty"]
    assert len(R.col_lists["repeats"]) > len(set(R.col_lists["repeats"]))
    assert all(cl[c] > 0 for name, cols in R.col_lists.items() for c in cols if c != R.empty_col)
    assert np.all(A.val != 0.0)


@pytest.mark.parametrize("shape", sorted(mc.SHAPES))
def test_rowop_references_against_scipy(shape):
    R = mc.rowop_case(shape)
    A = R.A
    S = scipy_of(A)
    d = mc.diagonal_reference(A, A.val)
    assert d.size == min(A.m, A.n) and np.array_equal(d, S.diagonal()) and np.array_equal(d != 0.0, R.with_diag[:d.size])
    for rows in R.row_lists.values():
        for diag in (1.0, -2.5):
            out = mc.zero_rows_reference(A, A.val, rows, diag)
            D = S.toarray()
            D[rows, :] = 0.0
            for r in rows:
                if R.with_diag[r]:
                    D[r, r] = diag
            assert np.array_equal(scipy_of(A, out).toarray(), D)
            untouched = ~np.isin(A.rows(), rows)
            assert np.array_equal(out[untouched], A.val[untouched])
    for cols in R.col_lists.values():
        D = S.toarray()
        D[:, cols] = 0.0
        assert np.array_equal(scipy_of(A, mc.zero_cols_reference(A, A.val, cols)).toarray(), D)


# ---- restriction, maps, masks -----------------------------------------------------------------------------------------------------------
def test_restrict_design():
    c = mc.restrict_case()
    A = c.A
    assert A.row_lengths().max() == 200 and c.rows != sorted(c.rows) and len(set(c.rows)) == len(c.rows) - 1 and len(c.rows) > 8
    kept = c.newcol >= 0
    assert (~kept).sum() == 42 and c.ncols_new == kept.sum() and sorted(c.newcol[kept]) == list(range(c.ncols_new))
    assert np.any(np.diff(c.newcol[kept]) < 0) and sorted(c.newcol_all) == list(range(A.n))
    new_in_row = [c.newcol[A.row(r)][c.newcol[A.row(r)] >= 0] for r in c.rows]
    assert any(np.any(np.diff(v) < 0) for v in new_in_row)                # the sort inside fh_mat_restrict matters
    listed = mc.dropped_positions(A, c.rows, c.newcol)
    v = c.values
    k = int(np.argmax(np.abs(v["negative_max"][listed])))
    assert v["negative_max"][listed][k] == -7777.0 and np.sort(v["negative_max"][listed])[-1] < 7777.0
    assert mc.dropped_max_reference(A, v["negative_max"], c.rows, c.newcol) == 7777.0
    d = v["denormal"][listed]
    assert np.count_nonzero(d) == 1 and d.max() == 5e-324 > 0.0 and mc.dropped_max_reference(A, v["denormal"], c.rows, c.newcol) == 5e-324
    k = listed[int(np.argmax(v["late_in_row"][listed]))]
    r = int(np.searchsorted(A.rowptr, k, side="right") - 1)
    assert k - A.rowptr[r] >= 64 and r in c.rows and mc.dropped_max_reference(A, v["late_in_row"], c.rows, c.newcol) == 99.5
    assert not np.any(v["all_zero"][listed]) and mc.dropped_max_reference(A, v["all_zero"], c.rows, c.newcol) == 0.0
    assert mc.dropped_positions(A, c.rows, c.newcol_all).size == 0 and mc.dropped_max_reference(A, A.val, c.rows, c.newcol_all) == 0.0
    for val in v.values():                                               # the row that is not listed holds a larger dropped value: it must not count
        assert mc.dropped_max_reference(A, val, [c.unlisted_row], c.newcol) == 1e300


@pytest.mark.parametrize("full", [False, True])
def test_restrict_reference_against_scipy(full):
    """fancy indexing: the listed rows, the kept columns in the order of their new numbers"""
    c = mc.restrict_case()
    A = c.A
    newcol = c.newcol_all if full else c.newcol
    ncols = A.n if full else c.ncols_new
    rp, col, val, mp = mc.restrict_reference(A, A.val, c.rows, newcol)
    old_of_new = np.empty(ncols, dtype=np.int64)
    old_of_new[newcol[newcol >= 0]] = np.flatnonzero(newcol >= 0)
    M = sorted_csr(scipy_of(A)[c.rows][:, old_of_new])
    assert M.shape == (len(c.rows), ncols) and np.array_equal(M.indptr, rp) and np.array_equal(M.indices, col) and np.array_equal(M.data, val)
    assert np.array_equal(A.val[mp], val) and np.array_equal(newcol[A.col[mp]], col)


def test_value_map_reference_against_scipy():
    S = mc.rowop_case("square").A
    dense = scipy_of(S).toarray()                                        # no stored value is zero: a zero of the dense copy is an entry S lacks
    for name, (D, src_row, src_col) in mc.value_map_cases().items():
        mp = mc.value_map_reference(D, S, src_row, src_col)
        sr = np.arange(D.m) if src_row is None else src_row
        sc = np.arange(D.n) if src_col is None else src_col
        r, cidx = sr[D.rows()], sc[D.col]
        want = np.where((r >= 0) & (cidx >= 0), dense[np.maximum(r, 0), np.maximum(cidx, 0)], 0.0)
        assert np.array_equal(mc.gather_reference(S.val, mp), want)
        assert np.any(mp < 0) and np.any(mp >= 0)
        if src_row is not None:
            lacks = (r >= 0) & (cidx >= 0) & (mp < 0)
            assert -1 in src_row and -1 in src_col and np.any(lacks) and np.any(np.diff(src_row) < 0) and np.any(np.diff(src_col) < 0)


def test_mask_references_against_scipy():
    R = mc.rowop_case("wide")
    A, S = R.A, scipy_of(R.A)
    rows = R.row_lists[7]
    pre = np.zeros(A.n, dtype=np.uint8)
    pre[[0, A.n - 1]] = 1
    cm = mc.col_mask_reference(A, rows, pre)
    want = np.asarray(abs(S[rows]).sum(axis=0)).ravel() > 0
    assert np.array_equal(cm.astype(bool), want | pre.astype(bool)) and cm[A.n - 1] == 1 and not want[A.n - 1]
    colmask = np.zeros(A.n, dtype=np.uint8)
    colmask[[3, 100]] = 1
    prer = np.zeros(A.m, dtype=np.uint8)
    prer[0] = 1                                                          # the empty row 0: only the or-ed-in mask sets it
    rm = mc.row_mask_reference(A, colmask, prer)
    want = np.asarray(abs(S[:, [3, 100]]).sum(axis=1)).ravel() > 0
    assert np.array_equal(rm.astype(bool), want | prer.astype(bool)) and not want[0] and 0 < want.sum() < A.m


# ---- block matrices ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.BLOCKS))
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_block_references_against_scipy(name, m):
    P = mc.block_case(name)
    assert np.any(P.row_lengths() == 0) and (P.m != P.n) == (name == "rectangular") and P.m * 4 > 256
    rp, col = mc.block_system_reference(P, m)
    K = sorted_csr(sp.kron(np.ones((m, m)), scipy_of(P, np.ones(P.nnz)), format="csr"))
    assert K.shape == (P.m * m, P.n * m) and np.array_equal(K.indptr, rp) and np.array_equal(K.indices, col)
    assert all(np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0) for r in range(P.m * m))
    rp, col, val = mc.block_diagonal_reference(P, m)
    K = sorted_csr(sp.kron(sp.identity(m), scipy_of(P), format="csr"))
    assert np.array_equal(K.indptr, rp) and np.array_equal(K.indices, col) and np.array_equal(K.data, val)
