"""The CSR structure kernels of femus_amd/csrc/fh_mat.hip on the designed inputs of tests/matrix_structure_cases.py: the device pattern builder
(k_pe_count, k_pe_fill, k_pe_rows) at and over its cap, the device transpose (k_tr_count, k_tr_fill, k_tr_sort) at and over its cap, the Dirichlet rows and
columns and the diagonal (k_zero_rows, k_zero_cols, k_diag_pos, k_get_diag) on square, wide and tall matrices, the restriction with its dropped maximum
(k_dropped_max), the value maps and gathers (k_gather_map), the masks, and the block matrices (k_block_system_cols, k_block_diagonal_fill).

Every comparison is exact (np.array_equal): these kernels move integers and copy doubles, there is no arithmetic to bound and no tolerance in this file.
The products that show a built matrix is usable multiply small integers, whose sums are exact in any order.  Mat.built_on() tells which builder ran.
Every refusal is one the host code raises before a launch -- except an element dof out of range, which k_pe_count flags and skips.

tests/test_matrix_structure_cases_host.py shows without a GPU that the cases are what they claim and that the references agree with scipy."""
import numpy as np
import pytest

import matrix_structure_cases as mc

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def destroy(*things):
    for t in things:
        if t is not None:
            t.destroy()


def upload(ctx, A, val=None):
    return ctx.matrix_csr(A.m, A.n, A.rowptr, A.col, A.val if val is None else val)


def assert_csr(Md, shape, rowptr, col, val=None):
    rp, c = Md.pattern()
    assert (Md.m_, Md.n_) == tuple(shape) and Md.nnz == len(col)
    assert np.array_equal(rp, rowptr) and np.array_equal(c, col)
    if val is not None:
        assert np.array_equal(bits(Md.values()), bits(val))


def mult(ctx, Md, x):
    xd, yd = ctx.vector_from(x), ctx.vector(Md.m_)
    try:
        yd.fill(SENTINEL)
        yd.matrix_mult(xd, Md)
        return yd.to_numpy()
    finally:
        destroy(xd, yd)


def assert_usable(ctx, Md, rowptr, col):
    """new values k + 1, one product against x = 1 .. n: small integers, exact"""
    val = np.arange(1.0, len(col) + 1)
    x = np.arange(1.0, Md.n_ + 1)
    Md.set_values(val)
    assert np.array_equal(mult(ctx, Md, x), mc.spmv_reference(rowptr, col, val, x))


# ---- pattern from elements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.TABLE_NAMES)
def test_pattern_from_elements(ctx, name):
    from femus_amd import capi
    t = mc.table(name)
    rowptr, col = mc.pattern_reference(t)
    A = B = None
    try:
        A = capi.Mat.from_elements(ctx, t.elem_dof, t.m, t.n)
        assert_csr(A, (t.m, t.n), rowptr, col, np.zeros(col.size))
        assert A.built_on() == mc.built_on_expected(t) == ("host_fallback" if name in mc.OVER_CAP else "device")
        # the project's claim: the same pattern as the host builder, row for row (the host builder makes all n rows; the first m are owned)
        hrp, hcol = capi.pattern_from_elements(t.elem_dof, t.n)
        rp, c = A.pattern()
        assert np.array_equal(rp, hrp[:t.m + 1])
        for r in range(t.m):
            assert np.array_equal(c[rp[r]:rp[r + 1]], hcol[hrp[r]:hrp[r + 1]]), "row %d" % r
        assert_usable(ctx, A, rowptr, col)
        # the order inside the dof lists races; the result must not
        B = capi.Mat.from_elements(ctx, t.elem_dof, t.m, t.n)
        assert B.built_on() == A.built_on()
        assert_csr(B, (t.m, t.n), rp, c, np.zeros(col.size))
    finally:
        destroy(A, B)


@pytest.mark.parametrize("name", sorted(mc.REFUSED_TABLES))
def test_pattern_from_elements_refusals(ctx, name):
    from femus_amd import capi
    t = mc.REFUSED_TABLES[name]
    with pytest.raises(capi.FemusHipError) as e:
        capi.Mat.from_elements(ctx, t.elem_dof, t.m, t.n)
    assert mc.REFUSAL in str(e.value)
    g = mc.table("star_16")
    A = capi.Mat.from_elements(ctx, g.elem_dof, g.m, g.n)
    try:
        assert_csr(A, (g.m, g.n), *mc.pattern_reference(g))
        assert A.built_on() == "device"
    finally:
        destroy(A)


# ---- transpose ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.TRANSPOSE_NAMES)
def test_transpose(ctx, name):
    A = mc.transpose_case(name)
    Ad = T1 = T2 = T3 = xd = yd = None
    try:
        Ad = upload(ctx, A)
        assert Ad.built_on() == "csr"
        rp, col, val = mc.transpose_reference(A)
        T1 = Ad.get_transpose()
        assert_csr(T1, (A.n, A.m), rp, col, val)
        assert T1.built_on() == A.design["built_on"]
        T2 = Ad.get_transpose()
        assert_csr(T2, (A.n, A.m), rp, col, val)
        assert T2.built_on() == T1.built_on()
        # the cached transpose of the product, built on the first values ...
        x = np.arange(1.0, A.m + 1)
        xd, yd = ctx.vector_from(x), ctx.vector(A.n)
        yd.matrix_mult_transpose(xd, Ad)
        assert np.array_equal(yd.to_numpy(), mc.spmv_reference(rp, col, val, x))
        # ... follows new values of the source, and so does a fresh transpose
        new = 2.0 * np.arange(A.nnz) + 7.0
        Ad.set_values(new)
        _, _, nval = mc.transpose_reference(A, new)
        yd.fill(SENTINEL)
        yd.matrix_mult_transpose(xd, Ad)
        assert np.array_equal(yd.to_numpy(), mc.spmv_reference(rp, col, nval, x))
        T3 = Ad.get_transpose()
        assert_csr(T3, (A.n, A.m), rp, col, nval)
        assert_csr(T1, (A.n, A.m), rp, col, val)                         # an explicit transpose is a matrix of its own
    finally:
        destroy(T1, T2, T3, Ad, xd, yd)


# ---- zero rows and columns, diagonal --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(mc.SHAPES))
def test_zero_rows(ctx, shape):
    from femus_amd import capi
    R = mc.rowop_case(shape)
    A = R.A
    Ad = upload(ctx, A)
    try:
        for n, rows in sorted(R.row_lists.items()):
            for diag in (1.0, -2.5):
                ref = mc.zero_rows_reference(A, A.val, rows, diag)
                untouched = ~np.isin(A.rows(), rows)
                Ad.set_values(A.val)
                Ad.mat_zero_rows(rows, diag)
                got = Ad.values()
                assert np.array_equal(bits(got), bits(ref)), "mat_zero_rows, list of %d, diag %g" % (n, diag)
                assert np.array_equal(bits(got[untouched]), bits(A.val[untouched]))
                Ad.set_values(A.val)
                idx = capi.Index(ctx, rows)
                try:
                    idx.zero_rows(Ad, diag)
                    got = Ad.values()
                finally:
                    idx.destroy()
                assert np.array_equal(bits(got), bits(ref)), "Index.zero_rows, list of %d, diag %g" % (n, diag)
                assert np.array_equal(bits(got[untouched]), bits(A.val[untouched]))
        assert_csr(Ad, (A.m, A.n), A.rowptr, A.col)
        # refused on the host, before any launch; the values stay
        Ad.set_values(A.val)
        for bad in ([0, A.m], [-1]):
            with pytest.raises(capi.FemusHipError):
                Ad.mat_zero_rows(bad, 1.0)
        assert np.array_equal(bits(Ad.values()), bits(A.val))
    finally:
        destroy(Ad)


@pytest.mark.parametrize("shape", sorted(mc.SHAPES))
def test_zero_cols(ctx, shape):
    R = mc.rowop_case(shape)
    A = R.A
    Ad = upload(ctx, A)
    try:
        for name, cols in sorted(R.col_lists.items()):
            ref = mc.zero_cols_reference(A, A.val, cols)
            untouched = ~np.isin(A.col, cols)
            Ad.set_values(A.val)
            Ad.zero_cols(cols)
            got = Ad.values()
            assert np.array_equal(bits(got), bits(ref)), name
            assert np.array_equal(bits(got[untouched]), bits(A.val[untouched]))
            if name == "empty":
                assert np.count_nonzero(got != A.val) == A.col_lengths()[5]
    finally:
        destroy(Ad)


@pytest.mark.parametrize("shape", sorted(mc.SHAPES))
def test_get_diagonal(ctx, shape):
    """into a vector of max(m, n) + 8 sentinels: the min(m, n) diagonal entries, 0.0 where a row has none, and every entry from min(m, n) on untouched (a tall
    matrix once wrote an entry for each of its m rows)"""
    R = mc.rowop_case(shape)
    A = R.A
    k = min(A.m, A.n)
    Ad, d = upload(ctx, A), ctx.vector(max(A.m, A.n) + 8)
    try:
        for val in (A.val, -3.0 * A.val):                                # the second call finds the cached diagonal positions
            Ad.set_values(val)
            d.fill(SENTINEL)
            Ad.get_diagonal(d)
            got = d.to_numpy()
            ref = mc.diagonal_reference(A, val)
            assert np.array_equal(bits(got[:k]), bits(ref))
            assert np.array_equal(got[:k] == 0.0, ~R.with_diag[:k])
            assert np.all(got[k:] == SENTINEL), "entries %s past min(m, n) = %d were written" % (np.flatnonzero(got[k:] != SENTINEL) + k, k)
    finally:
        destroy(Ad, d)


# ---- restrict, maps and gathers ---------------------------------------------------------------------------------------------------------
def test_restrict_and_regather(ctx):
    c = mc.restrict_case()
    A = c.A
    Ad = D = M = None
    try:
        Ad = upload(ctx, A)
        for newcol, ncols in ((c.newcol, c.ncols_new), (c.newcol_all, A.n)):
            rp, col, val, _ = mc.restrict_reference(A, A.val, c.rows, newcol)
            Ad.set_values(A.val)
            D, M = Ad.restrict(c.rows, newcol, ncols, check=False)
            assert_csr(D, (len(c.rows), ncols), rp, col, val)
            assert D.built_on() == "csr"
            new = 2.0 * np.arange(A.nnz) + 7.0
            Ad.set_values(new)
            assert np.array_equal(bits(D.values()), bits(val))
            M.gather_matrix_values(D, Ad)
            assert_csr(D, (len(c.rows), ncols), rp, col, mc.restrict_reference(A, new, c.rows, newcol)[2])
            destroy(D, M)
            D = M = None
    finally:
        destroy(D, M, Ad)


@pytest.mark.parametrize("variant", ["negative_max", "denormal", "late_in_row", "all_zero", "none_dropped"])
def test_restrict_check(ctx, variant):
    """the atomicMax on the bit pattern of a double returns the reference maximum itself"""
    c = mc.restrict_case()
    A = c.A
    val, newcol = (A.val, c.newcol_all) if variant == "none_dropped" else (c.values[variant], c.newcol)
    ref = mc.dropped_max_reference(A, val, c.rows, newcol)
    assert ref == {"negative_max": 7777.0, "denormal": 5e-324, "late_in_row": 99.5, "all_zero": 0.0, "none_dropped": 0.0}[variant]
    Ad = upload(ctx, A, val)
    D = M = None
    try:
        got = Ad.restrict_check(c.rows, newcol)
        assert bits([got])[0] == bits([ref])[0]
        assert Ad.restrict_check([], newcol) == 0.0
        if ref == 0.0:
            D, M = Ad.restrict(c.rows, newcol, A.n if variant == "none_dropped" else c.ncols_new, check=True)
            assert_csr(D, (len(c.rows), D.n_), *mc.restrict_reference(A, val, c.rows, newcol)[:3])
        else:
            with pytest.raises(AssertionError):
                Ad.restrict(c.rows, newcol, c.ncols_new, check=True)
    finally:
        destroy(D, M, Ad)


def test_value_map_and_gather(ctx):
    S = mc.rowop_case("square").A
    Sd = upload(ctx, S)
    try:
        for name, (D, src_row, src_col) in sorted(mc.value_map_cases().items()):
            mp = mc.value_map_reference(D, S, src_row, src_col)
            Dd = upload(ctx, D, np.full(D.nnz, SENTINEL))
            M = None
            try:
                M = Dd.value_map(Sd, src_row, src_col)
                M.gather_matrix_values(Dd, Sd)
                got = Dd.values()
                assert np.array_equal(bits(got), bits(mc.gather_reference(S.val, mp))), name
                assert np.all(got[mp < 0] == 0.0) and np.array_equal(got[mp >= 0], S.val[mp[mp >= 0]])
            finally:
                destroy(M, Dd)
    finally:
        destroy(Sd)


def test_gather_vector(ctx):
    """-1 entries give 0.0; a map shorter than dst leaves the tail alone"""
    from femus_amd import capi
    src = np.arange(1.0, 301.0) * 0.5
    mp = np.array([(37 * i + 5) % 300 if i % 6 else -1 for i in range(700)], dtype=np.int32)
    sd, dd, idx = ctx.vector_from(src), ctx.vector(711), None
    try:
        dd.fill(SENTINEL)
        idx = capi.Index(ctx, mp)
        idx.gather_vector(dd, sd)
        got = dd.to_numpy()
        assert np.array_equal(bits(got[:700]), bits(mc.gather_reference(src, mp)))
        assert np.all(got[700:] == SENTINEL)
    finally:
        destroy(idx, sd, dd)


@pytest.mark.parametrize("shape", sorted(mc.SHAPES))
def test_masks(ctx, shape):
    R = mc.rowop_case(shape)
    A = R.A
    Ad = upload(ctx, A)
    try:
        for rows in R.row_lists.values():
            assert np.array_equal(Ad.col_mask(rows), mc.col_mask_reference(A, rows))
            pre = np.zeros(A.n, dtype=np.uint8)
            pre[[0, A.n - 1, 7]] = 1                                      # or-ed into: the column n-1 holds nothing, only the given mask sets it
            got = Ad.col_mask(rows, pre.copy())
            assert np.array_equal(got, mc.col_mask_reference(A, rows, pre)) and got[A.n - 1] == 1
        for cols in ([3, 100], [R.empty_col], [], [A.n - 2, 0]):
            colmask = np.zeros(A.n, dtype=np.uint8)
            colmask[cols] = 1
            assert np.array_equal(Ad.row_mask(colmask), mc.row_mask_reference(A, colmask))
            pre = np.zeros(A.m, dtype=np.uint8)
            pre[[0, A.m - 1]] = 1                                         # row 0 is empty
            got = Ad.row_mask(colmask, pre.copy())
            assert np.array_equal(got, mc.row_mask_reference(A, colmask, pre)) and got[0] == 1
    finally:
        destroy(Ad)


def test_restrict_refusals(ctx):
    """each is raised by host code before a launch; the next correct call is served as if nothing had happened"""
    from femus_amd import capi
    c = mc.restrict_case()
    A = c.A
    Ad = upload(ctx, A)
    D = M = short = None

    def served():
        D, M = Ad.restrict(c.rows, c.newcol, c.ncols_new)
        try:
            assert_csr(D, (len(c.rows), c.ncols_new), *mc.restrict_reference(A, A.val, c.rows, c.newcol)[:3])
            assert Ad.restrict_check(c.rows, c.newcol_all) == 0.0
        finally:
            destroy(D, M)

    try:
        two = c.newcol.copy()
        row = A.row(c.rows[0])
        kept = row[c.newcol[row] >= 0]
        two[kept[1]] = two[kept[0]]                                      # two columns of a listed row onto one new column
        with pytest.raises(capi.FemusHipError, match="map to the same new column"):
            Ad.restrict(c.rows, two, c.ncols_new)
        served()
        with pytest.raises(capi.FemusHipError, match="new column .* out of range"):
            Ad.restrict(c.rows, c.newcol, c.ncols_new - 1)
        served()
        for bad in (c.rows + [A.m], [-1] + c.rows):
            with pytest.raises(capi.FemusHipError, match="fh_mat_restrict: row .* out of range"):
                Ad.restrict(bad, c.newcol, c.ncols_new)
            with pytest.raises(capi.FemusHipError, match="fh_mat_restrict_check: row .* out of range"):
                Ad.restrict_check(bad, c.newcol)
            with pytest.raises(capi.FemusHipError, match="row .* out of range"):
                Ad.col_mask(bad)
        served()
        D, M = Ad.restrict(c.rows, c.newcol, c.ncols_new)
        before = D.values()
        short = capi.Index(ctx, np.zeros(D.nnz - 1, dtype=np.int32))
        with pytest.raises(capi.FemusHipError, match="fh_mat_gather_values: map has"):
            short.gather_matrix_values(D, Ad)
        assert np.array_equal(bits(D.values()), bits(before))
        M.gather_matrix_values(D, Ad)
        assert np.array_equal(bits(D.values()), bits(before))
    finally:
        destroy(D, M, short, Ad)


# ---- block matrices ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.BLOCKS))
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_block_matrices(ctx, name, m):
    P = mc.block_case(name)
    Pd = upload(ctx, P)
    S = B = None
    try:
        rp, col = mc.block_system_reference(P, m)
        S = Pd.block_system(m)
        assert_csr(S, (P.m * m, P.n * m), rp, col, np.zeros(col.size))
        assert all(np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0) for r in range(P.m * m))
        assert S.built_on() == "device"
        assert_usable(ctx, S, rp, col)
        rp, col, val = mc.block_diagonal_reference(P, m)
        B = Pd.block_diagonal(m)
        assert_csr(B, (P.m * m, P.n * m), rp, col, val)
        assert B.built_on() == "device"
        x = np.arange(1.0, P.n * m + 1)
        assert np.array_equal(mult(ctx, B, x), mc.spmv_reference(rp, col, val, x))
    finally:
        destroy(S, B, Pd)


@pytest.mark.parametrize("m", [0, 5])
def test_block_matrices_refuse(ctx, m):
    from femus_amd import capi
    P = mc.block_case("empty_rows")
    Pd = upload(ctx, P)
    S = None
    try:
        with pytest.raises(capi.FemusHipError, match="1 .. 4 are served"):
            Pd.block_system(m)
        with pytest.raises(capi.FemusHipError, match="1 .. 4 are served"):
            Pd.block_diagonal(m)
        S = Pd.block_system(2)
        assert_csr(S, (P.m * 2, P.n * 2), *mc.block_system_reference(P, 2))
    finally:
        destroy(S, Pd)
