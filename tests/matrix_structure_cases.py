"""Inputs with a DESIGNED path through the CSR structure kernels (femus_amd/csrc/fh_mat.hip), each with its reference in plain numpy: sets and sorting for
patterns, index arithmetic for values -- no call into the library and no scipy in a reference.  Imported by tests/test_matrix_structure_cases_host.py
(which shows without a GPU that every design is what it claims -- candidate counts, column lengths, row lengths -- and that the references agree with
scipy where scipy has the operation) and by tests/test_gpu_matrix_structure.py (which holds the device to the references, exactly: these kernels move
integers and copy doubles).

  element tables    table(name) -> Table(elem_dof, m, n, design): m owned rows over n columns (fh_mat_create_from_elements);
                    reference pattern_reference(), candidate counts candidates()
  transposes        transpose_case(name) -> Csr with design: reference transpose_reference()
  row / column ops  rowop_case(shape) -> RowOps: the matrix, row lists, column lists; references zero_rows_reference, zero_cols_reference, diagonal_reference
  restriction       restrict_case() -> Restrict: source, rows, newcol, value variants for the dropped maximum; references restrict_reference,
                    dropped_max_reference, value_map_reference, col_mask_reference, row_mask_reference
  block matrices    block_case(name) -> Csr; references block_system_reference, block_diagonal_reference
  spmv_reference    y = A x by index arithmetic (small integers: exact in any order)

Nothing here comes from the device."""
import functools

import numpy as np

# ---- the limits of fh_mat.hip, restated ---------------------------------------------------------------------------------------------
PE_CAP = 1024              # candidate columns of a row the device pattern builder sorts; one row over it sends the whole matrix to the host builder
TR_CAP = 1024              # entries of a column the device transpose sorts; one column over it sends the whole transpose to the host loop
LANES = 64


def padded(n):
    """the power of two >= 64 the bitonic sorts pad n keys to"""
    p = LANES
    while p < n:
        p *= 2
    return p


class Csr:
    """rowptr, col (ascending in every row), val; `design` says what the case is made to hit"""

    def __init__(self, m, n, rowptr, col, val=None, design=None):
        self.m, self.n = int(m), int(n)
        self.rowptr = np.asarray(rowptr, dtype=np.int32)
        self.col = np.asarray(col, dtype=np.int32)
        self.val = np.arange(1, self.col.size + 1, dtype=np.float64) if val is None else np.asarray(val, dtype=np.float64)
        self.design = design or {}
        assert self.rowptr.size == self.m + 1 and self.rowptr[-1] == self.col.size == self.val.size

    @property
    def nnz(self):
        return int(self.col.size)

    def rows(self):
        """the row of every entry"""
        return np.repeat(np.arange(self.m, dtype=np.int64), np.diff(self.rowptr))

    def row_lengths(self):
        return np.diff(self.rowptr)

    def col_lengths(self):
        return np.bincount(self.col, minlength=self.n)

    def row(self, i):
        return self.col[self.rowptr[i]:self.rowptr[i + 1]]


def csr_from_rows(m, n, rows, val=None, design=None):
    """rows: one iterable of columns per row; sorted here, must be distinct"""
    cols = [np.array(sorted(r), dtype=np.int64) for r in rows]
    assert len(cols) == m and all(c.size == np.unique(c).size and (c.size == 0 or (c[0] >= 0 and c[-1] < n)) for c in cols)
    rowptr = np.concatenate([[0], np.cumsum([c.size for c in cols])])
    col = np.concatenate(cols) if cols and rowptr[-1] else np.zeros(0, np.int64)
    return Csr(m, n, rowptr, col, val, design)


def spmv_reference(rowptr, col, val, x):
    """y = A x, entry by entry"""
    m = len(rowptr) - 1
    y = np.zeros(m)
    np.add.at(y, np.repeat(np.arange(m), np.diff(rowptr)), np.asarray(val, dtype=np.float64) * np.asarray(x, dtype=np.float64)[col])
    return y


# ---- element tables -----------------------------------------------------------------------------------------------------------------
class Table:
    def __init__(self, elem_dof, m, n, **design):
        self.elem_dof = np.ascontiguousarray(elem_dof, dtype=np.int32)
        assert self.elem_dof.ndim == 2
        self.m, self.n, self.design = int(m), int(n), design


def candidates(t):
    """candidate columns of every owned row, as k_pe_rows counts them: the dof's occurrences in the table times nloc (an element that lists the dof twice
    stands twice in its list)"""
    nloc = t.elem_dof.shape[1]
    return np.bincount(t.elem_dof.ravel(), minlength=t.n)[:t.m] * nloc


def built_on_expected(t):
    c = candidates(t)
    return "host_fallback" if c.size and c.max() > PE_CAP else "device"


def pattern_reference(t):
    """row r: the dofs of all elements that hold r, as a sorted set"""
    rows = [set() for _ in range(t.m)]
    for e in t.elem_dof:
        dofs = set(int(d) for d in e)
        for d in dofs:
            if d < t.m:
                rows[d] |= dofs
    cols = [sorted(s) for s in rows]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    col = np.array([c for r in cols for c in r], dtype=np.int32)
    return rowptr, col


def _star(K, nloc):
    """K elements share dof 0 and nothing else; every element lists its dofs in descending order"""
    ed = np.zeros((K, nloc), dtype=np.int64)
    for e in range(K):
        ed[e] = np.arange((nloc - 1) * (e + 1), (nloc - 1) * e, -1).tolist() + [0]
    n = (nloc - 1) * K + 1
    return Table(ed, n, n, row=0, candidates=K * nloc)


def _identical_256():
    return Table(np.tile([7, 2, 9, 4], (256, 1)), 10, 10, row=2, candidates=1024, distinct=4)


def _repeated_dof():
    """elements that list a dof twice (3 in the first, 0 in the third) and three times (5 in the second)"""
    ed = [[3, 1, 3, 0], [5, 5, 2, 5], [0, 4, 0, 6], [6, 5, 4, 3]]
    return Table(ed, 7, 7, twice=(3, 0), thrice=5)


def _rect_table():
    """8 owned rows over 13 columns: the dofs 8 .. 12 appear as columns and own no row"""
    return [[12, 0, 8, 1], [1, 9, 2, 10], [7, 11, 3, 2], [4, 5, 6, 7], [10, 6, 0, 12]]


def _rect():
    return Table(_rect_table(), 8, 13)


def _rect_m0():
    return Table(_rect_table(), 0, 13)


def _hole():
    """no element holds dof 3: an empty row between full ones"""
    return Table([[2, 1, 0], [4, 2, 5], [6, 5, 4]], 7, 7, empty_row=3)


def _no_elements():
    return Table(np.zeros((0, 4), dtype=np.int32), 5, 5)


def _nloc1():
    return Table([[4], [0], [2], [4], [1]], 6, 6)


MIXED_COUNTS = (1, 63, 64, 65, 127, 128, 129, 512, 513)


def _mixed_rows():
    """nloc = 1 (the only width at which a row can have ONE candidate): dof d stands MIXED_COUNTS[d] times in the table, interleaved so that no list arrives in one
    piece; every key of a row is equal, so every lane-chunk edge of every padded size 64 .. 1024 lies inside a run of equal keys"""
    dofs = np.concatenate([np.full(c, d) for d, c in enumerate(MIXED_COUNTS)])
    order = np.argsort((np.arange(dofs.size) * 7919) % dofs.size, kind="stable")
    return Table(dofs[order].reshape(-1, 1), len(MIXED_COUNTS), len(MIXED_COUNTS), counts=MIXED_COUNTS)


TABLES = {
    "star_16": lambda: _star(16, 4), "star_17": lambda: _star(17, 4), "star_255": lambda: _star(255, 4), "star_256": lambda: _star(256, 4),
    "star_257": lambda: _star(257, 4), "star27_37": lambda: _star(37, 27), "star27_38": lambda: _star(38, 27),
    "identical_256": _identical_256, "repeated_dof": _repeated_dof, "rect": _rect, "rect_m0": _rect_m0, "hole": _hole, "no_elements": _no_elements,
    "nloc1": _nloc1, "mixed_rows": _mixed_rows,
}
TABLE_NAMES = sorted(TABLES)
OVER_CAP = ("star27_38", "star_257")            # the tables designed to be over PE_CAP: the host builder makes the whole matrix
# refused by fh_dof_lists_build before any row is built: (elem_dof, m, n)
REFUSED_TABLES = {
    "dof_equal_n": Table([[0, 1, 2], [2, 3, 5]], 5, 5),
    "dof_minus_one": Table([[0, 1, 2], [2, -1, 4]], 5, 5),
}
REFUSAL = "fh_mat_create_from_elements: a dof of an element is out of range"


@functools.lru_cache(maxsize=None)
def table(name):
    return TABLES[name]()


# ---- matrices for the transpose -----------------------------------------------------------------------------------------------------
LADDER_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024)
LONG_ROWS = ((5, 70), (700, 140))               # (source row, extra columns it alone or with the other fills): rows of more than 64 and more than 128 entries


def _ladder(extra_count=None):
    """m = 1024 rows (1025 with the column of 1025).  Every count of LADDER_COUNTS twice, the two columns of a count with different row strides, the counts not
    in order; column j of count c holds the rows (a i + b) mod m, i < c, a coprime to m.  Then 140 columns that only serve to make rows 5 and 700 long."""
    m = 1024 if extra_count is None else extra_count
    counts = list(LADDER_COUNTS[::-1]) + list(LADDER_COUNTS[1::2]) + list(LADDER_COUNTS[0::2])
    if extra_count is not None:
        counts.insert(7, extra_count)
    strides = [s for s in range(1, 200, 2) if s % 5 and s % 41]          # coprime to 1024 and to 1025 = 5 5 41
    entries = []
    for j, c in enumerate(counts):
        a, b = strides[j], 37 * j
        rows = (a * np.arange(c, dtype=np.int64) + b) % m
        assert np.unique(rows).size == c
        entries += [(int(r), j) for r in rows]
    nl = len(counts)
    for t in range(LONG_ROWS[1][1]):
        entries.append((LONG_ROWS[1][0], nl + t))
        if t < LONG_ROWS[0][1]:
            entries.append((LONG_ROWS[0][0], nl + t))
    n = nl + LONG_ROWS[1][1]
    rows = [[] for _ in range(m)]
    for r, j in entries:
        rows[r].append(j)
    built = "device" if max(counts) <= TR_CAP else "host_fallback"
    return csr_from_rows(m, n, rows, design={"counts": counts, "built_on": built})


def _lattice(m, n):
    """entry (i, j) where (5 i + 3 j) mod 7 < 2"""
    return csr_from_rows(m, n, [[j for j in range(n) if (5 * i + 3 * j) % 7 < 2] for i in range(m)], design={"built_on": "device"})


# a source without non-zeros: build_transpose launches nothing and leaves the matrix to the host loop (read off fh_mat.hip: `if (nnz == 0) return build_transpose_host`)
TRANSPOSES = {
    "ladder": _ladder, "ladder_1025": lambda: _ladder(1025), "wide": lambda: _lattice(7, 300), "tall": lambda: _lattice(300, 7),
    "nnz0": lambda: Csr(5, 4, np.zeros(6), [], design={"built_on": "host_fallback"}),
    "m0": lambda: Csr(0, 6, np.zeros(1), [], design={"built_on": "host_fallback"}),
}
TRANSPOSE_NAMES = sorted(TRANSPOSES)


@functools.lru_cache(maxsize=None)
def transpose_case(name):
    return TRANSPOSES[name]()


def transpose_reference(A, val=None):
    """(rowptr, col, val) of the transpose: the entries sorted by (column, row)"""
    val = A.val if val is None else np.asarray(val, dtype=np.float64)
    rows = A.rows()
    order = np.lexsort((rows, A.col))
    rowptr = np.concatenate([[0], np.cumsum(A.col_lengths())]).astype(np.int32)
    return rowptr, rows[order].astype(np.int32), val[order]


# ---- matrices for the row, column and diagonal operations ------------------------------------------------------------------------------
ROW_LENS = (0, 1, 31, 32, 33, 64, 65, 200)
SHAPES = {"square": (210, 210), "wide": (24, 230), "tall": (260, 210)}


class RowOps:
    def __init__(self, A, with_diag, row_lists, col_lists, empty_col):
        self.A, self.with_diag, self.row_lists, self.col_lists, self.empty_col = A, with_diag, row_lists, col_lists, empty_col


def _window_matrix(m, n, shift=0):
    """row i has ROW_LENS[i % 8] entries in a cyclic window over the columns 0 .. n-2 (column n-1 holds nothing); in every other group of eight rows the window
    is centred on the diagonal, in the others it starts right after it"""
    w = n - 1
    rows, with_diag = [], []
    for i in range(m):
        L = ROW_LENS[i % 8]
        centred = (i // 8) % 2 == 0
        start = (i - L // 2 if centred else i + 1) + shift
        cols = sorted(set((start + t) % w for t in range(L)))
        assert len(cols) == L
        rows.append(cols)
        with_diag.append(i in cols)
    return rows, np.array(with_diag)


@functools.lru_cache(maxsize=None)
def rowop_case(shape):
    m, n = SHAPES[shape]
    rows, with_diag = _window_matrix(m, n)
    nnz = sum(len(r) for r in rows)
    k = np.arange(nnz)
    A = csr_from_rows(m, n, rows, val=np.where(k % 3 == 0, -1.0, 1.0) * (k + 1.5))
    lens = A.row_lengths()

    def pick(L, diag):
        hits = [i for i in range(m) if lens[i] == L and bool(with_diag[i]) == diag]
        assert hits, (shape, L, diag)
        return hits[-1]

    last = m - 1
    r200d, r200n, r33d, r65n, r64d, r1d, r1n, r32n, r31d, r0 = (pick(200, True), pick(200, False), pick(33, True), pick(65, False), pick(64, True),
                                                               pick(1, True), pick(1, False), pick(32, False), pick(31, True), pick(0, False))
    row_lists = {
        1: [last],
        7: [r200n, r33d, last, r0, r1n, r33d, r64d],
        8: [r65n, last, r200d, r1d, r32n, r0, r200d, r31d],
        9: [r200d, r33d, last, r0, r65n, r33d, r64d, r1n, r32n],
    }
    empty_col = n - 1
    col_lists = {"one": [3], "repeats": [17, 3, n - 2, 17, 0, 3], "empty": [empty_col, 5, empty_col], "last_used": [n - 2]}
    return RowOps(A, with_diag, row_lists, col_lists, empty_col)


def zero_rows_reference(A, val, rows, diag):
    """a loop over the pattern: every entry of a listed row becomes 0, its diagonal entry -- where the row has one -- diag"""
    out = np.array(val, dtype=np.float64)
    for r in rows:
        for k in range(A.rowptr[r], A.rowptr[r + 1]):
            out[k] = diag if A.col[k] == r else 0.0
    return out


def zero_cols_reference(A, val, cols):
    out = np.array(val, dtype=np.float64)
    out[np.isin(A.col, np.asarray(cols))] = 0.0
    return out


def diagonal_reference(A, val):
    """the min(m, n) diagonal entries, 0.0 where a row has none"""
    d = np.zeros(min(A.m, A.n))
    for i in range(d.size):
        for k in range(A.rowptr[i], A.rowptr[i + 1]):
            if A.col[k] == i:
                d[i] = val[k]
    return d


# ---- restriction, value maps, masks ------------------------------------------------------------------------------------------------------
class Restrict:
    def __init__(self, A, rows, newcol, ncols_new, newcol_all, values, unlisted_row):
        self.A, self.rows, self.newcol, self.ncols_new, self.newcol_all, self.values, self.unlisted_row = A, rows, newcol, ncols_new, newcol_all, values, unlisted_row


def dropped_positions(A, rows, newcol):
    """positions of the entries of the listed rows whose new column is < 0"""
    return np.array([k for r in rows for k in range(A.rowptr[r], A.rowptr[r + 1]) if newcol[A.col[k]] < 0], dtype=np.int64)


def dropped_max_reference(A, val, rows, newcol):
    k = dropped_positions(A, rows, newcol)
    return float(np.max(np.abs(np.asarray(val)[k]))) if k.size else 0.0


@functools.lru_cache(maxsize=None)
def restrict_case():
    """source: the square matrix of the row operations (rows of up to 200 entries).  newcol: every column c with c % 5 == 3 is dropped, the others are renumbered by
    the rank of (37 c + 11) mod n -- injective and not monotone, so the new columns of a row do not arrive sorted.  rows: unsorted, one repeated, ten of them (three
    workgroups of k_dropped_max)."""
    R = rowop_case("square")
    A = R.A
    n = A.n
    key = (37 * np.arange(n) + 11) % n
    kept = np.arange(n) % 5 != 3
    newcol = np.full(n, -1, dtype=np.int32)
    newcol[kept] = np.argsort(np.argsort(key[kept]))
    newcol_all = np.argsort(np.argsort(key)).astype(np.int32)
    lens = A.row_lengths()
    long_rows = [i for i in range(A.m) if lens[i] == 200]
    rows = [long_rows[1], 40, 3, 209, long_rows[0], 40, 17, 88, 9, 130]
    unlisted_row = long_rows[2]
    assert unlisted_row not in rows
    base = A.val.copy()
    listed = dropped_positions(A, rows, newcol)
    unlisted = dropped_positions(A, [unlisted_row], newcol)
    assert listed.size and unlisted.size
    late = [k for k in dropped_positions(A, [long_rows[0]], newcol) if k - A.rowptr[long_rows[0]] >= 64]
    assert late

    def variant(fill, at=None, value=None):
        v = base.copy()
        v[listed] = fill(listed)
        v[unlisted] = 1e300                  # a row that is not listed must not count
        if at is not None:
            v[at] = value
        return v

    small = lambda k: 0.25 + (k % 7)
    values = {
        "negative_max": variant(small, listed[listed.size // 2], -7777.0),
        "denormal": variant(lambda k: np.zeros(k.size), listed[3], 5e-324),
        "late_in_row": variant(small, late[-1], 99.5),
        "all_zero": variant(lambda k: np.zeros(k.size)),
    }
    return Restrict(A, rows, newcol, int(kept.sum()), newcol_all, values, unlisted_row)


def restrict_reference(A, val, rows, newcol):
    """(rowptr, col, val, map): the listed rows in list order, the kept entries of each sorted by their new column; map names the source position"""
    rp, col, mp = [0], [], []
    for r in rows:
        pairs = sorted((int(newcol[A.col[k]]), k) for k in range(A.rowptr[r], A.rowptr[r + 1]) if newcol[A.col[k]] >= 0)
        col += [p[0] for p in pairs]
        mp += [p[1] for p in pairs]
        rp.append(len(col))
    mp = np.array(mp, dtype=np.int64)
    return np.array(rp, dtype=np.int32), np.array(col, dtype=np.int32), np.asarray(val, dtype=np.float64)[mp], mp


def value_map_reference(D, S, src_row=None, src_col=None):
    """map[k] for the entry k = (r, c) of D: the position of (src_row[r], src_col[c]) in S, -1 where a list says -1 or S has no such entry"""
    where = {}
    for i in range(S.m):
        for k in range(S.rowptr[i], S.rowptr[i + 1]):
            where[(i, int(S.col[k]))] = k
    out = np.full(D.nnz, -1, dtype=np.int64)
    for r in range(D.m):
        sr = r if src_row is None else int(src_row[r])
        for k in range(D.rowptr[r], D.rowptr[r + 1]):
            sc = int(D.col[k]) if src_col is None else int(src_col[D.col[k]])
            if sr >= 0 and sc >= 0:
                out[k] = where.get((sr, sc), -1)
    return out


def gather_reference(src_val, mp):
    mp = np.asarray(mp)
    return np.where(mp >= 0, np.asarray(src_val, dtype=np.float64)[np.maximum(mp, 0)], 0.0)


@functools.lru_cache(maxsize=None)
def value_map_cases():
    """name -> (D, src_row, src_col) against the square matrix S of the row operations.
    lists: a 12 x 15 target whose rows and columns point into S out of order, some at -1, some at entries S lacks.
    identity: S's own shape with every window moved three columns on -- part of every row is in S, part is not; lists None."""
    S = rowop_case("square").A
    src_row = np.array([200, -1, 7, 199, 64, 0, -1, 135, 7, 209, 31, 100], dtype=np.int32)
    src_col = np.array([150, 3, -1, 100, 0, 208, 99, 101, -1, 50, 7, 209, 200, 120, 60], dtype=np.int32)
    D = csr_from_rows(12, 15, [[j for j in range(15) if (i + 2 * j) % 3 != 1] for i in range(12)])
    rows, _ = _window_matrix(S.m, S.n, shift=3)
    I = csr_from_rows(S.m, S.n, rows)
    return {"lists": (D, src_row, src_col), "identity": (I, None, None)}


def col_mask_reference(A, rows, mask=None):
    out = np.zeros(A.n, dtype=np.uint8) if mask is None else np.array(mask, dtype=np.uint8)
    for r in rows:
        out[A.row(r)] = 1
    return out


def row_mask_reference(A, colmask, mask=None):
    out = np.zeros(A.m, dtype=np.uint8) if mask is None else np.array(mask, dtype=np.uint8)
    for r in range(A.m):
        if np.any(np.asarray(colmask)[A.row(r)]):
            out[r] = 1
    return out


# ---- block matrices ----------------------------------------------------------------------------------------------------------------------
def _with_empty_rows():
    """70 x 70, the rows 0, 13, 14 and 69 empty: 70 rows times m^2 = 4 is more than one workgroup of k_block_system_cols"""
    return csr_from_rows(70, 70, [[] if i in (0, 13, 14, 69) else [j for j in range(70) if (3 * i + 5 * j) % 11 < 3] for i in range(70)])


def _rectangular():
    """70 x 30 (a transfer is tall), row 20 empty"""
    return csr_from_rows(70, 30, [[] if i == 20 else [j for j in range(30) if (i + 7 * j) % 6 < 2] for i in range(70)])


BLOCKS = {"empty_rows": _with_empty_rows, "rectangular": _rectangular}


@functools.lru_cache(maxsize=None)
def block_case(name):
    return BLOCKS[name]()


def block_system_reference(S, m):
    """kron(ones(m, m), S): row (k, i) holds the columns of row i of S once per block l, shifted by l n"""
    rp, col = [0], []
    for k in range(m):
        for i in range(S.m):
            for l in range(m):
                col += [l * S.n + int(c) for c in S.row(i)]
            rp.append(len(col))
    return np.array(rp, dtype=np.int32), np.array(col, dtype=np.int32)


def block_diagonal_reference(P, m):
    """kron(I_m, P): row (k, i) is row i of P with its columns shifted by k n"""
    rp, col, val = [0], [], []
    for k in range(m):
        for i in range(P.m):
            s, e = P.rowptr[i], P.rowptr[i + 1]
            col += [k * P.n + int(c) for c in P.col[s:e]]
            val += list(P.val[s:e])
            rp.append(len(col))
    return np.array(rp, dtype=np.int32), np.array(col, dtype=np.int32), np.array(val, dtype=np.float64)
