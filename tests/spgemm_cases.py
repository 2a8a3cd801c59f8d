"""Operands with a DESIGNED path through the sparse products (femus_amd/csrc/fh_spgemm.hip), and a plain restatement of the rules the library chooses its
kernels by.  Imported by tests/test_spgemm_cases_host.py (which shows on a machine without a GPU that every case has the structure it claims and that
scipy's float64 product stays inside the bound the device is held to) and by tests/test_gpu_sparse_products.py (which compares the device with the
long-double restatement and asserts, through fh_mat_product_info, that each case took the path it was built for).

  case(name)      a triple (R, A, P) for D = R A P; R is None for "the transpose of P" (fh_mat_ptap).  `pair` names the product the case was designed for:
                  0 the inner one, A P; 1 the outer one, R (A P).  A case about one product C = A B is embedded as (S, A, B) or as (A, B, S) with S a
                  diagonal matrix, so that the designed product is the inner or the outer one of a triple product -- the product lists and the slots exist
                  only there -- and is the operand pair of the fh_mat_matmul tests as well
  expected_path   the library's choices, restated: numeric kernel, gl_log2, map sizes, device or host pattern, lanes_over_b
  sy_hash         the hash of the device pattern builder
  product_ld, triple_ld     C = A B and D = R A P in long double together with |A||B| and |R||A||P|: the yardstick, and the componentwise bound
                  |C - ref| <= (K + 2) 2^-52 |A||B|,  |D - ref| <= (K_R + K_A + 4) 2^-52 |R||A||P|     (K: the longest row of the left operand)
                  which holds for a sum of K products taken in any order, with or without fused multiply-add

Values are in +-(0.5, 1.5), so that nothing cancels exactly; the cases named cancel_* cancel on purpose (left operand of exact ones, B rows in pairs b, -b).
Nothing here comes from the device."""
import functools

import numpy as np
import scipy.sparse as sp

# ---- the limits of fh_spgemm.hip, restated ------------------------------------------------------------------------------------------
SY_TAB = 2048              # slots of the hash set of the device pattern builder
SY_CAP = 1024              # distinct columns of a row the device pattern builder sorts; one longer row sends the whole product to the host builder
LANES_MEAN = 24.0          # mean B row from which the device pattern builder puts the lanes over the B row
SLOTS_MEAN = 32.0          # mean B row from which the slots serve instead of the product lists
LISTS_CROW = 4000          # longest C row of the product lists (4 waves x (4000 + 1) ints of LDS)
LISTS_AROW = 2000          # longest A row of the product lists (4 waves x 2000 doubles of LDS; 16-bit offsets)
SLOTS_CROW = 2000          # longest C row of the slots (4 waves x 2000 doubles of LDS; 16-bit positions)
U = 2.0 ** -52


def _seed(*words):
    """a seed that does not depend on the hash randomisation of the interpreter"""
    s = 0
    for w in words:
        for ch in str(w):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def sy_hash(j):
    """the slot the device pattern builder tries first for column j"""
    return (((np.asarray(j, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(2 ** 32)) >> np.uint64(21)).astype(np.int64)


def expected_path(A, B, C, slot_map=1, device_symbolic=1):
    """what fh_mat_product_info reports for C = A B inside a triple product (C: the structural pattern), from the rules of build_slot_map and spgemm_pattern"""
    m = A.shape[0]
    blen, clen, alen = np.diff(B.indptr), np.diff(C.indptr), np.diff(A.indptr)
    mean = float(B.nnz) / max(B.shape[0], 1)
    max_crow = int(clen.max()) if m else 0
    max_arow = int(alen.max()) if m else 0
    products = int(blen[A.indices].sum())
    device = bool(device_symbolic) and m > 0 and A.nnz > 0 and B.nnz > 0 and max_crow <= SY_CAP
    out = {"kernel": "searching", "gl_log2": None, "products": 0, "max_crow": 0, "max_arow": 0,
           "pattern": "device" if device else "host", "lanes_over_b": (1 if mean >= LANES_MEAN else 0) if device else None}
    if not slot_map or m == 0 or max_crow == 0 or products == 0:
        return out
    if B.shape[0] > 0 and mean >= SLOTS_MEAN:
        if max_crow <= SLOTS_CROW:
            out.update(kernel="slots", products=products, max_crow=max_crow)
        return out
    if max_crow <= LISTS_CROW and max_arow <= LISTS_AROW:
        gl_log2 = 3
        while gl_log2 < 6 and float(1 << gl_log2) < mean:
            gl_log2 += 1
        out.update(kernel="lists", gl_log2=gl_log2, products=products, max_crow=max_crow, max_arow=max_arow)
    return out


def matmul_path(A, B, C, device_symbolic=1):
    """the same for a result of fh_mat_matmul: the searching kernel always"""
    return expected_path(A, B, C, slot_map=0, device_symbolic=device_symbolic)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
class Product:
    """a product on its structural pattern: indptr, indices (ascending in every row), val and absval in long double"""

    def __init__(self, shape, indptr, indices, val, absval):
        self.shape, self.indptr, self.indices, self.val, self.absval = shape, indptr, indices, val, absval

    def pattern(self):
        return sp.csr_matrix((np.ones(self.indices.size), self.indices, self.indptr), shape=self.shape)


def _product(shape, a_ptr, a_col, a_val, a_abs, b_ptr, b_col, b_val, b_abs):
    """every elementary product a_ik b_kj, listed row by row of A, entry by entry, in increasing k; the entries of C are the sums of their products
    in that order, in long double"""
    m, n = shape
    blen = np.diff(b_ptr)[a_col]
    tot = int(blen.sum())
    ea = np.repeat(np.arange(a_col.size), blen)
    eb = np.repeat(b_ptr[a_col].astype(np.int64), blen) + (np.arange(tot) - np.repeat(np.cumsum(blen) - blen, blen))
    i = np.repeat(np.arange(m), np.diff(a_ptr))[ea]
    key = i.astype(np.int64) * n + b_col[eb]
    order = np.argsort(key, kind="stable")
    key = key[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if tot else np.zeros(0, np.int64)
    prod, aprod = (a_val[ea] * b_val[eb])[order], (a_abs[ea] * b_abs[eb])[order]
    assert prod.dtype == np.longdouble
    val = np.add.reduceat(prod, first) if tot else np.zeros(0, np.longdouble)
    absval = np.add.reduceat(aprod, first) if tot else np.zeros(0, np.longdouble)
    rows, cols = key[first] // n, key[first] % n
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    return Product(shape, indptr, cols.astype(np.int32), val, absval)


def _ld(x):
    return np.asarray(x, dtype=np.longdouble)


def product_ld(A, B):
    """C = A B and |A||B| in long double"""
    return _product((A.shape[0], B.shape[1]), A.indptr, A.indices, _ld(A.data), _ld(np.abs(A.data)), B.indptr, B.indices, _ld(B.data), _ld(np.abs(B.data)))


def triple_ld(R, A, P):
    """(A P, R A P) in long double, the inner product not rounded to double in between; absval of the second is |R||A||P|"""
    AP = product_ld(A, P)
    return AP, _product((R.shape[0], P.shape[1]), R.indptr, R.indices, _ld(R.data), _ld(np.abs(R.data)), AP.indptr, AP.indices, AP.val, AP.absval)


def longest_row(M):
    return int(np.diff(M.indptr).max()) if M.shape[0] else 0


def ratio(val, ref, k):
    """largest |val - ref| / (k 2^-52 absval) over the entries: the bound holds when this is at most 1"""
    if ref.val.size == 0:
        return 0.0
    return float(np.max(np.abs(_ld(val) - ref.val) / (k * _ld(U) * ref.absval)))


def on_pattern(S, ref):
    """the values of the scipy matrix S on the pattern of ref (scipy may drop entries that cancel to zero: they are zeros here)"""
    S = S.tocsr()
    S.sort_indices()
    n = ref.shape[1]
    key_ref = np.repeat(np.arange(ref.shape[0], dtype=np.int64), np.diff(ref.indptr)) * n + ref.indices
    key_s = np.repeat(np.arange(S.shape[0], dtype=np.int64), np.diff(S.indptr)) * n + S.indices
    pos = np.searchsorted(key_ref, key_s)
    assert np.all(pos < key_ref.size) and np.array_equal(key_ref[pos], key_s), "an entry outside the structural pattern"
    out = np.zeros(key_ref.size)
    out[pos] = S.data
    return out


# ---- building blocks ----------------------------------------------------------------------------------------------------------------
def _vals(rng, k):
    return rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k)


def from_rows(rows, ncols, rng, values=None):
    """CSR matrix with the given columns in every row (sorted here), values in +-(0.5, 1.5) unless given"""
    rows = [np.sort(np.asarray(r, dtype=np.int64)) for r in rows]
    for r in rows:
        assert r.size == 0 or (np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < ncols), "a column twice or out of range"
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    indices = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)
    data = _vals(rng, indices.size) if values is None else np.full(indices.size, values, dtype=np.float64)
    return sp.csr_matrix((data, indices, indptr), shape=(len(rows), ncols))


def scaling(n, rng, exact=False):
    """a diagonal matrix: the trivial factor that makes a product of two the inner or the outer product of a triple product"""
    return from_rows([[i] for i in range(n)], n, rng, values=1.0 if exact else None)


def revalued(M, seed):
    """the pattern of M with other values: what a second assembly writes"""
    rng = np.random.default_rng(_seed("revalued", M.shape, M.nnz, seed))
    return sp.csr_matrix((_vals(rng, M.nnz), M.indices.copy(), M.indptr.copy()), shape=M.shape)


def random_rows(m, ncols, rng, most, empty_runs=()):
    """rows of 0 .. most distinct random columns; the rows in the runs [a, b) of empty_runs stay empty"""
    rows = [rng.permutation(ncols)[:int(rng.integers(0, min(most, ncols) + 1))] for _ in range(m)]
    for a, b in empty_runs:
        for i in range(a, min(b, m)):
            rows[i] = np.zeros(0, np.int64)
    return rows


class Case:
    def __init__(self, name, R, A, P, pair, design=None):
        self.name, self.R, self.A, self.P, self.pair, self.design = name, R, A, P, pair, dict(design or {})
        for M in (A, P) + (() if R is None else (R,)):
            assert M.has_canonical_format and M.indices.dtype == np.int32

    def Rx(self):
        """R as a matrix of its own"""
        if self.R is not None:
            return self.R
        T = self.P.T.tocsr()
        T.sort_indices()
        return T

    def designed(self):
        """the operands (A, B) of the product this case was built for; the B of an outer product is the inner product rounded to double"""
        if self.pair == 0:
            return self.A, self.P
        AP = product_ld(self.A, self.P)
        return self.Rx(), sp.csr_matrix((AP.val.astype(np.float64), AP.indices, AP.indptr), shape=AP.shape)

    def paths(self, slot_map=1, device_symbolic=1):
        """expected_path of the inner and of the outer product"""
        AP = product_ld(self.A, self.P).pattern()
        R = self.Rx()
        D = product_ld(R, AP).pattern()
        return [expected_path(self.A, self.P, AP, slot_map, device_symbolic), expected_path(R, AP, D, slot_map, device_symbolic)]


def inner(name, A, B, rng, design=None, exact=False):
    return Case(name, scaling(A.shape[0], rng, exact), A, B, 0, design)


def outer(name, A, B, rng, design=None, exact=False):
    return Case(name, A, B, scaling(B.shape[1], rng, exact), 1, design)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
MEAN_B = {"mean_b_8": (8, 0), "mean_b_8_above": (8, 1), "mean_b_16": (16, 0), "mean_b_16_above": (16, 1), "mean_b_24_below": (24, -1),
          "mean_b_24": (24, 0), "mean_b_32_below": (32, -1), "mean_b_32": (32, 0)}
MEAN_B_HEAD = (0, 0, 0, 1, 1, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 70, 100)


def _mean_b(name):
    """P^T A P with the mean row of P set to the entry: nnz(P) = mean * rows + delta.  The rows of P range from 0 to 100 entries (MEAN_B_HEAD); the others,
    of two neighbouring lengths, and the empty and one-entry rows set the mean"""
    mean, delta = MEAN_B[name]
    rng = np.random.default_rng(_seed(name))
    n, nc = 163, 200
    rest = mean * n + delta - sum(MEAN_B_HEAD)
    q, r = divmod(rest, n - len(MEAN_B_HEAD))
    lens = list(MEAN_B_HEAD) + [q + 1] * r + [q] * (n - len(MEAN_B_HEAD) - r)
    lens = [lens[i] for i in rng.permutation(n)]
    P = from_rows([rng.permutation(nc)[:k] for k in lens], nc, rng)
    A = from_rows(random_rows(n, n, rng, 10, empty_runs=((40, 47), (n - 3, n))), n, rng)
    return Case(name, None, A, P, 0, {"mean_b": (mean * n + delta, n)})


PLACES = {"first": 0, "middle": 101, "last": 202}


def _long_row(name):
    """one product whose limit row sits first, in the middle or last among 203 rows (not a multiple of the 4 rows of a workgroup):
    lists_crow_N   B rows of about 20 entries (lists); the limit row of A names 200 of them with disjoint columns: a C row of N = 4000 / 4001 entries
    slots_crow_N   B rows of about 40 entries (slots); the limit row names 50 with disjoint columns: N = 2000 / 2001
    lists_arow_N   B rows of 0 to 2 entries in 40 columns; the limit row of A has N = 2000 / 2001 entries"""
    kind, what, count, place = name.split("_")
    count, at, m = int(count), PLACES[place], 203
    rng = np.random.default_rng(_seed(name))
    if what == "crow":
        nrows, width, nb = (200, 20, 260) if kind == "lists" else (50, 40, 60)
        nc = count + 100
        perm = rng.permutation(nc)
        lens = [width] * nrows
        lens[int(rng.integers(nrows))] += count - nrows * width
        cuts = np.concatenate([[0], np.cumsum(lens)])
        brows = [perm[cuts[t]:cuts[t + 1]] for t in range(nrows)]
        brows += [rng.permutation(nc)[:int(rng.integers(width - 10, width + 11))] for _ in range(nb - nrows)]
        arows = random_rows(m, nb, rng, 4, empty_runs=((10, 14),))
        arows[at] = np.arange(nrows)
    else:
        nb, nc = 2100, 40
        brows = random_rows(nb, nc, rng, 2)
        arows = random_rows(m, nb, rng, 6, empty_runs=((10, 14),))
        arows[at] = rng.permutation(nb)[:count]
    A, B = from_rows(arows, nb, rng), from_rows(brows, nc, rng)
    design = {"row": at, ("c_row" if what == "crow" else "a_row"): count}
    return (outer if place == "middle" else inner)(name, A, B, rng, design)


COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024)


def _pattern_counts(name):
    """rows of C with COUNTS distinct columns (and 1025 in the cases named so): row t of A names B rows that cut a set of COUNTS[t] columns into chunks of 16
    (short B rows: one lane per B row) or 48 (long: the lanes over the B row); with dup, three times as many B rows again, random subsets of the same set.
    Two more rows: an empty row of A, and one that names empty rows of B only"""
    rng = np.random.default_rng(_seed(name))
    counts = COUNTS + ((1025,) if "1025" in name else ())
    chunk, dup, nc = (48 if "long_b" in name else 16), "dup" in name, 1500
    brows, arows = [], []
    for d in counts:
        cols = np.sort(rng.permutation(nc)[:d])
        mine = [cols[s:s + chunk] for s in range(0, d, chunk)]
        if dup and d:
            mine += [rng.permutation(cols)[:min(chunk, d)] for _ in range(3 * len(mine))]
        arows.append(np.arange(len(brows), len(brows) + len(mine)))
        brows += mine
    empties = np.arange(len(brows), len(brows) + 3)
    brows += [np.zeros(0, np.int64)] * 3
    arows += [np.zeros(0, np.int64), empties]
    order = rng.permutation(len(arows))
    A, B = from_rows([arows[i] for i in order], len(brows), rng), from_rows(brows, nc, rng)
    return inner(name, A, B, rng, {"counts": sorted(counts + (0, 0))})


HASH_COLS = 1500000         # columns to choose from: about 730 fall on every slot of the table


def _hash(name):
    """rows whose columns are chosen with the builder's own hash:
    hash_one_slot    600 columns that all fall on slot 777: a probe chain of 600
    hash_wrap        300 columns that all fall on slot 2040: the chain runs past 2047 to 0 and on to 291
    hash_over_half   1100 distinct columns: more than half the table, beyond what the builder sorts -- the host builder serves
    hash_overfull    2100 distinct columns: the table itself is full, the probe loop gives up"""
    rng = np.random.default_rng(_seed(name))
    h = sy_hash(np.arange(HASH_COLS))
    if name == "hash_one_slot":
        cols = np.flatnonzero(h == 777)[:600]
    elif name == "hash_wrap":
        cols = np.flatnonzero(h == 2040)[:300]
    else:
        cols = np.sort(rng.permutation(HASH_COLS)[:1100 if name == "hash_over_half" else 2100])
    cols = rng.permutation(cols)
    brows = [cols[s:s + 12] for s in range(0, cols.size, 12)]
    chain = len(brows)
    brows += [rng.permutation(HASH_COLS)[:int(rng.integers(0, 13))] for _ in range(20)]
    arows = random_rows(9, len(brows), rng, 5)
    arows[4] = np.arange(chain)
    arows[6] = np.concatenate([np.arange(0, chain, 3), [chain + 1, chain + 7]])       # part of the chain and others
    A, B = from_rows(arows, len(brows), rng), from_rows(brows, HASH_COLS, rng)
    return inner(name, A, B, rng, {"row": 4, "columns": np.sort(cols)})


def _two_builders(name):
    """R A P whose inner pattern stays below 1024 columns a row (device builder) and whose outer pattern has a row of 1200 (host builder)"""
    rng = np.random.default_rng(_seed(name))
    n, nc = 80, 2500
    perm = rng.permutation(nc)
    P = from_rows([perm[30 * i:30 * i + 30] for i in range(n)], nc, rng)
    A = from_rows([[i] for i in range(n)], n, rng)
    rrows = random_rows(5, n, rng, 3)
    rrows[2] = rng.permutation(n)[:40]
    return Case(name, from_rows(rrows, n, rng), A, P, 1, {"row": 2, "c_row": 1200})


ENTRY_PRODUCTS = (1, 2, 3, 4, 5, 63, 64, 65)
ENTRY_FILL = {"entry_products_gl3": 0, "entry_products_gl4": 79, "entry_products_gl5": 527}


def _entry_products(name):
    """row 3 of A has 65 entries; column c_p of B stands in the first p of the 65 B rows they name, so the entry (3, c_p) of C is made of p elementary
    products, p in ENTRY_PRODUCTS: lists shorter than, equal to and longer than the 4 lanes of an entry and the 16 entries of a pass.  Full rows of B that
    nobody names lift the mean B row, and with it gl_log2, to 4 and 5"""
    rng = np.random.default_rng(_seed(name))
    nc, colof = 20, dict(zip(ENTRY_PRODUCTS, (1, 3, 4, 7, 9, 12, 15, 19)))
    brows = [[colof[p] for p in ENTRY_PRODUCTS if p > t] for t in range(65)] + [[]] * 5 + [np.arange(nc)] * ENTRY_FILL[name]
    arows = random_rows(7, 70, rng, 6)
    arows[0], arows[3], arows[5] = [], np.arange(65), [10, 65, 66, 69]          # 65 .. 69: empty rows of B
    A, B = from_rows(arows, len(brows), rng), from_rows(brows, nc, rng)
    return (outer if name.endswith("gl4") else inner)(name, A, B, rng, {"row": 3, "columns": colof})


CROWS = (15, 16, 17, 2000)


def _crow_lengths(name):
    """C rows of 15, 16, 17 and 2000 entries (16 entries a pass in the list kernel) from B rows of 5 and fewer disjoint columns"""
    rng = np.random.default_rng(_seed(name))
    nc = 2100
    brows, arows = [], []
    for d in CROWS:
        cols = rng.permutation(nc)[:d]
        mine = [cols[s:s + 5] for s in range(0, d, 5)]
        arows.append(np.arange(len(brows), len(brows) + len(mine)))
        brows += mine
    arows = [arows[0], [], arows[1], arows[3], arows[2]]
    A, B = from_rows(arows, len(brows), rng), from_rows(brows, nc, rng)
    return inner(name, A, B, rng, {"c_rows": [15, 0, 16, 2000, 17]})


def _empty_rows(name):
    """P^T A P with runs of empty rows in A, empty rows and an empty column in P, entries of A that point at empty rows of P, and a row of A that points at
    nothing else"""
    rng = np.random.default_rng(_seed(name))
    n, nc = 50, 21
    prows = random_rows(n, nc - 1, rng, 6, empty_runs=((3, 6), (30, 34)))          # column 20 stays empty: an empty row of R
    arows = random_rows(n, n, rng, 8, empty_runs=((0, 7), (20, 31), (47, 50)))
    arows[12] = [3, 4, 5, 31, 33]
    return Case(name, None, from_rows(arows, n, rng), from_rows(prows, nc, rng), 0, {"row": 12})


def _no_entries(name):
    """every entry of A points at an empty row of B: a product without a single entry"""
    rng = np.random.default_rng(_seed(name))
    brows = [[], [0, 2], [], [1], []]
    arows = [[0, 2], [], [4], [0, 2, 4], [2], []]
    return inner(name, from_rows(arows, 5, rng), from_rows(brows, 3, rng), rng)


def _tiny(name):
    rng = np.random.default_rng(_seed(name))
    if name == "one_by_one":
        return Case(name, None, from_rows([[0]], 1, rng), from_rows([[0]], 1, rng), 0)
    if name == "one_row":
        n = 37
        return Case(name, from_rows([rng.permutation(n)[:9]], n, rng), from_rows(random_rows(n, n, rng, 6), n, rng), from_rows(random_rows(n, 11, rng, 4), 11, rng), 1)
    if name == "one_column":
        n = 37
        return Case(name, None, from_rows(random_rows(n, n, rng, 6), n, rng), from_rows([[0]] * 20 + [[]] * (n - 20), 1, rng), 0)
    m = int(name[2:])
    full = [np.arange(m)] * m
    return Case(name, None, from_rows(full, m, rng), from_rows([np.arange(max(m - 1, 1))] * m, max(m - 1, 1), rng), 0)


def _cancel(name):
    """the left operand holds exact ones; the rows of B come in pairs b, -b on one pattern and a row of A names both or neither: every entry of C is an exact
    zero when summed in increasing k, with or without fused multiply-add (1 * b is exact), and the structural pattern keeps it.  A kernel that sums in another
    order may leave a rounding error of b_1 + b_2 there: the bound, which is taken from |A||B| > 0, allows that.  cancel_inner: in A P; cancel_outer: in R (A P)"""
    rng = np.random.default_rng(_seed(name))
    npair, nc, m = 12, 30, 11
    base = from_rows(random_rows(npair, nc, rng, 7)[:-1] + [np.arange(0, nc, 3)], nc, rng)
    B = sp.vstack([base, -base]).tocsr()[np.arange(2 * npair).reshape(2, npair).T.ravel()]        # rows 2t, 2t + 1 = b_t, -b_t
    B.sort_indices()
    B = sp.csr_matrix((B.data, B.indices.astype(np.int32), B.indptr.astype(np.int32)), shape=B.shape)
    arows = []
    for i in range(m):
        t = rng.permutation(npair)[:int(rng.integers(1, 5))]
        arows.append(np.concatenate([2 * t, 2 * t + 1]))
    arows[5] = []
    A = from_rows(arows, 2 * npair, rng, values=1.0)
    return (inner if name == "cancel_inner" else outer)(name, A, B, rng, exact=True)


BUILDERS = {}
for _n in MEAN_B:
    BUILDERS[_n] = _mean_b
for _k, _w, _c in (("lists", "crow", 4000), ("lists", "crow", 4001), ("slots", "crow", 2000), ("slots", "crow", 2001), ("lists", "arow", 2000), ("lists", "arow", 2001)):
    for _p in PLACES:
        BUILDERS["%s_%s_%d_%s" % (_k, _w, _c, _p)] = _long_row
for _n in ("pattern_counts_short_b", "pattern_counts_long_b", "pattern_counts_dup_short_b", "pattern_counts_dup_long_b",
           "pattern_1025_short_b", "pattern_1025_long_b", "pattern_1025_dup_short_b"):
    BUILDERS[_n] = _pattern_counts
for _n in ("hash_one_slot", "hash_wrap", "hash_over_half", "hash_overfull"):
    BUILDERS[_n] = _hash
BUILDERS["two_builders"] = _two_builders
for _n in ENTRY_FILL:
    BUILDERS[_n] = _entry_products
BUILDERS["crow_lengths"] = _crow_lengths
BUILDERS["empty_rows"] = _empty_rows
BUILDERS["no_entries"] = _no_entries
for _n in ("one_by_one", "one_row", "one_column", "m_1", "m_2", "m_3", "m_4", "m_5"):
    BUILDERS[_n] = _tiny
for _n in ("cancel_inner", "cancel_outer"):
    BUILDERS[_n] = _cancel
NAMES = tuple(BUILDERS)
PTAP_NAMES = tuple(MEAN_B) + ("empty_rows", "one_by_one", "one_column", "m_1", "m_2", "m_3", "m_4", "m_5")       # the cases whose R is the transpose of P


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name](name)


@functools.lru_cache(maxsize=None)
def reference(name, new_a=0, new_p=0):
    """(R, A, P, A P, R A P) of a case in long double, for the values of the case or for the revalued A (seed new_a) / P (seed new_p); with R None, R follows P"""
    c = case(name)
    A = revalued(c.A, new_a) if new_a else c.A
    P = revalued(c.P, new_p) if new_p else c.P
    if c.R is None:
        R = P.T.tocsr()
        R.sort_indices()
    else:
        R = c.R
    return (R, A, P) + triple_ld(R, A, P)
