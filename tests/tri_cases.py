"""Matrices with a DESIGNED level schedule for the natural-order sweeps (femus_amd/csrc/fh_trisolve.hip), and a plain restatement of the rules the
library plans a sweep by.  Imported by tests/test_tri_cases_host.py (which shows on a machine without a GPU that every case has the level structure
it claims and that the float64 oracle is good enough a reference) and by tests/test_gpu_tri_sweeps.py (which compares the device with the oracle
on them and asserts, through fh_mg_sweep_info, that each case took the path it was built for).

  layered     rows numbered layer by layer; a row of layer k has lower entries only in layers k-reach .. k-1 (one at least in k-1), upper entries
              only in layers k+1 .. k+reach (one at least in k+1), nothing but the diagonal inside its layer: its forward level IS its layer, its
              backward level the layer counted from the end.  Unsymmetric pattern, values in (-1, 1), diagonal = row sum of |a_ij| + 1
  ilu_row     a band with one row (and its column) widened to a given number of entries: the row-length limits of the ILU(0) kernels
  schedule, segments, slots, sources, plan     the library's planning rules, restated
  sor_symmetric_ld, ilu0_factor_ld, ilu0_apply_ld     the sweeps as sequential loops in long double: the yardstick for the float64 oracle

Nothing here comes from the device."""
import functools

import numpy as np
import scipy.sparse as sp

TRI_SMALL = 256                 # rows of a small level
TRI_SMALL_WORK = 32768          # entries of a small level, whole rows
TRI_RING = 2                    # levels the run kernel keeps in LDS: the one in work and the one before
GROUPS = 64                     # rows of a level that the run kernel takes from its pipeline's registers; the rest of the level takes the second path
SEPARATOR = TRI_SMALL + 1       # a layer of this many rows gets a launch of its own
LENS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100)       # triangle lengths: both sides of 16 PF entries for PF = 2 and 4, and well into the tail loop


def _seed(*words):
    """a seed that does not depend on the hash randomisation of the interpreter"""
    s = 0
    for w in words:
        for ch in str(w):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def _finish(n, rows, cols, rng):
    """CSR matrix of the off-diagonal pattern (rows, cols): values uniform in (-1, 1), diagonal = row sum of |a_ij| + 1"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    assert not np.any(rows == cols)
    S = sp.csr_matrix((rng.uniform(-1.0, 1.0, rows.size), (rows, cols)), shape=(n, n))
    assert S.nnz == rows.size, "an entry was given twice"
    M = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()
    M.sort_indices()
    return M


def layered(sizes, lower, upper, reach=1, seed=0):
    """(M, layer of every row).  lower(k, rank, size) / upper(k, rank, size): the number of entries asked for left / right of the diagonal of row `rank` of
    layer k; cut to what the layers in reach hold, and at least 1 where a layer before / after exists at all."""
    sizes = [int(s) for s in sizes]
    K, start = len(sizes), np.concatenate([[0], np.cumsum(sizes)])
    n = int(start[-1])
    rng = np.random.default_rng(_seed("layered", sizes, reach, seed))
    rows, cols = [], []
    for k in range(K):
        for rank in range(sizes[k]):
            i = start[k] + rank
            for want, near, far in ((lower(k, rank, sizes[k]), k - 1, max(k - reach, 0)), (upper(k, rank, sizes[k]), k + 1, min(k + reach, K - 1))):
                if near < 0 or near >= K:
                    continue                                           # first layer: no lower part; last layer: no upper part
                lo, hi = min(near, far), max(near, far)
                pool = np.arange(start[lo], start[hi + 1])
                want = int(min(max(want, 1), pool.size))
                must = start[near] + rng.integers(sizes[near])          # the entry that pins the row's level
                rest = pool[pool != must]
                pick = np.concatenate([[must], rng.permutation(rest)[:want - 1]])
                rows += [i] * pick.size
                cols += pick.tolist()
    return _finish(n, rows, cols, rng), np.repeat(np.arange(K), sizes)


def revalued(M, seed=1):
    """the pattern of M with other values (same rule): what a second assembly writes into the operator"""
    rng = np.random.default_rng(_seed("revalued", M.shape, M.nnz, seed))
    C = M.tocoo()
    off = C.row != C.col
    return _finish(M.shape[0], C.row[off], C.col[off], rng)


def ilu_row(width, n=1500, at=700, seed=0):
    """a band (i +- 1 always, i +- 2 and i +- 3 with probability 0.6) of n rows; row `at` widened to exactly `width` entries, about half of them left of the
    diagonal (hundreds of pivots), and column `at` by the transposed positions.  The sub- and superdiagonal make n levels of one row in both directions."""
    rng = np.random.default_rng(_seed("ilu_row", width, n, at, seed))
    pat = set()
    for i in range(n):
        for d in (1, 2, 3):
            for j in (i - d, i + d):
                if 0 <= j < n and (d == 1 or rng.uniform() < 0.6):
                    pat.add((i, j))
    have_l = sorted(j for (i, j) in pat if i == at and j < at)
    have_u = sorted(j for (i, j) in pat if i == at and j > at)
    nl = (width - 1) // 2
    nu = width - 1 - nl
    assert len(have_l) <= nl <= at and len(have_u) <= nu <= n - at - 1
    more_l = rng.permutation(np.setdiff1d(np.arange(at), have_l))[:nl - len(have_l)]
    more_u = rng.permutation(np.setdiff1d(np.arange(at + 1, n), have_u))[:nu - len(have_u)]
    for j in np.concatenate([more_l, more_u]).tolist():
        pat.add((at, j))
        pat.add((j, at))
    pat = sorted(pat)
    return _finish(n, [p[0] for p in pat], [p[1] for p in pat], rng)


# ---- the planning rules of fh_trisolve.hip, restated -----------------------------------------------------------------------------
def schedule(M, forward):
    """level of every row: 1 + the largest level among the rows it reads (forward: columns j < i; backward: j > i), 0 where it reads none"""
    ip, ix, n = M.indptr, M.indices, M.shape[0]
    lev = np.zeros(n, dtype=np.int64)
    for i in (range(n) if forward else range(n - 1, -1, -1)):
        c = ix[ip[i]:ip[i + 1]]
        c = c[c < i] if forward else c[c > i]
        if c.size:
            lev[i] = lev[c].max() + 1
    return lev


def segments(M, lev, tri_runs=True):
    """[(first level, levels, is a run)]: a level is small with at most TRI_SMALL rows and at most TRI_SMALL_WORK entries over its whole rows; consecutive
    small levels form one run (one workgroup), every other level has a launch of its own"""
    nl = int(lev.max()) + 1 if lev.size else 0
    rows = np.bincount(lev, minlength=nl)
    work = np.bincount(lev, weights=np.diff(M.indptr), minlength=nl)
    small = (rows <= TRI_SMALL) & (work <= TRI_SMALL_WORK) & bool(tri_runs)
    seg, l = [], 0
    while l < nl:
        if not small[l]:
            seg.append((l, 1, False))
            l += 1
            continue
        e = l
        while e < nl and small[e]:
            e += 1
        seg.append((l, e - l, True))
        l = e
    return seg


def triangle_lengths(M):
    C = M.tocoo()
    n = M.shape[0]
    return np.bincount(C.row[C.col < C.row], minlength=n), np.bincount(C.row[C.col > C.row], minlength=n)


def percentile90(lengths):
    """the smallest length v such that at least 90 % of the rows have a triangle of at most v entries (lengths above 1023 count as 1023)"""
    h = np.bincount(np.minimum(lengths, 1023), minlength=1024)
    acc = 0
    for v in range(1024):
        acc += int(h[v])
        if float(acc) >= 0.9 * lengths.size:
            return v
    return 1023


def slots(lengths):
    """register slots per lane of the run kernel (PF): 2 while the 90th percentile of the direction's triangle lengths is at most 32, else 4"""
    return 2 if percentile90(lengths) <= 32 else 4


def sources(M, lev, seg, forward, pf):
    """where the run kernel takes the operands of a sweep from, counted over the entries of the direction's triangles of the rows inside runs.
    An operand computed by the level JUST BEFORE, inside the same run, comes from LDS; every other one from global memory.  The first GROUPS rows of a
    level go through the pipeline's registers -- entry p of a triangle sits in slot p // 16 of its lane, the slots from pf on are the tail loop --, the
    other rows through the second path.  Keys: (path, source) with path in "registers", "tail", "second" and source in "lds", "global"."""
    n = M.shape[0]
    nl = int(lev.max()) + 1 if n else 0
    run_first = np.full(max(nl, 1), -1)
    for l0, cnt, is_run in seg:
        if is_run:
            run_first[l0:l0 + cnt] = l0
    order = np.lexsort((np.arange(n), lev))                           # ascending row index inside a level
    rank = np.empty(n, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(np.bincount(lev, minlength=nl))])
    rank[order] = np.arange(n) - first[lev[order]]
    C = M.tocoo()                                                     # canonical CSR: entries in row order, columns ascending
    i, j = C.row.astype(np.int64), C.col.astype(np.int64)
    low, up = triangle_lengths(M)
    offset = np.arange(M.nnz) - M.indptr[i]                           # position inside the whole row
    takes = (j < i) if forward else (j > i)
    p = offset if forward else offset - (low[i] + 1)                  # position inside the triangle
    in_run = run_first[lev[i]] >= 0
    lds = in_run & (lev[j] < lev[i]) & (lev[i] - lev[j] < TRI_RING) & (lev[j] >= run_first[lev[i]])
    path = np.where(rank[i] >= GROUPS, 2, np.where(p // 16 >= pf, 1, 0))
    out = {}
    for q, pname in enumerate(("registers", "tail", "second")):
        for src, sname in ((True, "lds"), (False, "global")):
            out[(pname, sname)] = int(np.sum(takes & in_run & (path == q) & (lds == src)))
    return out


def plan(M, tri_runs=True):
    """what fh_mg_sweep_info reports per direction for this matrix, from the rules above; "run_lengths", "alone" (sizes of the levels with a launch of their
    own), "sources" and "lengths" (triangle lengths of the rows that go through the registers of a run) describe the case beyond that"""
    low, up = triangle_lengths(M)
    out = {}
    for name, forward, lengths in (("forward", True, low), ("backward", False, up)):
        lev = schedule(M, forward)
        seg = segments(M, lev, tri_runs)
        size = np.bincount(lev)
        runs = [s for s in seg if s[2]]
        pf = slots(lengths)
        info = {"levels": int(size.size), "runs": len(runs), "levels_in_runs": sum(s[1] for s in runs), "longest_run": max([s[1] for s in runs] + [0]),
                "largest_level_in_run": max([int(size[s[0]:s[0] + s[1]].max()) for s in runs] + [0]), "slots": pf}
        order = np.lexsort((np.arange(M.shape[0]), lev))
        first = np.concatenate([[0], np.cumsum(size)])
        rank = np.empty(M.shape[0], dtype=np.int64)
        rank[order] = np.arange(M.shape[0]) - first[lev[order]]
        in_run = np.zeros(size.size, dtype=bool)
        for s in runs:
            in_run[s[0]:s[0] + s[1]] = True
        out[name] = {"info": info, "level": lev, "segments": seg, "run_lengths": [s[1] for s in runs], "run_starts": [s[0] for s in runs],
                     "alone": [int(size[s[0]]) for s in seg if not s[2]], "sizes": size, "sources": sources(M, lev, seg, forward, pf),
                     "lengths": sorted(set(lengths[in_run[lev] & (rank < GROUPS)].tolist())), "p90": percentile90(lengths)}
    return out


def ilu_kernel(max_row, row_limit, ilu_ahead=2):
    """the factorisation kernel fh_tri_ilu_factor chooses for a longest row, given the limits fh_mg_sweep_info reports for the device"""
    if ilu_ahead and max_row <= row_limit["ahead"]:
        return "plan" if ilu_ahead >= 2 and max_row <= row_limit["plan"] else "ahead"
    return "lds_columns" if max_row <= row_limit["lds_columns"] else "plain"


# ---- the sweeps as sequential loops, in any dtype -------------------------------------------------------------------------------
def sor_symmetric_ld(M, r, dtype=np.longdouble):
    """PCSOR, omega = 1, one symmetric sweep from zero: forward t_i = r_i - sum_{j<i} a_ij z_j, z_i = t_i / a_ii; backward z_i = (t_i - sum_{j>i} a_ij z_j) / a_ii"""
    ip, ix, n = M.indptr, M.indices, M.shape[0]
    v, r = M.data.astype(dtype), np.asarray(r).astype(dtype)
    d = M.diagonal().astype(dtype)
    z, t = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for i in range(n):
        c, a = ix[ip[i]:ip[i + 1]], v[ip[i]:ip[i + 1]]
        m = c < i
        t[i] = r[i] - a[m] @ z[c[m]]
        z[i] = t[i] / d[i]
    for i in range(n - 1, -1, -1):
        c, a = ix[ip[i]:ip[i + 1]], v[ip[i]:ip[i + 1]]
        m = c > i
        z[i] = (t[i] - a[m] @ z[c[m]]) / d[i]
    return z


def ilu0_factor_ld(M, dtype=np.longdouble):
    """ILU(0) in natural order on M's pattern, IKJ form, no shift (the cases are diagonally dominant: asserted).  Returns the factors on the pattern:
    strict lower part L (unit diagonal), the rest U"""
    ip, ix, n = M.indptr, M.indices, M.shape[0]
    v = M.data.astype(dtype)
    dpos = np.array([ip[i] + np.searchsorted(ix[ip[i]:ip[i + 1]], i) for i in range(n)])
    assert np.all(ix[dpos] == np.arange(n))
    for i in range(n):
        rs, re = ip[i], ip[i + 1]
        cols = ix[rs:re]
        for p in range(rs, dpos[i]):
            k = ix[p]
            lik = v[p] / v[dpos[k]]
            v[p] = lik
            kc = ix[dpos[k] + 1:ip[k + 1]]
            pos = np.searchsorted(cols, kc)
            hit = (pos < cols.size) & (cols[np.minimum(pos, cols.size - 1)] == kc)
            v[rs + pos[hit]] -= lik * v[dpos[k] + 1:ip[k + 1]][hit]
        assert abs(v[dpos[i]]) > 1e-16 * np.abs(v[dpos[i] + 1:re]).sum()
    return v, dpos


def ilu0_apply_ld(M, factors, r):
    ip, ix, n = M.indptr, M.indices, M.shape[0]
    v, dpos = factors
    z = np.asarray(r).astype(v.dtype)
    for i in range(n):
        z[i] -= v[ip[i]:dpos[i]] @ z[ix[ip[i]:dpos[i]]]
    for i in range(n - 1, -1, -1):
        z[i] = (z[i] - v[dpos[i] + 1:ip[i + 1]] @ z[ix[dpos[i] + 1:ip[i + 1]]]) / v[dpos[i]]
    return z


def two_level(M, z, rhs):
    """what one cycle of the tests' wrapper returns for the preconditioned vector z = B rhs: identity coarse level, one pre-sweep, omega = 1"""
    return z + (rhs - M @ z)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def _short(k, rank, size):
    return 1 + rank % 5


def _runs():
    """runs of 1 .. 13 small levels, each between separator layers: every residue modulo the six steps of a trip, runs shorter than the pipeline's prologue,
    more than two trips; every run starts after a level with a launch of its own.  reach 2: the first two levels of a run read the separator before it."""
    sizes, q = [SEPARATOR], 0
    for length in range(1, 14):
        for _ in range(length):
            sizes.append(5 + (7 * q) % 44)
            q += 1
        sizes.append(SEPARATOR)
    return layered(sizes, _short, _short, reach=2, seed=1)


RUN_LEVEL_SIZES = (1, 16, 63, 64, 65, 128, 129, 200, 256)


def _level_sizes():
    """levels of 1 .. 256 rows inside one run (65 and more: the second path of a level, one to three further passes of 64 rows), 257 alone, a short run behind"""
    return layered((40,) + RUN_LEVEL_SIZES + (SEPARATOR, 30, 20), lambda k, r, s: 1 + r % 7, lambda k, r, s: 1 + (3 * r) % 7, reach=2, seed=2)


def _work_limit(extra):
    """a layer of 256 rows of 64 + 1 + 63 entries: 32 768 in all, still small; with one entry more it gets a launch of its own"""
    return layered((100, 256, 100), lambda k, r, s: 64 if k == 1 else 3, lambda k, r, s: (63 + (extra if r == 0 else 0)) if k == 1 else 3, reach=1, seed=3)


def _triangles(pf_forward, pf_backward):
    """eight layers of 140 rows.  Rows 0 .. 25 of every layer have the triangle lengths LENS (0: the first / last layer), in other combinations left and right;
    the other rows decide the 90th percentile: 2 to 4 entries on the side that is to get 2 slots, 40 on the side that is to get 4"""
    def side(pf, mult, add):
        return lambda k, r, s: LENS[(mult * r + add) % len(LENS)] if r < 26 else (2 + r % 3 if pf == 2 else 40)
    return layered((140,) * 8, side(pf_forward, 1, 0), side(pf_backward, 5, 3), reach=2, seed=4)


def _percentile(p90):
    """ten layers of 100 rows.  Per direction 100 rows without a triangle (the first / last layer) and 900 with one: 32 -- 800 rows of at most 32 entries, some of
    exactly 32, 100 of 33: the 900th shortest has 32; 33 -- one row more of 33"""
    def length(g):
        return 33 if (g % 9 == 0 or (p90 == 33 and g == 1)) else 32 if g % 9 == 1 else 1 + g % 7
    return layered((100,) * 10, lambda k, r, s: length((k - 1) * 100 + r), lambda k, r, s: length((8 - k) * 100 + r), reach=1, seed=5)


def _reach(reach, size, layers):
    """every triangle length of LENS with the operands 1 / up to `reach` levels back"""
    return layered((size,) * layers, lambda k, r, s: LENS[r % len(LENS)], lambda k, r, s: LENS[(5 * r + 3) % len(LENS)], reach=reach, seed=6)


def _long(levels):
    """more than 64 small levels in one run: the prefetching workgroup is launched"""
    return layered([1 + (11 * q) % 48 for q in range(levels)], lambda k, r, s: 1 + r % 4, lambda k, r, s: 1 + (r + k) % 4, reach=2, seed=7)


def _bidiagonal(n):
    """a_ii and a_i,i-1: n forward levels of one row; no row reads a later one, so the backward sweep is ONE level of n rows"""
    rng = np.random.default_rng(_seed("bidiagonal", n))
    return _finish(n, np.arange(1, n), np.arange(n - 1), rng), np.arange(n)


def _diagonal(n):
    rng = np.random.default_rng(_seed("diagonal", n))
    return sp.diags(rng.uniform(1.0, 2.0, n)).tocsr(), np.zeros(n, dtype=np.int64)


def _dense(n):
    rng = np.random.default_rng(_seed("dense", n))
    i, j = np.nonzero(~np.eye(n, dtype=bool))
    return _finish(n, i, j, rng), np.arange(n)


ILU_WIDTHS = (254, 255, 800, 801, 1200)      # and L, L + 1 with the limit L of the ahead kernel on the device at hand: ilu_row(L) in the GPU tests
ILU_L_MI355X = 365                            # 160 kB / (16 rows * 28 bytes per entry)

BUILDERS = {
    "runs": _runs,
    "level_sizes": _level_sizes,
    "work_limit_in": lambda: _work_limit(0),
    "work_limit_out": lambda: _work_limit(1),
    "triangles_f2_b4": lambda: _triangles(2, 4),
    "triangles_f4_b2": lambda: _triangles(4, 2),
    "percentile_32": lambda: _percentile(32),
    "percentile_33": lambda: _percentile(33),
    "reach_1": lambda: _reach(1, 120, 7),
    "reach_4": lambda: _reach(4, 90, 9),
    "long_70": lambda: _long(70),
    "long_200": lambda: _long(200),
    "bidiagonal_300": lambda: _bidiagonal(300),
    "n_1": lambda: _dense(1),
    "n_2": lambda: _dense(2),
    "diagonal_200": lambda: _diagonal(200),
    "diagonal_300": lambda: _diagonal(300),
}
LAYERED = ("runs", "level_sizes", "work_limit_in", "work_limit_out", "triangles_f2_b4", "triangles_f4_b2", "percentile_32", "percentile_33", "reach_1", "reach_4",
           "long_70", "long_200")
NAMES = tuple(BUILDERS) + tuple("ilu_row_%d" % w for w in ILU_WIDTHS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(M, designed layer of every row or None).  Do not modify what it returns: the tests share it"""
    if name.startswith("ilu_row_"):
        return ilu_row(int(name[8:])), None
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def case_plan(name):
    return plan(case(name)[0])


def rhs_of(M, seed=0):
    return np.random.default_rng(_seed("rhs", M.shape[0], seed)).uniform(-1.0, 1.0, M.shape[0])
