"""Inputs for the block Schwarz smoothers (femus_amd/csrc/fh_patch.hip) that are no mesh, and a plain restatement of what the kernels compute.
Imported by tests/test_patch_cases_host.py (which shows on a machine without a GPU that the inputs exercise what they are meant to and that
the float64 oracle is good enough a reference) and by tests/test_gpu_patch_smoothers.py (which compares the device with the oracle on them).

  saddle      A = [[K, B], [C, 0]] with one patch per pressure dof: a window of consecutive velocity dofs and that pressure dof, the sizes chosen
              around the limits the kernels branch on (64 register columns, PLDS_MAX = 96, 256 threads, 512 dofs)
  scattered   a row-dominant matrix with an unsymmetric pattern and patches drawn at random: dofs nobody covers, dofs in several patches,
              patches of one dof, sizes that differ widely on one level
  gauss_jordan_inverse, vanka_two_level   the inversion rule and the sweep in numpy, in any dtype (np.longdouble: the yardstick for the float64 oracle)

Nothing here comes from the device."""
import functools

import numpy as np
import scipy.sparse as sp

SIZE_LISTS = {
    "edges_2_98": (1, 2, 3, 17, 33, 63, 64, 65, 66, 95, 96, 97, 98),       # both sides of 64 and of PLDS_MAX; one row per lane and two
    "edges_256": (130, 255, 256, 257, 258),                               # one and two strides of 256 threads
    "edges_512": (376, 511, 512),                                         # the largest HEX27 patch and the limit
    "shipped_51": (51,) * 40,                                             # the interior patch of the QUAD9 cavity, many per colour
}
ORDERS = ("ascending", "pressure_first", "shuffled")


def _seed(*words):
    """a seed that does not depend on the hash randomisation of the interpreter"""
    s = 0
    for w in words:
        for ch in str(w):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=None)
def saddle(sizes, seed=0, order="ascending", pressure_block="last"):
    """(A, patches).  K: band of half-width 3, about 70 % filled, unsymmetric values in (-1, 1), diagonal = sum of the |off-diagonal| of the row + U(1, 2).
    Patch j: a window of sizes[j] - 1 consecutive velocity dofs and pressure dof j; neighbouring windows overlap by min(3, w // 2) dofs (w: the smaller
    of the two).  Column j of B and row j of C lie on window j, independent values in (0.5, 1.5); the pressure diagonal is stored as explicit zeros.
    A patch of size 1 is one velocity dof alone (a pressure dof alone would be the 1 x 1 zero matrix) and has no pressure dof.
    order: the dofs inside a patch ascending in the numbering [velocity | pressure], the pressure dof first, or shuffled.
    pressure_block "first": the same system numbered [pressure | velocity], A = [[0, C], [B, K]] -- a sorted patch then starts with its zero diagonal."""
    sizes = tuple(int(s) for s in sizes)
    assert order in ORDERS and pressure_block in ("last", "first") and min(sizes) >= 1 and max(sizes) <= 512
    rng = np.random.default_rng(_seed("saddle", sizes, seed))
    widths = [max(s - 1, 1) for s in sizes]
    start, s0 = [], 0
    for j, w in enumerate(widths):
        if j > 0:
            s0 = s0 + widths[j - 1] - min(3, widths[j - 1] // 2, w // 2)
        start.append(s0)
    nv = start[-1] + widths[-1]
    has_p = [s > 1 for s in sizes]
    pidx = np.cumsum(has_p) - 1                   # pressure dof of patch j (where it has one)
    npr = int(sum(has_p))
    K = sp.lil_matrix((nv, nv))
    for i in range(nv):
        for j in range(max(0, i - 3), min(nv, i + 4)):
            if j != i and rng.uniform() < 0.7:
                K[i, j] = rng.uniform(-1.0, 1.0)
    K = K.tocsr()
    K = K + sp.diags(np.asarray(abs(K).sum(axis=1)).ravel() + rng.uniform(1.0, 2.0, nv))
    rows, cols, bv, cv = [], [], [], []
    for j, (s, w) in enumerate(zip(start, widths)):
        if has_p[j]:
            rows += list(range(s, s + w))
            cols += [int(pidx[j])] * w
            bv += list(rng.uniform(0.5, 1.5, w))
            cv += list(rng.uniform(0.5, 1.5, w))
    B = sp.coo_matrix((bv, (rows, cols)), shape=(nv, npr))
    C = sp.coo_matrix((cv, (cols, rows)), shape=(npr, nv))
    A =(sp.bmat([[K, B], [C, None]]) if pressure_block == "last" else sp.bmat([[None, C], [B, K]])).tocsr()
    # the zero block goes in by pattern, not by arithmetic (a sum of scipy matrices may drop stored zeros)
    voff, poff = (0, nv) if pressure_block == "last" else (npr, 0)
    A = _with_stored_zeros(A, poff + np.arange(npr))
    assert np.all(A.diagonal()[poff:poff + npr] == 0.0) and A[poff:poff + npr][:, poff:poff + npr].nnz == npr
    patches = []
    for j, (s, w) in enumerate(zip(start, widths)):
        v = voff + np.arange(s, s + w)
        p = np.array([poff + pidx[j]] if has_p[j] else [], dtype=np.int64)
        if order == "ascending":
            d = np.sort(np.concatenate([v, p]))
        elif order == "pressure_first":
            d = np.concatenate([p, v])
        else:
            d = rng.permutation(np.concatenate([v, p]))
        patches.append(d.astype(np.int64))
        assert d.size == sizes[j]
    return A, patches


def _with_stored_zeros(A, diag_rows):
    """A with an explicitly stored (zero) diagonal entry in the given rows, which have none"""
    A = A.tocoo()
    r = np.concatenate([A.row, diag_rows])
    c = np.concatenate([A.col, diag_rows])
    v = np.concatenate([A.data, np.zeros(len(diag_rows))])
    o = np.lexsort((c, r))
    r, c, v = r[o], c[o], v[o]
    n = A.shape[0]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
    return sp.csr_matrix((v, c.astype(np.int32), indptr.astype(np.int32)), shape=A.shape)


@functools.lru_cache(maxsize=None)
def scattered(seed=0, sort_patches=False):
    """(M, patches): a random row-dominant matrix with an unsymmetric pattern (built like the matrix of
    test_multicolour_sweep_on_an_unsymmetric_pattern_is_race_free) and 120 patches of 1, 2, 5, 20, 40, 70 or 100 dofs, each a random choice without
    repeats from 90 % of the rows, in the order drawn: some rows are in no patch, some in several"""
    rng = np.random.default_rng(_seed("scattered", seed))
    n = 1500
    S = sp.random(n, n, density=0.006, random_state=np.random.RandomState(7 + seed), format="csr", data_rvs=lambda k: rng.uniform(-1, 1, k)).tolil()
    S.setdiag(0.0)
    S = S.tocsr()
    S.eliminate_zeros()
    M = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + 1.0)).tocsr()
    M.sort_indices()
    assert (abs(M) - abs(M).T).nnz > 0
    pool = rng.permutation(n)[:(9 * n) // 10]
    sizes = rng.choice([1, 2, 5, 20, 40, 70, 100], size=120)
    patches = [rng.choice(pool, size=int(s), replace=False).astype(np.int64) for s in sizes]
    if sort_patches:
        patches = [np.sort(d) for d in patches]
    return M, patches


def patch_matrix(A, d):
    return A[d][:, d].toarray()


def gauss_jordan_inverse(M, dtype=np.float64):
    """(inverse, number of row exchanges) by the rule of k_patch_invert and k_patch_invert_lds: in-place Gauss-Jordan, pivot = the largest |a_ik|,
    i >= k, the smallest row on ties; the pivot row scaled by 1 / pivot, the other rows a_ij -= a_ik a_kj with the column of the pivot replaced
    by -a_ik / pivot; the row interchanges undone as column interchanges, last first.  A pivot that is not > 0 raises."""
    A = np.array(M, dtype=dtype)
    n = A.shape[0]
    piv = np.zeros(n, dtype=np.int64)
    for k in range(n):
        col = np.abs(A[k:, k])
        pr = k + int(np.argmax(col))              # the first of the largest
        if not col[pr - k] > 0:
            raise ZeroDivisionError("singular at step %d" % k)
        piv[k] = pr
        if pr != k:
            A[[k, pr]] = A[[pr, k]]
        pv = 1 / A[k, k]
        f = A[:, k].copy()
        f[k] = 0
        rowk = A[k] * pv
        rowk[k] = pv
        A[k] = rowk
        A -= np.outer(f, rowk)
        A[:, k] = -f * pv
        A[k, k] = pv
    for k in range(n - 1, -1, -1):
        if piv[k] != k:
            A[:, [k, piv[k]]] = A[:, [piv[k], k]]
    return A, int(np.sum(piv != np.arange(n)))


def vanka_two_level(A, patches, color, inverses, b, omega, nsweeps, dtype=np.float64):
    """z + (b - A z), z = nsweeps multiplicative sweeps from zero, x_p += omega inv_p (b - A x)_p over the colours in sequence: what the two-level
    wrapper with an identity coarse level computes.  All of it in `dtype` (A as a dense array: scipy has no long double)."""
    Ad = np.asarray(A.toarray(), dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    x = np.zeros(b.size, dtype=dtype)
    om = dtype(omega)
    rows = [Ad[d] for d in patches]
    for _ in range(nsweeps):
        for c in range(int(np.max(color)) + 1):
            for p in np.where(np.asarray(color) == c)[0]:
                d = patches[p]
                x[d] += om * (np.asarray(inverses[p], dtype=dtype) @ (b[d] - rows[p] @ x))
    return x + (b - Ad @ x)
