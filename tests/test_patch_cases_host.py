"""The inputs of tests/test_gpu_patch_smoothers.py are worth running, and its reference is good enough -- on the host, no GPU.

  * the patches that are meant to need row exchanges need them, every one of them;
  * the patch matrices are well conditioned (the bound of the device test is a statement about rounding, not about conditioning);
  * the float64 oracle (femus_oracle_ns.VankaSmoother) is within 1e-13 of the same sweep in long double with inverses by the kernels' own rule:
    the device bound of 1e-12 leaves a factor of 10 over this assertion;
  * ILU(0) of the blocks differs from their exact inverse by more than 1e-3, so a kernel that ignored the pattern masks would be seen;
  * no block of the ascending saddle systems takes a shift.

The long double sweeps of the 376 / 511 / 512 list take 4-5 s each (Gauss-Jordan in numpy on long double), so that list runs them in two of its
orders only: ascending, and pressure first, where the oracle (which inverts the patch matrix in the order given) is at its worst, 5e-14; the other
lists and `scattered` run every order."""
import functools

import numpy as np
import pytest

import patch_cases as pc
from oracle import femus_oracle as fo
from oracle import femus_oracle_ns as ns

OMEGA, NSWEEPS = 0.7, 2
SADDLE = [(name, order, "last") for name in pc.SIZE_LISTS for order in pc.ORDERS] + [(name, "ascending", "first") for name in pc.SIZE_LISTS]
CASES = [pytest.param(("saddle",) + c, id="-".join(c[:2]) + ("-pressure_block_first" if c[2] == "first" else "")) for c in SADDLE] + [
    pytest.param(("scattered",), id="scattered")]
LONG_DOUBLE = [c for c in CASES if not (c.values[0][:2] == ("saddle", "edges_512") and c.values[0][2:] not in (("ascending", "last"), ("pressure_first", "last")))]


def build(case):
    if case[0] == "scattered":
        return pc.scattered(0)
    return pc.saddle(pc.SIZE_LISTS[case[1]], 0, case[2], case[3])


def test_the_cases_are_what_they_say():
    for name, sizes in pc.SIZE_LISTS.items():
        for order in pc.ORDERS:
            A, patches = pc.saddle(sizes, 0, order)
            assert [len(d) for d in patches] == list(sizes) and A.shape[0] <= 2000
            assert all(len(set(d.tolist())) == len(d) for d in patches)
            npr = sum(s > 1 for s in sizes)
            assert A.has_sorted_indices and np.all(A.diagonal()[-npr:] == 0.0)
            assert all(A[i, i] == 0.0 and i in A.indices[A.indptr[i]:A.indptr[i + 1]] for i in range(A.shape[0] - npr, A.shape[0]))      # stored zeros
            asc = [np.all(np.diff(d) > 0) for d in patches if len(d) > 2]
            assert all(asc) if order == "ascending" else not any(asc)
            if order == "pressure_first":
                assert all(d[0] >= A.shape[0] - npr for d in patches if len(d) > 1)
        assert all(np.array_equal(np.sort(a), np.sort(b)) for a, b in zip(pc.saddle(sizes, 0, "ascending")[1], pc.saddle(sizes, 0, "shuffled")[1]))
    M, patches = pc.scattered(0)
    count = np.bincount(np.concatenate(patches), minlength=M.shape[0])
    assert (count == 0).sum() >= M.shape[0] // 10 and count.max() >= 3                  # rows no patch covers, rows that three or more share
    assert {len(d) for d in patches} == {1, 2, 5, 20, 40, 70, 100} and len(patches) == 120
    assert (abs(M) - abs(M).T).nnz > 0
    color = ns.color_patches(patches, M)
    assert color.max() + 1 < len(patches)                                               # some colour holds several patches


@pytest.mark.parametrize("name", list(pc.SIZE_LISTS))
def test_row_exchanges_in_every_patch_of_the_pressure_first_numbering(name):
    """fh_mg_set_level_patches sorts every patch, so the order inside a caller's list no longer decides the pivots; numbered [pressure | velocity]
    a sorted patch starts with its zero diagonal and both inversion kernels must exchange rows.  (The other numbering needs none or one.)"""
    A, patches = pc.saddle(pc.SIZE_LISTS[name], 0, "ascending", "first")
    ex = [pc.gauss_jordan_inverse(pc.patch_matrix(A, np.sort(d)))[1] for d in patches]
    print("%s, pressure block first: %d..%d row exchanges per patch of more than one dof" % (name, min(e for e, d in zip(ex, patches) if len(d) > 1), max(ex)))
    assert all(e >= 1 for e, d in zip(ex, patches) if len(d) > 1)
    for d in patches[:6]:                        # the rule inverts
        M = pc.patch_matrix(A, np.sort(d))
        assert abs(pc.gauss_jordan_inverse(M)[0] @ M - np.eye(len(d))).max() < 1e-12


@pytest.mark.parametrize("case", CASES)
def test_patch_matrices_are_well_conditioned(case):
    A, patches = build(case)
    worst = max(np.linalg.cond(pc.patch_matrix(A, d)) for d in patches)
    print("largest 2-norm condition number of a patch matrix: %.1f" % worst)
    assert worst <= 100.0


@functools.lru_cache(maxsize=None)
def oracle_two_level(case):
    A, patches = build(case)
    color = ns.color_patches(patches, A)
    b = fo.lcg_fill(A.shape[0], 7)
    sm = ns.VankaSmoother(A, patches, color, OMEGA)
    z = np.zeros(A.shape[0])
    for _ in range(NSWEEPS):
        z = sm.sweep(b, z)
    return A, patches, color, b, z + (b - A @ z)


@pytest.mark.parametrize("case", LONG_DOUBLE)
def test_float64_oracle_against_long_double(case):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 here: this yardstick needs an extended type")
    A, patches, color, b, ref = oracle_two_level(case)
    inv = [pc.gauss_jordan_inverse(pc.patch_matrix(A, d), np.longdouble)[0] for d in patches]
    exact = pc.vanka_two_level(A, patches, color, inv, b, OMEGA, NSWEEPS, np.longdouble)
    scale = float(np.abs(exact).max())
    e_oracle = float(np.abs(ref - exact).max()) / scale
    inv64 = [pc.gauss_jordan_inverse(pc.patch_matrix(A, d))[0] for d in patches]
    e_rule = float(np.abs(pc.vanka_two_level(A, patches, color, inv64, b, OMEGA, NSWEEPS) - exact).max()) / scale
    print("float64 oracle %.1e, float64 Gauss-Jordan restatement %.1e from the long double sweep" % (e_oracle, e_rule))
    assert e_oracle <= 1e-13 and e_rule <= 1e-13


@pytest.mark.parametrize("name", list(pc.SIZE_LISTS) + ["scattered"])
def test_ilu0_blocks_differ_from_exact_blocks_and_take_no_shift(name):
    A, patches = pc.scattered(0, True) if name == "scattered" else pc.saddle(pc.SIZE_LISTS[name], 0, "ascending")
    ilu, exact = ns.AsmSmoother(A, patches), ns.AsmSmoother(A, patches, n_exact=len(patches))
    b = fo.lcg_fill(A.shape[0], 7)
    y0, y1 = ilu.apply(b), exact.apply(b)
    d = abs(y0 - y1).max() / abs(y1).max()
    print("ILU(0) blocks against exact blocks: %.1e of the largest entry" % d)
    assert d > 1e-3
    assert all(f[2] == 0.0 for f in ilu.ilu)
