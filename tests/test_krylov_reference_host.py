"""The host reference of the outer Krylov solvers (tests/krylov_reference.py) checks itself, without a GPU: every solver is stated by
recurrence (the device's algorithm) and by definition (least squares over the Krylov space, Galerkin projection, closed-form sum), and the two
must agree iterate by iterate.  Their distance sets the tolerance of tests/test_gpu_krylov.py; here the conditions on that tolerance, on the
compared iteration counts and on the stopping cases are asserted, so that the GPU test uses numbers that were checked."""
import numpy as np
import pytest

import krylov_reference as kr

ITERATE_CASES = kr.iterate_cases()
case_id = lambda c: "%s-%s-%d" % c


@pytest.mark.parametrize("case", ITERATE_CASES, ids=case_id)
def test_the_two_forms_agree_iterate_by_iterate(case):
    """x_k to 1e-12 of |x_direct| at every listed k (BIG: k <= 7) -- some thousand roundings, the conditioning of the small least-squares
    problems included -- and the reported norm to 1e-12 of the reference norm: the estimate of GMRES against the true minimum, the recurrence
    residual of CG against b - A x"""
    ic = kr.iterate_case(*case)
    for k in ic.listed:
        rec, dfn = ic.rec[k], ic.dfn[k]
        assert rec.its == k
        assert ic.dist[k] <= 1e-12, (k, ic.dist[k])
        assert abs(rec.rn - dfn.rn) <= 1e-12 * rec.ref, (k, rec.rn, dfn.rn)
        assert rec.ref == pytest.approx(dfn.ref, rel=1e-14)


@pytest.mark.parametrize("name,solver,restart,ks", [("ONE", "gmres", 30, (0, 1)), ("ONE", "fgmres", 30, (0, 1)), ("ONE", "cg", 0, (0, 1)),
                                                    ("ONE", "richardson", 0, (0, 1, 2)), ("D130", "richardson", 0, (0, 1, 2, 3, 4, 5)),
                                                    ("D130", "gmres", 4, (0, 1, 4, 5)), ("D130", "fgmres", 4, (0, 1, 4, 5)),
                                                    ("U130", "gmres", 30, (0,)), ("U130", "fgmres", 30, (0,)), ("S130", "cg", 0, (0,))])
def test_the_two_forms_agree_on_the_other_problems(name, solver, restart, ks):
    """one unknown, the diverging cycle, and k = 0 (the Knoll guess, or zero)"""
    pb = kr.problem(name)
    for k in ks:
        rec, dfn = kr.solve_recurrence(pb, solver, restart, k, **kr.NO_STOP), kr.solve_definition(pb, solver, restart, k)
        scale = max(np.linalg.norm(rec.x), np.linalg.norm(pb.x_direct))
        if name == "ONE" and solver != "richardson" and k == 1:      # the cycle is the exact solve: nothing left to do after the Knoll guess
            assert rec.its <= 1
        else:
            assert rec.its == k
        assert np.linalg.norm(rec.x - dfn.x) <= 1e-12 * scale
        assert abs(rec.rn - dfn.rn) <= 1e-12 * max(rec.ref, rec.rn)


@pytest.mark.parametrize("case", ITERATE_CASES, ids=case_id)
def test_tolerance_separates_consecutive_iterates(case):
    """tol = MARGIN * the largest distance of the two forms over the compared k; at every compared k it is at most 1e-2 of the step to the
    next iterate, so a result one iteration off fails by a factor 100; at most a quarter of the listed k are dropped for that"""
    ic = kr.iterate_case(*case)
    assert ic.tol == kr.MARGIN * max(ic.dist[k] for k in ic.ks)
    assert 0.0 < ic.tol <= 1e-10
    for k in ic.ks:
        assert ic.tol <= kr.STEP_FRACTION * ic.step[k], k
    assert len(ic.dropped) <= len(ic.listed) // 4, ic.dropped
    for k in ic.dropped:                                  # dropped only where the reference itself breaks the condition
        assert ic.tol > kr.STEP_FRACTION * ic.step[k]
    if case[1] in ("gmres", "fgmres") and case[0] != "BIG":
        m = case[2]
        assert m in ic.ks or m == 1 or m > max(ic.listed), "the last column of the first cycle"
        assert any(k % m == 0 for k in ic.ks) and any(k % m == 1 % m and k > m for k in ic.ks)      # end of a cycle, first column of the next


@pytest.mark.parametrize("case", [c for c in ITERATE_CASES if c[0] != "BIG"], ids=case_id)
def test_wrong_algorithms_are_far_outside_the_tolerance(case):
    """what the GPU test must tell apart: a zero guess in place of Knoll's, the scale 1 in place of 0.99999, an iterate one step early"""
    ic = kr.iterate_case(*case)
    pb, (name, solver, restart) = ic.problem, case
    for k in ic.ks:
        if solver in ("gmres", "fgmres"):
            wrong = kr.gmres_recurrence(pb, restart, k, solver == "fgmres", knoll=False).x
        elif solver == "richardson":
            wrong = kr.richardson_recurrence(pb, k, scale=1.0).x
        else:
            wrong = kr.cg_recurrence(pb, k - 1).x
        assert np.linalg.norm(wrong - ic.rec[k].x) / ic.xdn > 100.0 * ic.tol, k


@pytest.mark.parametrize("solver,restart", kr.stop_cases())
def test_stop_thresholds_sit_in_a_gap_of_the_history(solver, restart):
    sc = kr.stop_case(solver, restart)
    i = sc.index - 1
    assert sc.hist[i] >= 1.5 * sc.hist[i + 1] and sc.hist[i] == min(sc.hist[:i + 1])
    assert sc.hist[i + 1] < sc.threshold < sc.hist[i]
    at_index = kr.solve_recurrence(sc.problem, solver, restart, sc.index, **kr.NO_STOP)
    for tol in (dict(rtol=sc.threshold / sc.ref), dict(atol=sc.threshold)):
        res = kr.solve_recurrence(sc.problem, solver, restart, 1000, **tol)
        assert res.its == sc.index and np.array_equal(res.x, at_index.x) and res.rn == at_index.rn


@pytest.mark.parametrize("solver", ["richardson", "gmres", "fgmres"])
def test_the_diverging_cycle_diverges(solver):
    dc = kr.divergence_case(solver)
    pb = dc.problem
    M = np.column_stack([pb.cycle(e) for e in np.eye(pb.n)])
    assert np.abs(np.linalg.eigvals(np.eye(pb.n) - M @ pb.A.toarray())).max() > 2.0          # the cycle as an iteration
    assert all(b2 > a2 for a2, b2 in zip(dc.hist, dc.hist[1:dc.index + 2]))
    lo, hi = (dc.hist[dc.index - 1], dc.hist[dc.index]) if solver == "richardson" else (dc.hist[0], dc.hist[1])
    assert lo * 1.1 < dc.dtol * dc.ref < hi / 1.1
    restart = 0 if solver == "richardson" else 30
    res = kr.solve_recurrence(pb, solver, restart, 12, dtol=dc.dtol)
    assert res.its == dc.index and res.rn > dc.dtol * res.ref and np.isfinite(res.x).all()
    assert kr.solve_recurrence(pb, solver, restart, 12, dtol=1e50).its == 12


def test_problems_are_what_they_are_said_to_be():
    for name, n, nc in (("U130", 130, 9), ("U257", 257, 17), ("S130", 130, 9), ("BIG", 600001, 33)):
        pb = kr.problem(name)
        A, P = pb.A, pb.P
        assert A.shape == (n, n) and P.shape == (n, nc) and np.allclose(np.asarray(P.sum(axis=1)).ravel(), 1.0)
        if name == "S130":
            assert abs(A - A.T).max() == 0.0 and np.linalg.eigvalsh(A.toarray()).min() > 0.0
            Md = np.column_stack([pb.cycle(e) for e in np.eye(n)])
            assert np.abs(Md - Md.T).max() <= 1e-14 * np.abs(Md).max()                        # npre = npost: a symmetric cycle, as CG needs
        else:
            assert abs(A - A.T).max() > 0.5
        if name == "BIG":
            assert n > 8 * 256 * 256 and n % 256 != 0 and A.nnz == 3 * n - 2
        else:
            assert A.nnz > 3 * n - 2
    assert kr.problem("ONE").n == 1
