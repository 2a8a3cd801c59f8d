"""The inputs of tests/test_gpu_tri_sweeps.py are what they claim to be, and the float64 oracle is a good enough reference on them (no GPU).

Every case of tests/tri_cases.py is built for one path of the natural-order sweeps (femus_amd/csrc/fh_trisolve.hip).  Here the library's planning rules,
restated in tri_cases, are applied to each case and compared with the design: the level of every row, the runs and their lengths, the levels with a launch of
their own, the register slots, where the operands come from.  The GPU tests then assert that the library reports the same plan (fh_mg_sweep_info).

Distance of the float64 oracle from the same sweeps in long double, largest over all cases: see DESIGN.md; asserted at 1e-14."""
import numpy as np
import pytest

import tri_cases as tc
from oracle import femus_oracle as fo

ILU_EXTRA = tuple("ilu_row_%d" % w for w in (tc.ILU_L_MI355X, tc.ILU_L_MI355X + 1, 1201))
ALL = tc.NAMES + ILU_EXTRA


@pytest.mark.parametrize("name", tc.LAYERED)
def test_the_level_of_a_row_is_its_layer(name):
    M, layer = tc.case(name)
    P = tc.case_plan(name)
    assert np.array_equal(P["forward"]["level"], layer)
    assert np.array_equal(P["backward"]["level"], layer.max() - layer)
    assert (abs(M) - abs(M).T).nnz > 0                                    # the pattern is unsymmetric
    d = M.diagonal()
    assert np.allclose(d, np.asarray(abs(M).sum(axis=1)).ravel() - d + 1.0)


def _runs(P, direction):
    return P[direction]["run_lengths"], P[direction]["alone"]


def test_runs_of_every_length_between_separators():
    M, layer = tc.case("runs")
    P = tc.case_plan("runs")
    assert _runs(P, "forward") == (list(range(1, 14)), [tc.SEPARATOR] * 14)
    assert _runs(P, "backward") == (list(range(13, 0, -1)), [tc.SEPARATOR] * 14)
    assert {n % 6 for n in P["forward"]["run_lengths"]} == set(range(6)) and max(P["forward"]["run_lengths"]) > 12
    for d in ("forward", "backward"):
        assert min(P[d]["run_starts"]) > 0                                # every run starts after a level of another launch
        assert P[d]["sources"][("registers", "lds")] > 0 and P[d]["sources"][("registers", "global")] > 0
    # the first two levels of every forward run of two or more read the separator before the run
    lev = P["forward"]["level"]
    C = M.tocoo()
    for l0, n in zip(P["forward"]["run_starts"], P["forward"]["run_lengths"]):
        for l in range(l0, l0 + min(n, 2)):
            assert np.any((lev[C.row] == l) & (lev[C.col] == l0 - 1) & (C.col < C.row)), (l0, l)
    assert np.diff(M.indptr).max() <= 11                 # short rows: the host oracle stays quick
    assert M.shape[0] < 11463


def test_level_sizes_inside_a_run():
    P = tc.case_plan("level_sizes")
    for d in ("forward", "backward"):
        assert P[d]["alone"] == [tc.SEPARATOR]
        assert P[d]["info"]["largest_level_in_run"] == 256
        assert P[d]["sources"][("second", "lds")] > 0 and P[d]["sources"][("second", "global")] > 0
    assert P["forward"]["run_lengths"] == [10, 2] and P["backward"]["run_lengths"] == [2, 10]
    assert tuple(P["forward"]["sizes"][1:10]) == tc.RUN_LEVEL_SIZES


@pytest.mark.parametrize("name,work", [("work_limit_in", tc.TRI_SMALL_WORK), ("work_limit_out", tc.TRI_SMALL_WORK + 1)])
def test_the_work_limit_is_met_exactly_and_passed_by_one(name, work):
    M, layer = tc.case(name)
    P = tc.case_plan(name)
    assert int(np.diff(M.indptr)[layer == 1].sum()) == work and int((layer == 1).sum()) == tc.TRI_SMALL
    for d in ("forward", "backward"):
        assert _runs(P, d) == (([3], []) if name == "work_limit_in" else ([1, 1], [256]))


@pytest.mark.parametrize("name,pf,pb", [("triangles_f2_b4", 2, 4), ("triangles_f4_b2", 4, 2)])
def test_triangle_lengths_round_the_register_slots(name, pf, pb):
    P = tc.case_plan(name)
    assert (P["forward"]["info"]["slots"], P["backward"]["info"]["slots"]) == (pf, pb)
    for d in ("forward", "backward"):
        assert P[d]["run_lengths"] == [8]
        assert set(tc.LENS) <= set(P[d]["lengths"])                       # among the rows that go through the registers
        assert all(P[d]["sources"][(p, s)] > 0 for p in ("registers", "second") for s in ("lds", "global"))
        # the tail loop takes a row's highest columns: the layer just before in the forward sweep (LDS), the farthest layer in the backward sweep (global
        # memory); with 2 slots it starts early enough for both.  The backward tail from LDS: case reach_1
        S = P[d]["sources"]
        assert S[("tail", "lds" if d == "forward" else "global")] > 0 and (P[d]["info"]["slots"] == 4 or min(S[("tail", "lds")], S[("tail", "global")]) > 0)


@pytest.mark.parametrize("p90", [32, 33])
def test_the_percentile_that_chooses_the_slots(p90):
    M, _ = tc.case("percentile_%d" % p90)
    P = tc.case_plan("percentile_%d" % p90)
    for d, lengths in zip(("forward", "backward"), tc.triangle_lengths(M)):
        assert P[d]["p90"] == p90 and P[d]["info"]["slots"] == (2 if p90 == 32 else 4)
        assert lengths.size == 1000 and int((lengths <= 32).sum()) == (900 if p90 == 32 else 899) and int((lengths == 32).sum()) >= 90 and lengths.max() == 33


def test_operand_distance():
    near, far = tc.case_plan("reach_1"), tc.case_plan("reach_4")
    for d in ("forward", "backward"):
        for p in ("registers", "tail", "second"):
            assert near[d]["sources"][(p, "global")] == 0 and near[d]["sources"][(p, "lds")] > 0        # all from the level just before
            assert far[d]["sources"][(p, "global")] > 0 and far[d]["sources"][(p, "lds")] > 0
        assert set(tc.LENS[:-1]) <= set(far[d]["lengths"]) and set(tc.LENS) <= set(near[d]["lengths"])
        assert near[d]["run_lengths"] == [7] and far[d]["run_lengths"] == [9]


def test_long_runs_and_tiny_matrices():
    for n in (70, 200):
        P = tc.case_plan("long_%d" % n)
        for d in ("forward", "backward"):
            assert _runs(P, d) == ([n], []) and P[d]["info"]["largest_level_in_run"] <= 48
    P = tc.case_plan("bidiagonal_300")
    assert _runs(P, "forward") == ([300], []) and P["forward"]["info"]["largest_level_in_run"] == 1 and _runs(P, "backward") == ([], [300])
    for name, runs, alone in (("n_1", [1], []), ("n_2", [2], []), ("diagonal_200", [1], []), ("diagonal_300", [], [300])):
        P = tc.case_plan(name)
        for d in ("forward", "backward"):
            assert _runs(P, d) == (runs, alone), name
    assert tc.case_plan("diagonal_200")["forward"]["lengths"] == [0]


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith("ilu_row_")])
def test_one_row_of_exactly_the_width(name):
    M, _ = tc.case(name)
    w = int(name[8:])
    lengths = np.diff(M.indptr)
    low, up = tc.triangle_lengths(M)
    assert lengths.max() == w and int((lengths > 8).sum()) == 1 and low[700] == (w - 1) // 2 and low[700] >= 126
    P = tc.case_plan(name)
    for d in ("forward", "backward"):
        assert _runs(P, d) == ([M.shape[0]], [])                          # one row per level, one run: the wide row goes through the tail loop
        # the tail loop of the wide row: its one operand of the level just before (column 699) is the LAST lower entry; the first upper one sits in a register
        assert P[d]["sources"][("tail", "lds")] == (1 if d == "forward" else 0) and P[d]["sources"][("tail", "global")] > 90


def test_the_kernel_rule_on_the_limits_of_an_mi355x():
    limit = {"plan": 254, "ahead": tc.ILU_L_MI355X, "lds_columns": 800, "plain": 1200}
    expect = {254: ("plan", "ahead", "lds_columns"), 255: ("ahead", "ahead", "lds_columns"), 365: ("ahead", "ahead", "lds_columns"),
              366: ("lds_columns",) * 3, 800: ("lds_columns",) * 3, 801: ("plain",) * 3, 1200: ("plain",) * 3}
    for w, kernels in expect.items():
        assert tuple(tc.ilu_kernel(w, limit, a) for a in (2, 1, 0)) == kernels


@pytest.mark.parametrize("name", ALL)
def test_float64_oracle_against_long_double(name):
    """the oracle's preconditioned vector z = B rhs, which the device is compared with, against the same sweeps as sequential loops in long double: 1e-14 in
    the relative 2-norm and per component relative to the largest; ILU(0) needs no shift"""
    M, _ = tc.case(name)
    rhs = tc.rhs_of(M)
    z = fo.sor_symmetric_natural(M, 1.0 / M.diagonal(), rhs)
    LU = fo.ilu0_factor(M)
    assert LU[2] == 0.0
    y = fo.ilu0_apply(LU, rhs)
    for kind, got, ref in (("sor", z, tc.sor_symmetric_ld(M, rhs)), ("ilu0", y, tc.ilu0_apply_ld(M, tc.ilu0_factor_ld(M), rhs))):
        got = got.astype(np.longdouble)
        norm2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        worst = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("%s %s: oracle against long double %.1e (2-norm), %.1e (worst component)" % (name, kind, norm2, worst))
        assert norm2 < 1e-14 and worst < 1e-14
