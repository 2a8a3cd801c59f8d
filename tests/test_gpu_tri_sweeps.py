"""GPU: the natural-order sweeps (femus_amd/csrc/fh_trisolve.hip: PCSOR's symmetric sweep, the ILU(0) factorisation and solve) on matrices with a
DESIGNED level schedule (tests/tri_cases.py; tests/test_tri_cases_host.py shows without a GPU that each case is what it claims), against the
float64 oracle's sequential sweeps.

Every test asserts through fh_mg_sweep_info that its case took the path it was built for: the levels, the runs of small levels and their
lengths, the register slots of the run kernel, the kernel of the factorisation.  A test that cannot say which kernel ran does not test it.

Wrapper, as in test_gpu_multigrid.py: level 0 the identity, level 1 the case with one pre-sweep and omega = 1, so that one cycle returns
x = z + (b - A z) with z = B b.  Compared per component, relative to the largest component of the reference -- one wrong row among thousands must
not average out -- at 1e-12, the bound test_natural_order_sweeps_on_unstructured_patterns uses for these sweeps; the float64 oracle itself is
within 4e-16 of the same sweeps in long double on these cases (test_tri_cases_host.py).  Largest errors seen: DESIGN.md."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from femus_amd import capi
from oracle import femus_oracle as fo
import tri_cases as tc

pytestmark = pytest.mark.gpu
SMOOTHERS = {"sor": capi.SMOOTH_SOR, "ilu0": capi.SMOOTH_ILU0}
BOUND = 1e-12
KINDS = ("sor", "ilu0")


def device(ctx, M, kind):
    n = M.shape[0]
    eye = sp.identity(n, format="csr")
    mats = [ctx.matrix_scipy(eye), ctx.matrix_scipy(M), ctx.matrix_scipy(eye)]
    mg = capi.Multigrid(ctx, 2)
    mg.set_level(0, mats[0], None, None, 0, 1.0, 1, 0)
    mg.set_level(1, mats[1], mats[2], None, SMOOTHERS[kind], 1.0, 1, 0)
    mg.setup()
    return mg, mats


def cycle(ctx, mg, rhs):
    b, x = ctx.vector_from(rhs), ctx.vector(rhs.size)
    mg.vcycle(b, x)
    first = x.to_numpy().copy()
    mg.vcycle(b, x)                                 # the replay of the captured graph
    return first, x.to_numpy().copy()


def oracle(M, kind, rhs):
    """x = z + (rhs - M z) with the float64 oracle's z = B rhs; the wrapper's residual in long double, so that the reference carries the oracle's error only"""
    if kind == "sor":
        z = fo.sor_symmetric_natural(M, 1.0 / M.diagonal(), rhs)
    else:
        LU = fo.ilu0_factor(M)
        assert LU[2] == 0.0
        z = fo.ilu0_apply(LU, rhs)
    return tc.two_level(M.astype(np.longdouble), z.astype(np.longdouble), rhs.astype(np.longdouble))


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    M, _ = tc.case(name)
    return oracle(M, kind, tc.rhs_of(M))


def worst_component(got, ref):
    return float(np.abs(got.astype(np.longdouble) - ref).max() / np.abs(ref).max())


def lds_bytes(kernel, max_row):
    return 16 * max_row * {"plan": 28, "ahead": 28, "lds_columns": 12, "plain": 8}[kernel]


def assert_path(mg, M, kind, plan, ilu_ahead=2):
    """the library planned the sweeps as the restated rules plan them, and factored with the kernel the rule names; returns that kernel"""
    info = mg.sweep_info(1)
    for d in ("forward", "backward"):
        assert info[d] == plan[d]["info"], (d, info[d], plan[d]["info"])
    if kind == "sor":
        assert info["ilu"]["kernel"] is None
        return None
    max_row = int(np.diff(M.indptr).max())
    kernel = tc.ilu_kernel(max_row, info["ilu"]["row_limit"], ilu_ahead)
    assert info["ilu"]["kernel"] == kernel and info["ilu"]["lds_bytes"] == lds_bytes(kernel, max_row) and info["ilu"]["shift"] == 0.0, info["ilu"]
    return kernel


@pytest.fixture(scope="module")
def row_limit(ctx):
    """the longest row each factorisation kernel is granted on this device"""
    mg, mats = device(ctx, tc.case("n_2")[0], "ilu0")
    limit = mg.sweep_info(1)["ilu"]["row_limit"]
    mg.destroy()
    assert limit["plan"] == 254 and 255 <= limit["ahead"] < 800
    return limit


def ilu_row_cases(row_limit):
    """case name -> the kernel it is built for: each side of 254 / 255, of the ahead kernel's limit L / L + 1 and of 800 / 801, and the longest row served"""
    L = row_limit["ahead"]
    return {"ilu_row_254": "plan", "ilu_row_255": "ahead", "ilu_row_%d" % L: "ahead", "ilu_row_%d" % (L + 1): "lds_columns", "ilu_row_800": "lds_columns",
            "ilu_row_801": "plain", "ilu_row_1200": "plain"}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", tc.NAMES)
def test_designed_schedules_against_the_oracle(ctx, name, kind):
    """the planned path is the designed one; one cycle against the oracle per component; the replayed graph gives the same bits; with tri_runs = 0 (a launch per
    level, sums by wave shuffles) the plan has no run and the bits are the same"""
    M, _ = tc.case(name)
    rhs, ref = tc.rhs_of(M), reference(name, kind)
    out = []
    for runs in (1, 0):
        ctx.set_option("tri_runs", runs)
        try:
            mg, mats = device(ctx, M, kind)
            kernel = assert_path(mg, M, kind, tc.case_plan(name) if runs else tc.plan(M, tri_runs=False))
            assert runs or (mg.sweep_info(1)["forward"]["runs"], mg.sweep_info(1)["backward"]["runs"]) == (0, 0)
            first, replay = cycle(ctx, mg, rhs)
            mg.destroy()
        finally:
            ctx.set_option("tri_runs", 1)
        assert np.array_equal(first, replay)
        out.append(first)
    err = worst_component(out[0], ref)
    print("%s %s%s: worst component against the oracle %.2e" % (name, kind, " (%s)" % kernel if kernel else "", err))
    assert np.isfinite(out[0]).all() and err < BOUND
    assert np.array_equal(out[0], out[1])
    if not name.startswith("ilu_row_"):
        assert kernel in (None, "plan")


@pytest.mark.parametrize("which", ["254", "255", "L", "L+1", "800", "801", "1200"])
def test_rows_at_the_limits_of_the_factorisation_kernels(ctx, row_limit, which):
    """each side of 254 / 255, L / L + 1 and 800 / 801 and the longest row served, 1 200: the kernel the case is built for factored it (three of them with more than
    the 64 kB of LDS a kernel gets without asking), the solve agrees with the oracle, and ilu_ahead = 2, 1, 0 give the same bits where they choose other kernels"""
    L = row_limit["ahead"]
    assert row_limit == {"plan": 254, "ahead": L, "lds_columns": 800, "plain": 1200}
    for name, built_for in ilu_row_cases(row_limit).items():
        if name != "ilu_row_%d" % (L if which == "L" else L + 1 if which == "L+1" else int(which)):
            continue
        M, _ = tc.case(name)
        max_row = int(name[8:])
        assert int(np.diff(M.indptr).max()) == max_row
        rhs, ref = tc.rhs_of(M), reference(name, "ilu0")
        out, kernels = [], []
        for ahead in (2, 1, 0):
            ctx.set_option("ilu_ahead", ahead)
            try:
                mg, mats = device(ctx, M, "ilu0")
                kernels.append(assert_path(mg, M, "ilu0", tc.case_plan(name), ahead))
                out.append(cycle(ctx, mg, rhs)[0])
                mg.destroy()
            finally:
                ctx.set_option("ilu_ahead", 2)
        assert kernels[0] == built_for, (name, kernels)
        assert kernels[2] == ("lds_columns" if max_row <= 800 else "plain") and kernels[1] == ("ahead" if max_row <= L else kernels[2])
        if max_row in (L, 800, 1200):
            assert lds_bytes(built_for, max_row) > 64 * 1024
        err = worst_component(out[0], ref)
        print("%s ilu0 %s: worst component against the oracle %.2e" % (name, kernels, err))
        assert err < BOUND
        assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


def test_a_row_of_1201_entries_is_refused(ctx):
    M, _ = tc.case("ilu_row_1201")
    eye = sp.identity(M.shape[0], format="csr")
    mats = [ctx.matrix_scipy(eye), ctx.matrix_scipy(M), ctx.matrix_scipy(eye)]
    mg = capi.Multigrid(ctx, 2)
    mg.set_level(0, mats[0], None, None, 0, 1.0, 1, 0)
    mg.set_level(1, mats[1], mats[2], None, capi.SMOOTH_ILU0, 1.0, 1, 0)
    with pytest.raises(capi.FemusHipError, match="1201 entries.*at most 1200"):
        mg.setup()
    mg.destroy()
    mg, mats = device(ctx, M, "sor")               # the limit is the factorisation's: the symmetric sweep serves the row
    first, replay = cycle(ctx, mg, tc.rhs_of(M))
    mg.destroy()
    assert np.array_equal(first, replay) and worst_component(first, reference("ilu_row_1201", "sor")) < BOUND


@pytest.mark.parametrize("name", [n for n in tc.NAMES if not n.startswith("ilu_row_")])
def test_factorisation_kernels_give_the_same_bits(ctx, name):
    """rows of at most 254 entries: k_ilu_factor_plan (ilu_ahead = 2), k_ilu_factor_ahead (1) and k_ilu_factor<true> (0) factor every designed case to the same bits"""
    M, _ = tc.case(name)
    rhs = tc.rhs_of(M)
    out, kernels = [], []
    for ahead in (2, 1, 0):
        ctx.set_option("ilu_ahead", ahead)
        try:
            mg, mats = device(ctx, M, "ilu0")
            kernels.append(assert_path(mg, M, "ilu0", tc.case_plan(name), ahead))
            out.append(cycle(ctx, mg, rhs)[0])
            mg.destroy()
        finally:
            ctx.set_option("ilu_ahead", 2)
    assert kernels == ["plan", "ahead", "lds_columns"]
    assert worst_component(out[0], reference(name, "ilu0")) < BOUND
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


@pytest.mark.parametrize("name,kind", [("runs", "sor"), ("triangles_f2_b4", "sor"), ("runs", "ilu0"), ("triangles_f2_b4", "ilu0"), ("ilu_row_254", "ilu0"),
                                       ("ilu_row_L", "ilu0"), ("ilu_row_800", "ilu0"), ("ilu_row_1200", "ilu0")])
def test_new_values_in_the_operator_reach_the_sweeps(ctx, row_limit, name, kind):
    """new values written into the operator and setup() again: the cycle follows the new values, through the plan (and the elimination plan) of the pattern --
    the info call shows the same path and the same kernel, one case per factorisation kernel"""
    if name == "ilu_row_L":
        name = "ilu_row_%d" % row_limit["ahead"]
    M, _ = tc.case(name)
    M2 = tc.revalued(M)
    assert np.array_equal(M.indices, M2.indices) and np.array_equal(M.indptr, M2.indptr) and not np.any(M.data == M2.data)
    rhs = tc.rhs_of(M)
    mg, mats = device(ctx, M, kind)
    kernel = assert_path(mg, M, kind, tc.case_plan(name))
    before = mg.sweep_info(1)
    first, _ = cycle(ctx, mg, rhs)
    assert worst_component(first, reference(name, kind)) < BOUND
    mats[1].set_values(M2.data)
    mg.setup()
    assert mg.sweep_info(1) == before and assert_path(mg, M2, kind, tc.case_plan(name)) == kernel
    second, replay = cycle(ctx, mg, rhs)
    mg.destroy()
    ref2 = oracle(M2, kind, rhs)
    assert worst_component(first, ref2) > 1e-3                      # the two operators are far apart
    assert worst_component(second, ref2) < BOUND and np.array_equal(second, replay)
    if kind == "ilu0" and name.startswith("ilu_row_"):
        assert kernel == ilu_row_cases(row_limit)[name]


def test_the_shift_of_a_restarted_factorisation_is_reported(ctx):
    """a pivot that cancels exactly (u_11 = 1 - 1 * 1 / 1) restarts the factorisation of A + shift I: the info call names the shift the oracle takes"""
    n = 40
    M = sp.lil_matrix((n, n))
    for i in range(n):
        M[i, i] = 2.0
        if i + 1 < n:
            M[i, i + 1] = M[i + 1, i] = -1.0
    M[0, 0], M[0, 1], M[1, 0], M[1, 1] = 1.0, 1.0, 1.0, 1.0
    M = M.tocsr()
    shift = fo.ilu0_factor(M)[2]
    assert shift > 0.0
    mg, mats = device(ctx, M, "ilu0")
    info = mg.sweep_info(1)
    mg.destroy()
    assert info["ilu"]["shift"] == shift and info["ilu"]["kernel"] == "plan"
    assert info["forward"] == tc.plan(M)["forward"]["info"] and info["forward"]["longest_run"] == n
