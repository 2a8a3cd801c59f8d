"""The sparse products (femus_amd/csrc/fh_spgemm.hip: fh_mat_ptap, fh_mat_abc, fh_mat_matmul) on the designed operands of tests/spgemm_cases.py.
Every test asserts through fh_mat_product_info that its case took the path it was built for -- numeric kernel, gl_log2, map sizes, device or host pattern,
lanes_over_b, for the inner and for the outer product -- compares the pattern with the structural one exactly, and holds the values to the componentwise
bound of the long-double restatement:  |C - ref| <= (K + 2) 2^-52 |A||B|  for one product,  (K_R + K_A + 4) 2^-52 |R||A||P|  for the triple product.

Bit equalities, where the code promises them: a pattern built on the device and one built on the host carry the same arrays and values; a numeric rerun,
and one after C was overwritten with NaN, give the same bits; the slots and the searching kernel give the same bits (both add a * b to a zero accumulator
in increasing k).  The product lists sum in another order and get the bound only.

tests/test_spgemm_cases_host.py shows without a GPU that the cases have the structure they claim."""
import numpy as np
import pytest

import spgemm_cases as sc

pytestmark = pytest.mark.gpu

DEFAULTS = {"spgemm_slot_map": 1, "spgemm_device_symbolic": 1}


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def restore(ctx):
    for name, value in DEFAULTS.items():
        ctx.set_option(name, value)


def destroy(*mats):
    for M in mats:
        if M is not None:
            M.destroy()


def assert_pattern(Md, ref):
    rp, col = Md.pattern()
    assert (Md.m_, Md.n_) == ref.shape
    assert np.array_equal(rp, ref.indptr) and np.array_equal(col, ref.indices)          # structural: the entries that cancel to zero included


def assert_values(what, Md, ref, k):
    v = Md.values()
    r = sc.ratio(v, ref, k)
    print("%s: error / bound %.3g" % (what, r))
    assert np.all(np.isfinite(v)) and r <= 1.0
    return v


def k_triple(R, A):
    return sc.longest_row(R) + sc.longest_row(A) + 4


@pytest.mark.parametrize("name", sc.NAMES)
def test_abc_path_pattern_values_and_state(ctx, name):
    """D = R A P with an explicit R: the path, the pattern, the values; reruns to the same bits, also over a D full of NaN; new values of A, then of P
    (and of R with it where R is the transpose of P) are followed on the same plan; the first values give the first bits again"""
    from femus_amd import capi
    c = sc.case(name)
    R, A, P, AP, D = sc.reference(name)
    Rd, Ad, Pd, Dd = ctx.matrix_scipy(R), ctx.matrix_scipy(A), ctx.matrix_scipy(P), None
    try:
        Dd = capi.Mat.abc(Rd, Ad, Pd)
        info = Dd.product_info()
        assert info == c.paths()
        assert_pattern(Dd, D)
        first = assert_values(name + " abc", Dd, D, k_triple(R, A))
        Dd.abc_numeric(Rd, Ad, Pd)
        assert np.array_equal(bits(Dd.values()), bits(first))
        Dd.set_values(np.full(Dd.nnz, np.nan))
        Dd.abc_numeric(Rd, Ad, Pd)
        assert np.array_equal(bits(Dd.values()), bits(first))
        R2, A2, P2, _, D2 = sc.reference(name, new_a=1)
        Ad.set_values(A2.data)
        Dd.abc_numeric(Rd, Ad, Pd)
        assert_values(name + " abc, new A", Dd, D2, k_triple(R2, A2))
        R3, A3, P3, _, D3 = sc.reference(name, new_a=1, new_p=2)
        Pd.set_values(P3.data)
        Rd.set_values(R3.data)
        Dd.abc_numeric(Rd, Ad, Pd)
        assert_values(name + " abc, new A and P", Dd, D3, k_triple(R3, A3))
        assert Dd.product_info() == info
        assert_pattern(Dd, D)
        Ad.set_values(A.data)
        Pd.set_values(P.data)
        Rd.set_values(R.data)
        Dd.abc_numeric(Rd, Ad, Pd)
        assert np.array_equal(bits(Dd.values()), bits(first))
    finally:
        destroy(Dd, Rd, Ad, Pd)
        restore(ctx)


@pytest.mark.parametrize("name", sc.PTAP_NAMES)
def test_ptap_path_pattern_values_and_state(ctx, name):
    """C = P^T A P: as above; after new values of P the transpose the product keeps must follow by itself"""
    from femus_amd import capi
    c = sc.case(name)
    R, A, P, AP, D = sc.reference(name)
    Ad, Pd, Dd = ctx.matrix_scipy(A), ctx.matrix_scipy(P), None
    try:
        Dd = capi.Mat.ptap(Pd, Ad)
        info = Dd.product_info()
        assert info == c.paths()
        assert_pattern(Dd, D)
        first = assert_values(name + " ptap", Dd, D, k_triple(R, A))
        R2, A2, P2, _, D2 = sc.reference(name, new_p=2)
        Pd.set_values(P2.data)
        Dd.ptap_numeric(Pd, Ad)
        assert_values(name + " ptap, new P", Dd, D2, k_triple(R2, A2))
        R3, A3, P3, _, D3 = sc.reference(name, new_a=1, new_p=2)
        Ad.set_values(A3.data)
        Dd.set_values(np.full(Dd.nnz, np.nan))
        Dd.ptap_numeric(Pd, Ad)
        assert_values(name + " ptap, new A and P", Dd, D3, k_triple(R3, A3))
        assert Dd.product_info() == info
        Ad.set_values(A.data)
        Pd.set_values(P.data)
        Dd.ptap_numeric(Pd, Ad)
        assert np.array_equal(bits(Dd.values()), bits(first))
    finally:
        destroy(Dd, Ad, Pd)
        restore(ctx)


@pytest.mark.parametrize("name", sc.NAMES)
def test_matmul_path_pattern_and_values(ctx, name):
    """C = A B on the product the case was designed for: the searching kernel, the pattern from the builder the case aims at, and the same arrays and bits
    from the host builder"""
    c = sc.case(name)
    A, B = c.designed()
    ref = sc.product_ld(A, B)
    Ad, Bd, Cd, Ch = ctx.matrix_scipy(A), ctx.matrix_scipy(B), None, None
    try:
        Cd = Ad.matmul(Bd)
        assert Cd.product_info() == [sc.matmul_path(A, B, ref.pattern())]
        assert_pattern(Cd, ref)
        v = assert_values(name + " matmul", Cd, ref, sc.longest_row(A) + 2)
        ctx.set_option("spgemm_device_symbolic", 0)
        Ch = Ad.matmul(Bd)
        assert Ch.product_info() == [sc.matmul_path(A, B, ref.pattern(), device_symbolic=0)]
        assert_pattern(Ch, ref)
        assert np.array_equal(bits(Ch.values()), bits(v))
    finally:
        destroy(Cd, Ch, Ad, Bd)
        restore(ctx)


@pytest.mark.parametrize("name", sc.NAMES)
def test_options_change_the_path_not_the_product(ctx, name):
    """spgemm_device_symbolic 0: the host builder makes both patterns, and arrays and values are the same to the bit.  spgemm_slot_map 0: the searching kernel
    serves both products; where neither product took the lists before, the values are the same to the bit -- the slots and the searching kernel add a * b to
    a zero accumulator in increasing k with the same expression -- and inside the bound elsewhere, the lists sum in another order"""
    from femus_amd import capi
    c = sc.case(name)
    R, A, P, AP, D = sc.reference(name)
    Rd, Ad, Pd, made = ctx.matrix_scipy(R), ctx.matrix_scipy(A), ctx.matrix_scipy(P), []
    try:
        made.append(capi.Mat.abc(Rd, Ad, Pd))
        base = made[0].values()
        kernels = [p["kernel"] for p in made[0].product_info()]
        assert kernels == [p["kernel"] for p in c.paths()]
        ctx.set_option("spgemm_device_symbolic", 0)
        made.append(capi.Mat.abc(Rd, Ad, Pd))
        assert made[1].product_info() == c.paths(device_symbolic=0)
        assert_pattern(made[1], D)
        assert np.array_equal(bits(made[1].values()), bits(base))
        ctx.set_option("spgemm_device_symbolic", 1)
        ctx.set_option("spgemm_slot_map", 0)
        made.append(capi.Mat.abc(Rd, Ad, Pd))
        assert made[2].product_info() == c.paths(slot_map=0)
        assert_pattern(made[2], D)
        v = assert_values(name + " abc, searching kernel", made[2], D, k_triple(R, A))
        if "lists" not in kernels:
            assert np.array_equal(bits(v), bits(base))
    finally:
        destroy(*made, Rd, Ad, Pd)
        restore(ctx)


def test_a_matmul_result_has_no_plan_and_other_matrices_no_record(ctx):
    """the record of the pattern's origin does not make a matmul result reusable by the triple products; a matrix that is no product has no record"""
    c = sc.case("m_3")
    Ad, Pd = ctx.matrix_scipy(c.A), ctx.matrix_scipy(c.P)
    Cd = Ad.matmul(Ad)
    try:
        assert len(Cd.product_info()) == 1
        with pytest.raises(Exception, match="no reusable plan"):
            Cd.ptap_numeric(Pd, Ad)
        with pytest.raises(Exception, match="no reusable plan"):
            Cd.abc_numeric(Ad, Ad, Ad)
        with pytest.raises(Exception, match="not the result"):
            Ad.product_info()
    finally:
        destroy(Cd, Ad, Pd)
        restore(ctx)
