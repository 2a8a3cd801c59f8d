"""The designed operands of tests/spgemm_cases.py, checked without a GPU: every case has the structure it claims (mean rows, longest rows, distinct counts,
hash chains) and therefore the path through fh_spgemm.hip it was built for (expected_path), and scipy's float64 product of it stays inside the componentwise
bound of the long-double restatement -- the same bound tests/test_gpu_sparse_products.py holds the device to.  The GPU tests then assert that the library
reports the same path (fh_mat_product_info)."""
import numpy as np
import pytest
import scipy.sparse as sp

import spgemm_cases as sc


def designed_path(name, **options):
    c = sc.case(name)
    return c.paths(**options)[c.pair]


def designed_pattern(name):
    A, B = sc.case(name).designed()
    return A, B, sc.product_ld(A, B).pattern()


def test_long_double_is_longer_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_hash_restated():
    """the 32-bit product of the kernel, on values worked out by hand: 1 * 2654435761 >> 21 = 1265, and the wrap of the product at 2^32"""
    assert sc.sy_hash(0) == 0 and sc.sy_hash(1) == 2654435761 >> 21 == 1265
    assert sc.sy_hash(2) == ((2 * 2654435761) - 2 ** 32) >> 21
    assert sc.sy_hash(1499999) == ((1499999 * 2654435761) % 2 ** 32) >> 21
    h = sc.sy_hash(np.arange(sc.HASH_COLS))
    assert h.min() == 0 and h.max() == sc.SY_TAB - 1


def test_gl_log2_six_cannot_be_reached():
    """the loop of build_slot_map allows gl_log2 up to 6, but 6 needs a mean B row above 32 and a mean from 32 on has left for the slots before: over a fine grid
    of means, the lists see 3 (mean <= 8), 4 (<= 16) and 5 (< 32) and nothing else"""
    A = sp.csr_matrix(np.ones((1, 64)))
    seen = set()
    for nnz in range(64, 64 * 40):
        mean = nnz / 64.0
        lens = np.full(64, nnz // 64)
        lens[:nnz % 64] += 1
        B = sp.csr_matrix((np.ones(nnz), np.concatenate([np.arange(k) for k in lens]), np.concatenate([[0], np.cumsum(lens)])), shape=(64, 64))
        C = sp.csr_matrix(np.ones((1, int(lens.max()))))
        C.resize(1, 64)
        e = sc.expected_path(A, B, C)
        assert e["kernel"] == ("lists" if mean < 32 else "slots")
        if e["kernel"] == "lists":
            assert e["gl_log2"] == (3 if mean <= 8 else 4 if mean <= 16 else 5)
            seen.add(e["gl_log2"])
    assert seen == {3, 4, 5}


@pytest.mark.parametrize("name", sc.MEAN_B)
def test_mean_b_cases(name):
    mean, delta = sc.MEAN_B[name]
    c = sc.case(name)
    P = c.P
    assert P.nnz == mean * P.shape[0] + delta and c.design["mean_b"] == (P.nnz, P.shape[0])
    lens = np.diff(P.indptr)
    assert lens.min() == 0 and lens.max() > 64 and (lens == 1).sum() >= 3 and (lens == 0).sum() >= 3
    e = designed_path(name)
    m = P.nnz / P.shape[0]
    assert e["kernel"] == ("lists" if m < 32 else "slots")
    assert e["gl_log2"] == {"mean_b_8": 3, "mean_b_8_above": 4, "mean_b_16": 4, "mean_b_16_above": 5, "mean_b_24_below": 5, "mean_b_24": 5,
                            "mean_b_32_below": 5, "mean_b_32": None}[name]
    assert e["pattern"] == "device" and e["lanes_over_b"] == (1 if name in ("mean_b_24", "mean_b_32_below", "mean_b_32") else 0)
    assert e["products"] == int(lens[c.A.indices].sum()) > 0


@pytest.mark.parametrize("name", [n for n in sc.NAMES if sc.BUILDERS[n] is sc._long_row])
def test_long_row_cases(name):
    kind, what, count, place = name.split("_")
    count = int(count)
    c = sc.case(name)
    A, B, C = designed_pattern(name)
    assert A.shape[0] == 203 and A.shape[0] % 4 != 0 and c.design["row"] == sc.PLACES[place] and c.pair == (1 if place == "middle" else 0)
    clen, alen = np.diff(C.indptr), np.diff(A.indptr)
    at = c.design["row"]
    e = designed_path(name)
    mean = B.nnz / B.shape[0]
    if what == "crow":
        assert clen[at] == count == clen.max() and np.sum(clen == count) == 1 and np.delete(clen, at).max() < count - 100
        assert (mean < 32) == (kind == "lists") and alen.max() <= 200
        limit = sc.LISTS_CROW if kind == "lists" else sc.SLOTS_CROW
        assert count in (limit, limit + 1)
        assert e["kernel"] == (kind if count == limit else "searching") and e["pattern"] == "host"
        if count == limit:
            assert e["max_crow"] == limit
    else:
        assert alen[at] == count == alen.max() and np.delete(alen, at).max() <= 6 and clen.max() <= 40 and mean < 8
        assert count in (sc.LISTS_AROW, sc.LISTS_AROW + 1)
        assert e["kernel"] == ("lists" if count == sc.LISTS_AROW else "searching") and e["pattern"] == "device" and e["lanes_over_b"] == 0
        if count == sc.LISTS_AROW:
            assert e["max_arow"] == sc.LISTS_AROW and e["gl_log2"] == 3


@pytest.mark.parametrize("name", [n for n in sc.NAMES if sc.BUILDERS[n] is sc._pattern_counts])
def test_pattern_count_cases(name):
    c = sc.case(name)
    A, B, C = designed_pattern(name)
    clen = np.diff(C.indptr)
    assert sorted(clen.tolist()) == c.design["counts"]
    assert set(sc.COUNTS) <= set(clen.tolist()) and (1025 in clen) == ("1025" in name)
    assert np.sum((clen == 0) & (np.diff(A.indptr) > 0)) == 1                 # a row of A that names empty rows of B only
    products = np.diff(B.indptr)[A.indices].sum()
    if "dup" in name:
        assert products >= 3 * C.nnz                                            # every column of C named three times and more
    else:
        assert products == C.nnz
    for both in c.paths():
        assert both["pattern"] == ("host" if "1025" in name else "device")
    e = designed_path(name)
    assert e["lanes_over_b"] == (None if "1025" in name else 1 if "long_b" in name else 0)
    assert e["kernel"] == ("slots" if "long_b" in name else "lists")


@pytest.mark.parametrize("name", ["hash_one_slot", "hash_wrap", "hash_over_half", "hash_overfull"])
def test_hash_cases(name):
    c = sc.case(name)
    A, B, C = designed_pattern(name)
    row = C.indices[C.indptr[c.design["row"]]:C.indptr[c.design["row"] + 1]]
    assert np.array_equal(row, c.design["columns"])
    h = sc.sy_hash(row)
    e = designed_path(name)
    if name == "hash_one_slot":
        assert row.size == 600 and np.all(h == 777) and e["pattern"] == "device"
    elif name == "hash_wrap":
        assert row.size == 300 and np.all(h == 2040) and 2040 + 300 > sc.SY_TAB and e["pattern"] == "device"       # slots 2040 .. 2047, then 0 .. 291
    elif name == "hash_over_half":
        assert sc.SY_TAB // 2 < row.size == 1100 < sc.SY_TAB and e["pattern"] == "host"
    else:
        assert row.size == 2100 > sc.SY_TAB and e["pattern"] == "host"
    assert np.diff(C.indptr).max() == row.size


def test_two_builders_case():
    c = sc.case("two_builders")
    first, second = c.paths()
    assert first["pattern"] == "device" and second["pattern"] == "host"
    A, B, C = designed_pattern("two_builders")
    assert np.diff(C.indptr)[c.design["row"]] == c.design["c_row"] == 1200 and np.diff(B.indptr).max() <= 1024


@pytest.mark.parametrize("name", sc.ENTRY_FILL)
def test_entry_product_cases(name):
    c = sc.case(name)
    A, B, C = designed_pattern(name)
    count = (abs(sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)) @ sp.csr_matrix((np.ones(B.nnz), B.indices, B.indptr), shape=B.shape)).tocsr()
    for p, col in c.design["columns"].items():
        assert count[c.design["row"], col] == p
    assert np.any(np.diff(B.indptr)[A.indices] == 0)                           # entries of A that point at empty rows of B
    e = designed_path(name)
    assert e["kernel"] == "lists" and e["gl_log2"] == int(name[-1])


def test_crow_lengths_case():
    A, B, C = designed_pattern("crow_lengths")
    assert np.diff(C.indptr).tolist() == sc.case("crow_lengths").design["c_rows"]
    assert designed_path("crow_lengths")["kernel"] == "lists"


def test_small_and_empty_cases():
    c = sc.case("empty_rows")
    alen, plen = np.diff(c.A.indptr), np.diff(c.P.indptr)
    assert np.all(alen[0:7] == 0) and np.all(alen[20:31] == 0) and np.all(alen[47:50] == 0)
    assert alen[12] > 0 and np.all(plen[c.A.indices[c.A.indptr[12]:c.A.indptr[13]]] == 0)
    assert np.diff(c.Rx().indptr)[-1] == 0
    A, B, C = designed_pattern("no_entries")
    assert A.nnz > 0 and B.nnz > 0 and C.nnz == 0
    assert [p["pattern"] for p in sc.case("no_entries").paths()] == ["device", "host"]
    assert sc.case("one_by_one").A.shape == (1, 1) and sc.case("one_row").R.shape[0] == 1 and sc.case("one_column").P.shape[1] == 1
    assert [sc.case("m_%d" % m).A.shape[0] for m in range(1, 6)] == [1, 2, 3, 4, 5]
    assert sc.PTAP_NAMES == tuple(n for n in sc.NAMES if sc.case(n).R is None)


@pytest.mark.parametrize("name", ["cancel_inner", "cancel_outer"])
def test_cancelling_cases_keep_their_zeros(name):
    A, B, C = designed_pattern(name)
    ref = sc.product_ld(A, B)
    assert ref.val.size == C.nnz > 0 and np.all(ref.val == 0) and np.all(ref.absval > 0)
    assert (A @ B).tocsr().count_nonzero() == 0


def test_every_threshold_has_a_case_on_either_side():
    kernels = {n: [p["kernel"] for p in sc.case(n).paths()] for n in sc.NAMES}
    assert any("slots" in k for k in kernels.values()) and any("lists" in k for k in kernels.values()) and any("searching" in k for k in kernels.values())
    # cases that never take the lists serve the bit comparison of the slots with the searching kernel
    assert sum(1 for k in kernels.values() if "slots" in k and "lists" not in k) >= 3
    for n in sc.NAMES:
        for p in sc.case(n).paths(slot_map=0):
            assert p["kernel"] == "searching" and p["products"] == 0
        for p in sc.case(n).paths(device_symbolic=0):
            assert p["pattern"] == "host" and p["lanes_over_b"] is None


RATIOS = {}


@pytest.mark.parametrize("name", sc.NAMES)
def test_scipy_float64_is_inside_the_bound(name):
    """the float64 reference the other suites compare with is itself inside the componentwise bound, for one product and for the triple product"""
    c = sc.case(name)
    R, A, P, AP, D = sc.reference(name)
    r1 = sc.ratio(sc.on_pattern(A @ P, AP), AP, sc.longest_row(A) + 2)
    r3 = sc.ratio(sc.on_pattern(R @ (A @ P), D), D, sc.longest_row(R) + sc.longest_row(A) + 4)
    A2, B2 = c.designed()
    C2 = sc.product_ld(A2, B2)
    r2 = sc.ratio(sc.on_pattern(A2 @ B2, C2), C2, sc.longest_row(A2) + 2)
    RATIOS[name] = max(r1, r2, r3)
    print("%s: error / bound of scipy in float64: A P %.3g, designed product %.3g, R A P %.3g" % (name, r1, r2, r3))
    assert r1 <= 1.0 and r2 <= 1.0 and r3 <= 1.0
    # new values keep the pattern
    R2, A2, P2, AP2, D2 = sc.reference(name, new_a=1, new_p=2)
    assert np.array_equal(D2.indices, D.indices) and np.array_equal(D2.indptr, D.indptr)
    assert D.val.size == 0 or name == "cancel_outer" or not np.array_equal(D2.val, D.val)
