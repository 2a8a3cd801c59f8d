"""The nested-dissection ordering of the exact coarse solve as host code (fh_coarse_dissection): no device, the patterns are built here with numpy."""
import numpy as np
import pytest

from femus_amd import capi


def _q2_interior_pattern(nel):
    """CSR pattern and coordinates of the interior Q2 nodes of a box of nel elements per direction on the unit cube (or square): two nodes are
    coupled when an element holds both"""
    per_dim = []
    for ne in nel:
        node = np.arange(1, 2 * ne)                                 # interior nodes of the 2 ne + 1 on a line
        lo, hi = (node - 1) // 2, node // 2                         # the elements a node lies in: one for a mid-node, two for a vertex
        share = (lo[:, None] <= hi[None, :]) & (lo[None, :] <= hi[:, None])
        per_dim.append((share, node / (2.0 * ne)))
    couple = np.ones((1, 1), bool)
    for share, _ in per_dim:                                        # first direction slowest
        couple = np.kron(couple, share)
    grids = np.meshgrid(*[x for _, x in per_dim], indexing="ij")
    xy = np.stack([g.ravel() for g in grids], axis=1)
    rows, cols = np.nonzero(couple)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=couple.shape[0]))]).astype(np.int32)
    return rowptr, cols.astype(np.int32), xy


@pytest.fixture(scope="module")
def box3d():
    return _q2_interior_pattern((8, 8, 8))


@pytest.fixture(scope="module")
def box2d():
    return _q2_interior_pattern((5, 5))


def _block_sizes(off):
    return list(np.diff(off[:-1])), int(off[-1] - off[-2])


@pytest.mark.parametrize("nd,blocks,separator", [(4, [735] * 4, 435), (8, [343] * 8, 631)])
def test_q2_box_is_cut_at_element_planes(box3d, nd, blocks, separator):
    """the 3375 interior nodes of the 8^3-element level: the block and separator sizes test_dissection_cuts_a_q2_block_at_element_planes asserts
    on the device for the same level"""
    rowptr, col, xy = box3d
    assert rowptr.size - 1 == 3375
    order, off = capi.coarse_dissection(rowptr, col, xy, nd)
    assert _block_sizes(off) == (blocks, separator)


@pytest.mark.parametrize("which,nd", [("box3d", 4), ("box3d", 8), ("box2d", 2), ("box2d", 4)])
def test_order_is_a_permutation_and_blocks_do_not_touch(request, which, nd):
    rowptr, col, xy = request.getfixturevalue(which)
    n = rowptr.size - 1
    order, off = capi.coarse_dissection(rowptr, col, xy, nd)
    assert np.array_equal(np.sort(order), np.arange(n))
    assert np.all(np.diff(off) >= 0) and off[0] == 0 and off[-1] == n
    k = off.size - 2
    assert k >= 2
    block_of = np.full(n, -1)                                       # -1: separator
    for i in range(k):
        block_of[order[off[i]:off[i + 1]]] = i
    bi, bj = block_of[np.repeat(np.arange(n), np.diff(rowptr))], block_of[col]
    assert not np.any((bi >= 0) & (bj >= 0) & (bi != bj))           # no stored entry joins two different interior blocks


@pytest.mark.parametrize("nel,nd", [((3, 3), 8), ((8, 8, 8), 0), ((8, 8, 8), 1), ((5, 5), 1)])
def test_nothing_to_cut_is_one_block_in_the_identity_order(request, nel, nd):
    """fewer than 64 unknowns (3 x 3 elements: 25 interior nodes), or coarse_nd 0 / 1"""
    rowptr, col, xy = request.getfixturevalue("box3d") if nel == (8, 8, 8) else _q2_interior_pattern(nel)
    n = rowptr.size - 1
    order, off = capi.coarse_dissection(rowptr, col, xy, nd)
    assert list(off) == [0, n, n]
    assert np.array_equal(order, np.arange(n))
