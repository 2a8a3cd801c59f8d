"""The transfer of an element mesh as app_poisson._prolongator_from_children builds it on the host, against a plain restatement of its rule: for every shape
(names sorted as strings), child j, fine local node n, coarse local function k with a non-zero weight EP[j][n][k] and coarse element e of the shape, the weight is
INSERTED at (ed_f[nch e + j][n], ed_c[e][k]) -- in the order (shape, j, n, k, e), the last insertion of an entry stays, a zero weight adds no entry.  This is
the yardstick of the device builder (tests/test_gpu_element_transfer.py), which imports the host builder from here.  No device: the matrix the host builder
would upload is caught on its way to capi.Mat.from_csr.

The same walk records what the rule's fine print decides on these meshes -- whether an entry ever receives two different weights (then "the last insertion"
matters) and whether two elements that hold a fine dof ever give its row different columns (then "the union" matters); DESIGN section 4.2 quotes the result."""
import functools

import numpy as np
import pytest

from femus_amd import app_poisson as app
from femus_amd import capi, mixed_mesh
from test_gpu_element_mesh import MESHES, MIXED_CUBE, host_chain

FAMILIES = ["linear", "serendipity", "biquadratic"]
FAM = {"linear": 0, "serendipity": 1, "biquadratic": 2}
TET15_MESHES = ("cube_Tet.neu", MIXED_CUBE)


class _Builder:
    """what _prolongator_from_children reads of a Poisson001"""

    def __init__(self, fe):
        self.fe, self.ctx = fe, None


def groups_of(kind, fe):
    """(shape, its elements, dofs per element) in the order run_elements passes them"""
    return [(s, np.nonzero(kind == s)[0], mixed_mesh.CLASSES[s][FAM[fe]]) for s in sorted(set(kind.tolist()))]


def host_prolongator(fe, coarse, fine):
    """(rowptr, col, val) of the matrix the host builder hands to capi.Mat.from_csr for two consecutive levels (kind, ed, xs, ff, own)"""
    got = []
    keep = capi.Mat.__dict__["from_csr"]
    capi.Mat.from_csr = classmethod(lambda cls, ctx, m, n, rowptr, col, val=None: got.append((int(m), int(n), np.array(rowptr), np.array(col), np.array(val))))
    try:
        app.Poisson001._prolongator_from_children(_Builder(fe), groups_of(coarse[0], fe), coarse[1], fine[1], coarse[4][FAM[fe]], fine[4][FAM[fe]])
    finally:
        capi.Mat.from_csr = keep
    (m, n, rowptr, col, val), = got
    assert (m, n) == (fine[4][FAM[fe]], coarse[4][FAM[fe]]) and rowptr.shape == (m + 1,) and rowptr[-1] == col.size == val.size
    return rowptr.astype(np.int64), col.astype(np.int64), val.astype(np.float64)


@functools.lru_cache(maxsize=None)
def host_transfer(name, fe, level):
    """the host builder's matrix from `level` into `level + 1` of the chain of tests/test_gpu_element_mesh.py, read-only"""
    chain = host_chain(name, False)
    out = host_prolongator(fe, chain[level], chain[level + 1])
    for a in out:
        a.setflags(write=False)
    return out


def restated(fe, coarse, fine):
    """the rule, insertion by insertion into a dict; beside it every weight an entry ever received and the columns each (fine element, node) gives its row"""
    kind, ed_c, ed_f = coarse[0], coarse[1], fine[1]
    entries, seen, patterns = {}, {}, {}
    for s in sorted(set(kind.tolist())):
        EP = capi.fe_elem_prolongator(s, fe)
        nch, nc = EP.shape[0], mixed_mesh.CLASSES[s][FAM[fe]]
        assert EP.shape == (nch, nc, nc)
        for j in range(nch):
            for n in range(nc):
                for k in range(nc):
                    w = EP[j, n, k]
                    if w == 0.0:
                        continue
                    for e in np.nonzero(kind == s)[0]:
                        f = nch * int(e) + j
                        r, c = int(ed_f[f, n]), int(ed_c[e, k])
                        entries[(r, c)] = w
                        seen.setdefault((r, c), set()).add(np.float64(w).tobytes())
                        patterns.setdefault(r, {}).setdefault(f, set()).add(c)
    return entries, seen, patterns


@pytest.mark.parametrize("fe", FAMILIES)
@pytest.mark.parametrize("name", MESHES)
def test_the_host_builder_is_the_stated_rule(name, fe):
    chain = host_chain(name, False)
    rowptr, col, val = host_transfer(name, fe, 0)
    entries, seen, patterns = restated(fe, chain[0], chain[1])
    m = chain[1][4][FAM[fe]]
    assert len(entries) == col.size and sorted(patterns) == list(range(m))           # every fine dof of the family has a row
    keys = sorted(entries)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    assert np.array_equal(rows, [k[0] for k in keys]) and np.array_equal(col, [k[1] for k in keys])        # rows in order, columns ascending inside a row
    assert np.array_equal(val.view(np.uint64), np.array([entries[k] for k in keys]).view(np.uint64))
    # what the fine print of the rule decides here
    two_weights = sum(len(b) > 1 for b in seen.values())
    two_patterns = sum(len({frozenset(c) for c in by_elem.values()}) > 1 for by_elem in patterns.values())
    print("%s %s: %d entries, %d with two different weights, %d of %d rows whose elements disagree on the columns" % (name, fe, len(entries), two_weights, two_patterns, m))
    # found: the weights of TET15 (the P2 + bubble family of the tetrahedron) reach a shared fine dof with different last bits from different children, so on
    # meshes with tetrahedra the biquadratic transfer depends on WHICH insertion is the last; no other shape or family does, and the columns never differ
    assert (two_weights > 0) == (fe == "biquadratic" and name in TET15_MESHES)
    assert two_patterns == 0
