"""TEST INFRASTRUCTURE ONLY.  The meshes, vectors and thresholds that tests/test_element_error_flag_host.py and tests/test_gpu_element_error_flag.py share, and the
literal reference's results on them (tests/amr_flag_reference.py), computed once per case and left unchanged.

Meshes: the golden files, (a) as read and once uniformly refined; (b) that mesh with about half of its elements flagged by a half-space (flagged_chain_of of
tests/test_element_refine_flagged_host.py) and refined once more, so that elements of an older level are present; the mixed cube as read.  sol = lcg_fill, eps =
lcg_fill with another seed times a bump that is exactly zero outside a ball around the corner of largest coordinates (which lies in the refined half), so that
far elements have err_i == 0.  RADIUS (in units of the mesh's extent) and THRESHOLD were searched once so that the conditions check_inputs() asserts hold, and are
fixed here.  Some cases run with the third- and fifth-order rules: other tables, and fewer turns of the literal reference's Python loop over every Gauss point."""
import functools

import numpy as np

import amr_flag_reference as ref
from oracle import femus_oracle as fo
from test_element_refine_flagged_host import flagged_chain_of
from test_gpu_element_mesh import MIXED_CUBE, coarse, host_chain

SEED_SOL, SEED_EPS = 2024, 77
NEIGHBOR = (0.0, 0.25)
NORMS = ("L2", "H1")

# (file, distorted, variant, Gauss rule, families)
MESHES = [
    ("tri2.neu", False, "a", "seventh", (0, 1, 2)),
    ("tri2.neu", False, "b", "seventh", (0, 1, 2)),
    ("square_mixed.neu", False, "a", "seventh", (0, 1, 2)),
    ("square_mixed.neu", True, "b", "seventh", (0, 1, 2)),
    ("square_mixed.neu", False, "b", "fifth", (2,)),
    ("cube_Tet.neu", False, "a", "third", (1,)),
    ("cube_Tet.neu", False, "b", "third", (0,)),
    ("cube_Wedge.neu", False, "a", "seventh", (2,)),
    ("cube_Wedge.neu", True, "b", "third", (0, 1)),
    ("cube_Hex.neu", False, "a", "seventh", (1,)),
    ("cube_Hex.neu", False, "b", "third", (0, 2)),
    (MIXED_CUBE, False, "read", "seventh", (0, 1, 2)),
]
RADIUS = 0.55
THRESHOLD = {
    'tri2-a-seventh-fe0-L2': 0.0112,
    'tri2-a-seventh-fe0-H1': 0.0255,
    'tri2-a-seventh-fe1-L2': 0.00123,
    'tri2-a-seventh-fe1-H1': 0.00355,
    'tri2-a-seventh-fe2-L2': 0.00141,
    'tri2-a-seventh-fe2-H1': 0.00264,
    'tri2-b-seventh-fe0-L2': 0.0759,
    'tri2-b-seventh-fe0-H1': 0.258,
    'tri2-b-seventh-fe1-L2': 0.026,
    'tri2-b-seventh-fe1-H1': 0.074,
    'tri2-b-seventh-fe2-L2': 0.0242,
    'tri2-b-seventh-fe2-H1': 0.0545,
    'square_mixed-a-seventh-fe0-L2': 0.00881,
    'square_mixed-a-seventh-fe0-H1': 0.0266,
    'square_mixed-a-seventh-fe1-L2': 0.00149,
    'square_mixed-a-seventh-fe1-H1': 0.00371,
    'square_mixed-a-seventh-fe2-L2': 0.00169,
    'square_mixed-a-seventh-fe2-H1': 0.0026,
    'square_mixed-b-distorted-seventh-fe0-L2': 0.0999,
    'square_mixed-b-distorted-seventh-fe0-H1': 0.287,
    'square_mixed-b-distorted-seventh-fe1-L2': 0.028,
    'square_mixed-b-distorted-seventh-fe1-H1': 0.0496,
    'square_mixed-b-distorted-seventh-fe2-L2': 0.0312,
    'square_mixed-b-distorted-seventh-fe2-H1': 0.12,
    'square_mixed-b-fifth-fe2-L2': 0.0295,
    'square_mixed-b-fifth-fe2-H1': 0.103,
    'cube_Tet-a-third-fe1-L2': 0.0146,
    'cube_Tet-a-third-fe1-H1': 0.063,
    'cube_Tet-b-third-fe0-L2': 0.0496,
    'cube_Tet-b-third-fe0-H1': 0.203,
    'cube_Wedge-a-seventh-fe2-L2': 0.00915,
    'cube_Wedge-a-seventh-fe2-H1': 0.0215,
    'cube_Wedge-b-distorted-third-fe0-L2': 0.0199,
    'cube_Wedge-b-distorted-third-fe0-H1': 0.0717,
    'cube_Wedge-b-distorted-third-fe1-L2': 0.00801,
    'cube_Wedge-b-distorted-third-fe1-H1': 0.0296,
    'cube_Hex-a-seventh-fe1-L2': 0.00861,
    'cube_Hex-a-seventh-fe1-H1': 0.0226,
    'cube_Hex-b-third-fe0-L2': 0.0372,
    'cube_Hex-b-third-fe0-H1': 0.123,
    'cube_Hex-b-third-fe2-L2': 0.00773,
    'cube_Hex-b-third-fe2-H1': 0.0245,
    'cube_all_sha-read-seventh-fe0-L2': 0.0297,
    'cube_all_sha-read-seventh-fe0-H1': 0.15,
    'cube_all_sha-read-seventh-fe1-L2': 0.00845,
    'cube_all_sha-read-seventh-fe1-H1': 0.0299,
    'cube_all_sha-read-seventh-fe2-L2': 0.0111,
    'cube_all_sha-read-seventh-fe2-H1': 0.0103,
}


def mesh_id(m):
    return "%s-%s%s-%s" % (m[0].split(".")[0][:12], m[2], "-distorted" if m[1] else "", m[3])


CASES = [(m, fe, norm) for m in MESHES for fe in m[4] for norm in NORMS]


def case_id(c):
    return "%s-fe%d-%s" % (mesh_id(c[0]), c[1], c[2])


def half_space(dim):
    mid = 0.0 if dim == 2 else 0.5

    def fn(x, level):
        return x[0] > mid
    return fn


@functools.lru_cache(maxsize=None)
def mesh_of(name, distorted, variant):
    """(kind, ed, xs, own, lev, level)"""
    if variant == "read":
        kind, ed, xs, ff, own = coarse(name, distorted)
        return kind, ed, xs, list(own), np.zeros(kind.shape[0], dtype=np.int64), 0
    a = host_chain(name, distorted)[1]
    if variant == "a":
        return a[0], a[1], a[2], list(a[4]), np.zeros(a[0].shape[0], dtype=np.int64), 0
    b = flagged_chain_of(a, n=1, fn=half_space(a[2].shape[1]))[1]
    return b[0], b[1], b[2], list(b[4]), np.asarray(b[5]), 1


@functools.lru_cache(maxsize=None)
def faces_of(name, distorted, variant):
    """ff[nel, 6] of mesh_of's mesh"""
    if variant == "read":
        return coarse(name, distorted)[3]
    a = host_chain(name, distorted)[1]
    return a[3] if variant == "a" else flagged_chain_of(a, n=1, fn=half_space(a[2].shape[1]))[1][3]


def bump(xs, radius):
    """(1 - r^2 / R^2)^2 inside the ball of radius R = radius * extent around the corner of largest coordinates, exactly 0 outside"""
    corner, extent = xs.max(axis=0), float((xs.max(axis=0) - xs.min(axis=0)).max())
    q = ((xs - corner) ** 2).sum(axis=1) / (radius * extent) ** 2
    return np.where(q < 1.0, (1.0 - q) ** 2, 0.0)


def vectors(m, fe, radius=None):
    kind, ed, xs, own, lev, level = mesh_of(*m[:3])
    n = own[fe]
    sol = fo.lcg_fill(n, SEED_SOL)
    eps = fo.lcg_fill(n, SEED_EPS) * bump(xs[:n], RADIUS if radius is None else radius)
    return sol, eps


@functools.lru_cache(maxsize=None)
def gauss_values(m, fe):
    kind, ed, xs, own, lev, level = mesh_of(*m[:3])
    sol, eps = vectors(m, fe)
    return ref.gauss_values(kind, ed, xs, fe, sol, eps, m[3])


@functools.lru_cache(maxsize=None)
def reference(m, fe, norm, neighbor_threshold, threshold=None):
    kind, ed, xs, own, lev, level = mesh_of(*m[:3])
    thr = THRESHOLD[case_id((m, fe, norm))] if threshold is None else threshold
    return ref.walk(gauss_values(m, fe), kind, ed, lev, level, fe, norm, thr, neighbor_threshold, xs.shape[1])


def check_inputs(m, fe, norm, neighbor_threshold, r):
    """what the inputs must provide, asserted on the reference alone"""
    S, W, flags, refinable = r["strong"], r["weak"], r["flags"] != 0, r["refinable"]
    positive = refinable & (r["err2"] > 0)
    frac = S[positive].sum() / max(1, positive.sum())
    assert 0.2 <= frac <= 0.8, "%.2f of the refinable elements with err > 0 are strong" % frac
    assert (flags & ~S).any(), "no element is flagged through the neighbour rule alone"
    if m[2] != "a":
        assert (refinable & ~flags).any(), "every refinable element is flagged"
    if m[2] == "b":
        assert (~refinable).any() and refinable.any()
    assert (refinable & (r["err2"] == 0)).any(), "no far element with err == 0"
    for t in (r["eps2"], neighbor_threshold * r["eps2"]):
        for i in np.nonzero(refinable)[0]:
            if t == 0 and r["err2"][i] == 0:
                continue
            assert abs(r["err2"][i] - t * r["vol"][i]) > 1e-9 * t * r["vol"][i], "element %d sits on the threshold" % i
    # the order-independent form of the rule
    strong_near = np.array([any(S[j] for j in r["near"][i][1:]) for i in range(S.size)])
    assert np.array_equal(flags, S | (W & strong_near))
