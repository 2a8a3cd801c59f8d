"""The batched element loop of the simplex, prism and mixed-shape oracles (oracle/femus_oracle_mixed.py: assemble_batched) against the plain loops it
restates (femus_oracle_{tri,tet,wedge,mixed}.assemble): every shape, family and Gauss rule on two-level meshes with curved elements, a non-polynomial source
and a non-zero state, 1e-14 relative to the largest entry.  CPU only."""
import os

import numpy as np
import pytest

from oracle import femus_oracle_mixed as om
from oracle import femus_oracle_tet as oq
from oracle import femus_oracle_tri as ot
from oracle import femus_oracle_wedge as ow

HERE = os.path.dirname(os.path.abspath(__file__))
RULES = ["first", "third", "fifth", "seventh", "ninth"]
FES = ["linear", "serendipity", "biquadratic"]


def _bend(xs):
    """nodes moved smoothly inside the unit box (curved elements), the boundary kept"""
    return xs + 0.01 * np.sin(5 * xs[:, list(range(1, xs.shape[1])) + [0]]) * (xs * (1 - xs)).prod(axis=1, keepdims=True) * 60


def _source(x):
    return np.exp(x[0]) * (1 + x[1]) - (x[2] if len(x) > 2 else 0.0)


def _meshes():
    """name -> (kind for assemble_batched, loop routine(ed, xs, fe, source, sol, order), element table, coordinates, nodes by family)"""
    out = {}
    ed, xs, ff, own = ot.refine(*ot.box_mesh(3, 2)[:3])
    out["tri"] = ("tri", ot.assemble, ed, _bend(xs), own)
    ed, xs, ff, own = oq.refine(*oq.read_gambit(os.path.join(HERE, "golden", "cube_Tet.neu"))[:3])
    out["tet"] = ("tet", oq.assemble, ed, _bend(xs), own)
    ed, xs, ff, own = ow.refine(*ow.read_gambit(os.path.join(HERE, "golden", "cube_Wedge.neu"))[:3])
    out["wedge"] = ("wedge", ow.assemble, ed, _bend(xs), own)
    for name, mesh in (("mixed3d", "cube_all_shapes_Six_boundary_groups.neu"), ("mixed2d", "square_mixed.neu")):
        kind, ed, xs, ff, own = om.refine(*om.read_gambit(os.path.join(HERE, "golden", mesh))[:4])
        lo, hi = xs.min(axis=0), xs.max(axis=0)
        xs = lo + _bend((xs - lo) / (hi - lo)) * (hi - lo)
        out[name] = (kind, lambda ed, xs, fe, source, sol, order, kind=kind: om.assemble(kind, ed, xs, fe, source, sol, order), ed, xs, own)
    return out


MESHES = {}


@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("mesh", ["tri", "tet", "wedge", "mixed3d", "mixed2d"])
def test_batched_oracle_equals_the_element_loop(mesh, fe, order):
    if not MESHES:
        MESHES.update(_meshes())
    kind, loop, ed, xs, own = MESHES[mesh]
    ndof = om.n_dofs(own, fe)
    u = np.random.default_rng(5).uniform(-1, 1, ndof)
    K, F = loop(ed, xs, fe, _source, u, order)
    Kb, Fb = om.assemble_batched(kind, ed, xs, fe, _source, sol=u, order=order, chunk=97)     # several chunks, the last one partial
    K = K.toarray() if hasattr(K, "toarray") else K
    Kb = Kb.toarray()
    assert Kb.shape == K.shape == (ndof, ndof) and Fb.shape == F.shape
    assert np.abs(Kb - K).max() <= 1e-14 * np.abs(K).max()
    assert np.abs(Fb - F).max() <= 1e-14 * np.abs(F).max()
    # the state enters: without it the residual is the load alone
    _, F0 = om.assemble_batched(kind, ed, xs, fe, _source, order=order)
    assert np.abs(F0 - Fb).max() > 1e-3 * np.abs(F).max()
