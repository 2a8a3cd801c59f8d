"""mixed_mesh.boundary_faces / boundary_owners -- the face loop of app_poisson.Poisson001.run_elements stated on arrays -- against a literal transcription of that
loop: elements and faces in order, a dictionary per dof, the last writer stays.  They are the host yardstick of capi.ElementMesh.boundary_faces /
boundary_owners (tests/test_gpu_element_plan.py).  No device."""
import itertools

import numpy as np
import pytest

from femus_amd import capi, mixed_mesh
from test_element_refine_flagged_host import flagged_chain
from test_element_transfer_host import FAM, FAMILIES
from test_gpu_element_mesh import MESHES, host_chain
from test_gpu_element_transfer import host_boundary_sets


def face_loop(level, fe, flags):
    """run_elements' loop over the faces of `flags`: (faces [(element, face, nodes)] in its order, {dof: (flag, coordinates)} as its dictionary ends up)"""
    kind, ed, xs, ff = level[:4]
    fn_by = {s: [capi.fe_face_nodes(s, fe, f) for f in range(mixed_mesh.NFACES[s])] for s in sorted(set(kind.tolist()))}
    faces, val = [], {}
    for iel, f in zip(*np.nonzero(ff < -1)):
        flag = int(ff[iel, f])
        if flag not in flags:
            continue
        nodes = ed[iel, fn_by[kind[iel]][f]]
        faces.append((int(iel), int(f), [int(n) for n in nodes]))
        for node in nodes:
            val[int(node)] = (flag, xs[node])
    return faces, val


def flag_subsets(level0):
    """single flags, pairs, all of them, one that no face carries, none; flags in an order that is not ascending"""
    flags = sorted({int(f) for f in np.unique(level0[3]) if f < -1})
    subs = [(f,) for f in flags] + list(itertools.islice(itertools.combinations(flags[::-1], 2), 8)) + [tuple(flags), (-1000,), ()]
    return flags, subs


def check_level(level, fe, sub):
    """both statements against the loop; returns how many dofs lie on faces of two different flags of `sub`"""
    faces, val = face_loop(level, fe, set(sub))
    elem, face, nodes, nn = mixed_mesh.boundary_faces(level, fe, sub)
    assert elem.shape == face.shape == nn.shape == (len(faces),) and nodes.shape == (len(faces), 9)
    assert [(int(e), int(f), [int(n) for n in row[:k]]) for e, f, row, k in zip(elem, face, nodes, nn)] == faces
    assert all((row[k:] == -1).all() for row, k in zip(nodes, nn))
    dofs, owner, xy = mixed_mesh.boundary_owners(level, FAM[fe], sub)
    want = sorted(val)
    assert dofs.tolist() == want and owner.tolist() == [val[d][0] for d in want]
    assert xy.shape == (len(want), level[2].shape[1]) and all(np.array_equal(xy[k].view(np.uint64), val[d][1].view(np.uint64)) for k, d in enumerate(want))
    by_flag = host_boundary_sets(level[:5], fe)
    assert set(want) == set().union(*[by_flag.get(f, set()) for f in sub])
    return sum(1 for d in want if sum(d in by_flag.get(f, ()) for f in set(sub)) > 1)


@pytest.mark.parametrize("name", MESHES)
def test_the_array_statements_equal_the_face_loop(name):
    chain = host_chain(name, False)
    flags, subs = flag_subsets(chain[0])
    for level in chain:
        decided = 0
        for fe in FAMILIES:
            for sub in subs:
                decided += check_level(level, fe, sub)
        by_flag = host_boundary_sets(level, "linear")
        meet = any(by_flag[a] & by_flag[b] for a, b in itertools.combinations(flags, 2))
        print("%s, %d elements: %d flags, %d (dof, subset, family) cases where two listed flags meet" % (name, level[0].shape[0], len(flags), decided))
        assert (decided > 0) == meet


def test_the_overwrite_rule_decides_on_an_edge_of_the_cube():
    """two flags meet on an edge of cube_Tet.neu: the dofs there belong to the face that comes later in the walk, which is not always the same flag"""
    level = host_chain("cube_Tet.neu", False)[1]
    flags, _ = flag_subsets(level)
    by_flag = host_boundary_sets(level, "biquadratic")
    a, b = next((a, b) for a, b in itertools.combinations(flags, 2) if by_flag[a] & by_flag[b])
    dofs, owner, _ = mixed_mesh.boundary_owners(level, "biquadratic", [a, b])
    shared = np.isin(dofs, sorted(by_flag[a] & by_flag[b]))
    assert shared.sum() > 2 and set(owner[shared].tolist()) <= {a, b}
    _, val = face_loop(level, "biquadratic", {a, b})
    assert owner[shared].tolist() == [val[int(d)][0] for d in dofs[shared]]
    assert set(owner[~shared & np.isin(dofs, sorted(by_flag[a]))].tolist()) == {a}


def test_a_flagged_level():
    chain = flagged_chain("triAMR.neu", False)
    flags, subs = flag_subsets(chain[0])
    for level in chain[1:]:
        assert len(set(level[5].tolist())) > 1                   # elements of several levels
        for fe in FAMILIES:
            for sub in subs:
                check_level(level, fe, sub)
