"""Gambit neutral-file reader (GambitIO::read) against meshes written by the independent writer of
tests/gambit_writer.py, and against the reference's own input files when the reference tree is present (this container only)."""
import os

import numpy as np
import pytest

from femus_amd import capi
from oracle import femus_oracle as fo

from gambit_writer import write_neu
from reference_files import reference_file


@pytest.mark.parametrize("box", [(3, 2, 0), (2, 3, 2)])
def test_reader_round_trip_of_a_box_mesh(tmp_path, box):
    mo = fo.coarse_box_mesh(*box, lo=(-1., 0., 0.5), hi=(2., 1., 1.5))
    path = tmp_path / "box.neu"
    write_neu(path, mo.geom, mo.elem_dof, mo.coords, mo.face_flag)
    m = capi.Mesh.read_gambit(path)
    ed, xy, ff = m.arrays()
    assert np.array_equal(ed, mo.elem_dof)                      # same elements, same first-touch numbering
    assert np.allclose(xy, mo.coords, rtol=0, atol=1e-10)       # "%20.11e" in the file
    assert np.array_equal(ff, mo.face_flag)
    assert m.own_size == list(mo.own_size)
    f = m.refine()                                              # the read mesh feeds the refinement like a generated one
    assert f.nel == m.nel * 2 ** m.dim
    m.destroy(), f.destroy()


def test_reader_scales_coordinates_and_reports_errors(tmp_path):
    mo = fo.coarse_box_mesh(2, 2, 0)
    path = tmp_path / "q.neu"
    write_neu(path, mo.geom, mo.elem_dof, mo.coords, mo.face_flag)
    m = capi.Mesh.read_gambit(path, Lref=2.0)
    assert np.allclose(m.arrays()[1], mo.coords / 2.0, atol=1e-10)
    m.destroy()
    with pytest.raises(capi.FemusHipError, match="can not read parameters"):
        capi.Mesh.read_gambit(tmp_path / "missing.neu")
    bad = tmp_path / "bad.neu"
    bad.write_text(open(path).read().replace(" 2  9 ", " 2  8 ", 1))
    with pytest.raises(capi.FemusHipError, match="Invalid element type"):
        capi.Mesh.read_gambit(bad)


REF = "/root/reference/applications"
FILES = [("003_NavierStokes/SteadyNavierStokesParallel/input/box10x10.neu", "quad", 100, 441, {-2: 10, -3: 30}),
         ("001_Poisson/input/cube_Hex.neu", "hex", 8, 125, {-2: 4, -3: 4, -4: 4, -5: 4, -6: 4, -7: 4})]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present")
@pytest.mark.parametrize("rel,geom,nel,nnode,sets", FILES)
def test_reader_on_the_reference_input_files(rel, geom, nel, nnode, sets):
    m = capi.Mesh.read_gambit(os.path.join(REF, rel))
    ed, xy, ff = m.arrays()
    assert (m.nel, m.nnode) == (nel, nnode)
    assert {int(k): int(v) for k, v in zip(*np.unique(ff[ff < -1], return_counts=True))} == sets
    Xc = fo.xc_table(geom).astype(float)
    fn = fo.face_nodes(geom)
    lo, hi = xy.min(0), xy.max(0)
    for e in range(nel):
        X = xy[ed[e]]
        H = np.stack([(X[1] - X[0]) / 2, (X[3] - X[0]) / 2] + ([(X[4] - X[0]) / 2] if m.dim == 3 else []))
        assert np.allclose(X, X[-1] + Xc @ H) and np.linalg.det(H) > 0     # FEMuS local order, right-handed
        for f in range(ff.shape[1]):                                       # flagged faces = faces on the bounding box
            P = xy[ed[e, fn[f]]]
            on = any(np.allclose(P[:, k], lo[k]) or np.allclose(P[:, k], hi[k]) for k in range(m.dim))
            assert on == (ff[e, f] < -1)
    m.destroy()


def test_reader_orders_elements_by_material_then_group(tmp_path):
    """Mesh::mesh_reorder_elem_quantities: elements sorted by (material, group, file order) before the node numbering"""
    mo = fo.coarse_box_mesh(3, 2, 0)
    groups = [(7, 4, [0, 3]), (6, 2, [1, 5]), (9, 2, [2, 4])]          # (group name, material, elements)
    path = tmp_path / "g.neu"
    write_neu(path, mo.geom, mo.elem_dof, mo.coords, mo.face_flag, groups=groups)
    m = capi.Mesh.read_gambit(path)
    ed, xy, ff = m.arrays()
    expect = [1, 5, 2, 4, 0, 3]                                          # material 2 (groups 6, 9), then material 4
    centre = lambda X: np.round(X[:, 8], 12)
    assert np.allclose(xy[ed[:, 8]], mo.coords[mo.elem_dof[expect, 8]], atol=1e-10)     # element centres in the new order
    assert np.array_equal(ff, mo.face_flag[expect])
    # first-touch numbering of the reordered elements: vertices of the first element come first
    assert sorted(ed[0, :4].tolist()) == [0, 1, 2, 3]
    m.destroy()


def test_reader_on_the_curved_mesh_of_testNSSteadyDD():
    """unittests/testNSSteadyDD/input/nsbenc.neu (the mesh behind the reference's stored norms, main.cpp:202-244): 98 curved QUAD9
    elements around a cylinder, 3 element groups, 4 boundary sets -- every element comes out right-handed in FEMuS local order with
    edge nodes between their vertices, every node belongs to an element, and the boundary faces are exactly the faces met once"""
    m = capi.Mesh.read_gambit(reference_file("unittests/testNSSteadyDD/input/nsbenc.neu"))
    ed, xy, ff = m.arrays()
    assert (m.nel, m.nnode, m.dim) == (98, 442, 2)
    assert set(np.unique(ff).tolist()) == {-5, -4, -3, -2, -1}                        # sets 1..4 -> flags -2..-5 (GambitIO.cpp:337)
    assert np.unique(ed).size == 442
    edge_v = [(0, 1), (1, 2), (2, 3), (3, 0)]
    seen = {}
    for e in range(m.nel):
        X = xy[ed[e]]
        area = 0.5 * sum(X[a][0] * X[b][1] - X[b][0] * X[a][1] for a, b in edge_v)
        assert area > 0                                                                # counter-clockwise
        for k, (a, b) in enumerate(edge_v):
            assert np.linalg.norm(X[4 + k] - 0.5 * (X[a] + X[b])) < 0.2 * np.linalg.norm(X[a] - X[b])     # mid node near the chord
            key = tuple(sorted((int(ed[e, a]), int(ed[e, b]))))
            seen.setdefault(key, []).append((e, k))
    for key, uses in seen.items():
        assert len(uses) in (1, 2)
        for e, k in uses:
            assert (ff[e, k] < -1) == (len(uses) == 1)                                 # boundary set <=> an edge met once
    # refinement of the curved mesh: children keep the orientation, node count as for any QUAD9 refinement
    f = m.refine()
    assert f.nel == 4 * 98
    m.destroy(), f.destroy()


def test_element_groups_of_the_known_answer_mesh_and_its_selective_levels():
    """unittests/testNSSteadyDD: the Gambit groups 5 / 6 / 7 of nsbenc.neu drive SetRefinementFlag (main.cpp:262-280: group 5 is refined on the two
    selective levels above the four uniform ones, main.cpp:55-82); children inherit group and material (MeshRefinement.cpp:263-266)"""
    import os
    m = capi.Mesh.read_gambit(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nsbenc.neu"))
    g, mt = m.elem_groups()
    assert dict(zip(*np.unique(g, return_counts=True))) == {5: 20, 6: 40, 7: 38} and set(mt) == {2}
    ms = [m]
    for l in range(1, 6):
        g, _ = ms[-1].elem_groups()
        lev, _ = ms[-1].elem_levels()
        flags = np.ones(ms[-1].nel, np.uint8) if l < 4 else ((g == 5) & (lev == ms[-1].level)).astype(np.uint8)
        nxt = ms[-1].refine_flagged(flags)
        gn, _ = nxt.elem_groups()
        ch = ms[-1].child_elems()
        for e in (0, ms[-1].nel // 2, ms[-1].nel - 1):
            kids = ch[e][ch[e] >= 0]
            assert np.all(gn[kids] == g[e])
        ms.append(nxt)
    assert [x.nel for x in ms] == [98, 392, 1568, 6272, 1280 * 4 + 4992, 5120 * 4 + 4992]
    assert ms[3].elem_levels()[1] and not ms[4].elem_levels()[1] and not ms[5].elem_levels()[1]
    assert capi.Mesh.box(2, 1, 0).elem_groups()[0].tolist() == [1, 1]


def test_hanging_node_map_on_the_selective_levels_of_the_known_answer_mesh():
    """the two non-homogeneous levels of unittests/testNSSteadyDD (curved elements around the cylinder): the library's hanging-node constraints
    (Mesh::GetAMRRestrictionAndAMRSolidMark as fh_mesh_amr_constraints restates it) against the oracle's independent restatement, node by node"""
    import os
    from oracle import femus_oracle as fo
    from oracle import femus_oracle_amr as fa
    ms = [capi.Mesh.read_gambit(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nsbenc.neu"))]
    for l in range(1, 6):
        g, _ = ms[-1].elem_groups()
        lev, _ = ms[-1].elem_levels()
        ms.append(ms[-1].refine_flagged(np.ones(ms[-1].nel, np.uint8) if l < 4 else ((g == 5) & (lev == ms[-1].level)).astype(np.uint8)))
    for l in (4, 5):
        m = ms[l]
        ed, xy, ff = m.arrays()
        mo = fo.Mesh("quad", ed, xy, ff, level=l)
        mo.elem_level = m.elem_levels()[0].astype(np.int64)
        for fe in ("biquadratic", "linear"):
            hang, ptr, master, w = m.amr_constraints(fe)
            R = fa.amr_restriction(mo, fe)
            assert hang.size > 0 and sorted(R) == hang.tolist()
            for i, h in enumerate(hang):
                got = dict(zip(master[ptr[i]:ptr[i + 1]].tolist(), w[ptr[i]:ptr[i + 1]].tolist()))
                want = {k: v for k, v in R[int(h)].items() if k != int(h)}
                got = {k: v for k, v in got.items() if k != int(h)}
                assert set(got) == set(want), (l, fe, int(h))
                assert max(abs(got[k] - want[k]) for k in want) <= 1e-12
