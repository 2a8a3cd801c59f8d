"""capi.ElementMesh (fh_elem_mesh_*): the device-resident element mesh of any mix of hexahedra, tetrahedra, prisms, quadrilaterals and triangles, and its uniform
refinement on the device, against the product-side oracle femus_amd/mixed_mesh.py: refine -- integers equal, coordinates equal as bits.  The meshes are the
files of tests/golden and the TRI6 box, as read and with their level-0 nodes moved (curved elements: then WHICH child writes a shared node's coordinates shows
in the last bits).  The host chains are computed once per mesh and shared, read-only."""
import functools
import os

import numpy as np
import pytest

from femus_amd import capi, mixed_mesh

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILES = ["cube_Tet.neu", "cube_Wedge.neu", "cube_all_shapes_Six_boundary_groups.neu", "square_mixed.neu", "tri2.neu", "triAMR.neu"]
MESHES = FILES + ["tri_box"]
THREE_D = FILES[:3]
MIXED_CUBE = "cube_all_shapes_Six_boundary_groups.neu"
NEL = {"cube_Tet.neu": (105, 840, 6720), "cube_Wedge.neu": (16, 128, 1024), MIXED_CUBE: (20, 160, 1280), "square_mixed.neu": (6, 24, 96), "tri2.neu": (2, 8, 32),
       "triAMR.neu": (8, 32, 128), "tri_box": (12, 48, 192)}


def _frozen(mesh):
    for a in mesh[:4]:
        a.setflags(write=False)
    return mesh[:4] + (list(mesh[4]),)


@functools.lru_cache(maxsize=None)
def coarse(name, distorted):
    kind, ed, xs, ff, own = mixed_mesh.tri_box(2, 3, (0, 0), (1, 1)) if name == "tri_box" else mixed_mesh.read_gambit(os.path.join(HERE, "golden", name))
    if distorted:
        xs = xs + 0.03 * np.random.default_rng(1).uniform(-1, 1, xs.shape)
    return _frozen((kind, ed, xs, ff, own))


def host_chain_of(mesh, n=2):
    out = [mesh]
    for _ in range(n):
        out.append(_frozen(mixed_mesh.refine(*out[-1][:4])))
    return out


@functools.lru_cache(maxsize=None)
def host_chain(name, distorted):
    return host_chain_of(coarse(name, distorted))


def same(a, b):
    """two (kind, ed, xs, ff, own): names, integers (padding included) and class ends equal, coordinates equal as bits"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert a[1].shape[1:] == (27,) and a[3].shape[1:] == (6,)
    assert list(a[4]) == list(b[4])
    assert a[2].shape == b[2].shape and np.array_equal(np.ascontiguousarray(a[2]).view(np.int64), np.ascontiguousarray(b[2]).view(np.int64))


def device_chain(ctx, mesh, n=2):
    """[level 0 .. n] downloaded from a chain of resident meshes; nothing goes up after level 0"""
    dev = [capi.ElementMesh.from_arrays(ctx, *mesh)]
    try:
        for _ in range(n):
            dev.append(dev[-1].refine())
        out = [m.arrays() for m in dev]
        info = [(m.nel, m.nnode, m.dim, m.level, m.own) for m in dev]
    finally:
        for m in dev:
            m.destroy()
    return out, info


@pytest.mark.parametrize("distorted", [False, True], ids=["as_read", "distorted"])
@pytest.mark.parametrize("name", MESHES)
def test_two_device_refinements_equal_the_host_refiner(ctx, name, distorted):
    host = host_chain(name, distorted)
    assert tuple(lv[0].shape[0] for lv in host) == NEL[name] and all((lv[3] < -1).any() for lv in host)
    if name == "cube_Tet.neu":
        assert (host[1][3] < -1).sum() == 192
    dev, info = device_chain(ctx, host[0])
    for level, (h, d, (nel, nnode, dim, lev, own)) in enumerate(zip(host, dev, info)):
        same(d, h)
        assert (nel, nnode, dim, lev, own) == (h[0].shape[0], h[2].shape[0], h[2].shape[1], level, list(h[4]))
        assert d[1].dtype == np.int64 and d[3].dtype == np.int64 and d[2].dtype == np.float64


@pytest.mark.parametrize("name", THREE_D)
def test_the_coordinate_comparison_tells_the_creating_child(name):
    """control on the oracle alone: refined with its coarse elements in reversed order, a distorted three-dimensional mesh gets other last bits in some
    of its nodes -- other children create them -- so a kernel that lets the wrong child write a node's coordinates fails the test above"""
    kind, ed, xs, ff, _ = coarse(name, True)
    rows = lambda x: set(map(bytes, np.ascontiguousarray(x)))
    a, b = rows(mixed_mesh.refine(kind, ed, xs, ff)[2]), rows(mixed_mesh.refine(kind[::-1], ed[::-1], xs, ff[::-1])[2])
    print("%s: %d of %d coordinate rows differ in bits" % (name, len(a - b), len(a)))
    assert len(a) == len(b) and len(a - b) > 0


@pytest.mark.parametrize("name", [MIXED_CUBE, "square_mixed.neu"])
def test_shapes_interleaved(ctx, name):
    kind, ed, xs, ff, own = coarse(name, True)
    perm = np.random.default_rng(7).permutation(kind.shape[0])
    kp = kind[perm]
    assert (kp[1:] != kp[:-1]).sum() > (kind[1:] != kind[:-1]).sum()             # the shapes alternate
    mesh = (kp, ed[perm], xs, ff[perm], own)
    for h, d in zip(host_chain_of(mesh), device_chain(ctx, mesh)[0]):
        same(d, h)


def test_hexahedra_alone_through_this_path(ctx):
    """the hexahedra of the mixed cube with the node ids they have there (nodes of the other shapes stay, unused); against mixed_mesh.refine, whose sums run in
    local-node order (the hex path of fh_mesh_t adds in another order and is no yardstick here)"""
    kind, ed, xs, ff, own = coarse(MIXED_CUBE, True)
    sel = kind == "hex"
    assert 0 < sel.sum() < kind.shape[0]
    mesh = (kind[sel], ed[sel], xs, ff[sel], own)
    for h, d in zip(host_chain_of(mesh), device_chain(ctx, mesh)[0]):
        same(d, h)


@pytest.mark.parametrize("name", [MIXED_CUBE, "cube_Tet.neu", "square_mixed.neu"])
def test_three_refinements_of_one_resident_mesh_are_identical(ctx, name):
    """slot numbers depend on the race between the threads; ids, flags and coordinates must not"""
    host = host_chain(name, True)
    c = capi.ElementMesh.from_arrays(ctx, *host[1])
    got = []
    for _ in range(3):
        f = c.refine()
        got.append(f.arrays())
        f.destroy()
    c.destroy()
    for g in got:
        same(g, host[2])


@pytest.mark.parametrize("name", [MIXED_CUBE, "triAMR.neu"])
def test_residency(ctx, name):
    host = host_chain(name, True)
    chained = device_chain(ctx, host[0])[0][2]
    up = capi.ElementMesh.from_arrays(ctx, *host[1])
    assert up.level == 0
    f = up.refine()
    same(f.arrays(), chained)
    f.destroy()
    again = up.refine()                          # the coarse mesh is unchanged by a refinement and by the end of its fine mesh
    same(again.arrays(), chained)
    same(up.arrays(), host[1])
    again.destroy()
    up.destroy()


def _copy(name):
    m = coarse(name, False)
    return [np.array(a) for a in m[:4]] + [m[4]]


def _bad(what):
    kind, ed, xs, ff, own = _copy("cube_Tet.neu")
    if what == "line":
        kind = kind.astype("<U5")
        kind[3] = "line"
    elif what == "tet_in_2d":
        kind, ed, xs, ff, own = _copy("square_mixed.neu")
        kind = kind.astype("<U5")
        kind[2] = "tet"
    elif what == "id_nnode":
        ed[5, 7] = xs.shape[0]
    elif what == "minus_one_inside":
        ed[9, 14] = -1
    elif what == "dim_1":
        xs = xs[:, :1]
    return kind, ed, xs, ff, own


@pytest.mark.parametrize("what,words", [("line", "line"), ("tet_in_2d", "3-dimensional in a 2-dimensional"), ("id_nnode", "outside [0, "), ("minus_one_inside", "outside [0, "),
                                        ("dim_1", "dim must be 2 or 3")])
def test_refusals(ctx, what, words):
    with pytest.raises(capi.FemusHipError) as err:
        capi.ElementMesh.from_arrays(ctx, *_bad(what))
    assert words in str(err.value), str(err.value)
    # and the context goes on working
    host = host_chain("tri2.neu", False)
    same(device_chain(ctx, host[0], 1)[0][1], host[1])


def test_the_application_refines_on_the_device(ctx, tmp_path, monkeypatch):
    """Poisson001 on input3D_Tet_first.json (four levels, as shipped): its levels are the host chain's, and it did not call the host refiner"""
    from femus_amd import app_poisson as app
    from test_tet_3d import MESH, _shipped
    chain = host_chain_of(mixed_mesh.read_gambit(MESH), 3)
    os.makedirs(tmp_path / "input")
    (tmp_path / "input" / "cube_Tet.neu").write_bytes(open(MESH, "rb").read())
    p = app.Poisson001(ctx, _shipped("first", 4), base_dir=str(tmp_path))

    def host_refiner(*a, **k):
        raise AssertionError("the application refined on the host")
    monkeypatch.setattr(mixed_mesh, "refine", host_refiner)
    out = p.run()
    monkeypatch.undo()
    assert out["converged"] and len(out["levels"]) == 4
    for (ed, xs, ff), h in zip(out["levels"], chain):
        assert np.array_equal(ed, h[1][:, :15]) and np.array_equal(ff, h[3][:, :4])
        assert np.array_equal(np.ascontiguousarray(xs).view(np.int64), h[2].view(np.int64))
    p.destroy()
