"""capi.ElementMesh.matrix / boundary_faces / boundary_owners and capi.GenericAssembler.from_mesh (femus_amd/csrc/fh_elemplan.hip): pattern, assembly plan and
boundary data made from the device copy of an element mesh, against what the host makes from the downloaded arrays -- app_poisson._pattern_from_elements,
capi.GenericAssembler on the arrays, mixed_mesh.boundary_faces / boundary_owners (pinned to the face loop by tests/test_element_boundary_host.py).  Integers
equal, values equal as bits.  Then Poisson001.run_elements(mesh_data="device") against mesh_data="host"."""
import os

import numpy as np
import pytest

import femus_amd
from femus_amd import app_poisson as app
from femus_amd import capi, mixed_mesh
from test_element_boundary_host import flag_subsets
from test_element_refine_flagged_host import EX4, flagged_chain
from test_element_transfer_host import FAM, FAMILIES
from test_gpu_element_constraints import EX4_CONFIG
from test_gpu_element_mesh import MESHES, MIXED_CUBE, coarse, host_chain, host_chain_of
from test_gpu_element_mesh_flagged import resident_flagged_chain
from test_gpu_element_transfer import _mixed, _tet, _tri, destroy, fan, resident_chain
from test_gpu_generic_assembler import SOURCE, args_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PE_CAP = 1024                                     # candidate columns one wave of the pattern builder sorts


class _Ctx:
    def __init__(self, ctx):
        self.ctx = ctx


def host_pattern(ctx, level, fe):
    """the Mat of _pattern_from_elements on a downloaded level, its groups as run_elements makes them"""
    kind, ed, fam = level[0], level[1], FAM[fe]
    eds = [ed[kind == s][:, :mixed_mesh.CLASSES[s][fam]] for s in sorted(set(kind.tolist()))]
    return app.Poisson001._pattern_from_elements(_Ctx(ctx), eds, level[4][fam])


def pattern_of(K):
    rp, col = K.pattern()
    return rp.astype(np.int64), col.astype(np.int64)


def same_pattern(ctx, m, level, fe):
    Kd, Kh = m.matrix(fe), host_pattern(ctx, level, fe)
    try:
        n = level[4][FAM[fe]]
        assert (Kd.m_, Kd.n_) == (n, n)
        d, h = pattern_of(Kd), pattern_of(Kh)
        assert d[0].shape == h[0].shape and np.array_equal(d[0], h[0]), "rowptr"
        assert d[1].shape == h[1].shape and np.array_equal(d[1], h[1]), "col"
    finally:
        destroy(Kd, Kh)


def fan_chain(n, levels):
    chain = [fan(n)]
    for _ in range(levels):
        chain.append(mixed_mesh.refine(*chain[-1][:4]))
    return chain


# ---- 1. pattern ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_the_pattern_of_the_resident_level_is_the_host_s(ctx, name):
    chain = host_chain(name, False)
    dev = resident_chain(ctx, chain[0])
    try:
        for level in (1, 2):
            for fe in FAMILIES:
                same_pattern(ctx, dev[level], chain[level], fe)
    finally:
        destroy(dev)


@pytest.mark.parametrize("n,levels", [(64, 2), (160, 1)], ids=["centre_in_64", "beyond_the_wave"])
def test_the_pattern_around_a_vertex_of_many_triangles(ctx, n, levels):
    """the centre of the fan sits in n elements of 7 biquadratic dofs: 448 candidate columns, and with n = 160 the 1120 that the wave's LDS does not hold -- the
    builder's host path, which fetches the device table"""
    chain = fan_chain(n, levels)
    top = chain[-1]
    centre = int(np.nonzero((top[2] == 0.0).all(axis=1))[0][0])
    assert (top[1][:, :3] == centre).sum() == n and ((n * 7 > PE_CAP) == (n == 160))
    dev = resident_chain(ctx, chain[0], levels)
    try:
        same_pattern(ctx, dev[-1], top, "biquadratic")
    finally:
        destroy(dev)


# ---- 2. - 4. the plan ------------------------------------------------------------------------------------------------------------------------------------
def _permuted_cube():
    kind, ed, xs, ff, own = coarse(MIXED_CUBE, True)
    perm = np.random.default_rng(7).permutation(kind.shape[0])             # the permutation of test_gpu_element_mesh.py::test_shapes_interleaved
    assert (kind[perm][1:] != kind[perm][:-1]).sum() > (kind[1:] != kind[:-1]).sum()
    return kind[perm], ed[perm], xs, ff[perm], own


def plan_case(ctx, case):
    """(resident mesh, the same level on the host, everything to destroy) -- level-0 nodes distorted"""
    if case == "flagged_triAMR":
        chain = flagged_chain("triAMR.neu", True)
        dev = resident_flagged_chain(ctx, chain)
        assert not dev[2].homogeneous
        return dev[2], chain[2][:5], dev
    if case == "fan":
        chain = fan_chain(64, 1)
        dev = resident_chain(ctx, chain[0], 1)
        return dev[1], chain[1], dev
    mesh = _permuted_cube() if case == "mixed_cube_permuted" else coarse({"mixed_cube": MIXED_CUBE}.get(case, case), True)
    chain = host_chain_of(mesh, 1)
    dev = resident_chain(ctx, chain[0], 1)
    return dev[1], chain[1], dev


PLAN_CASES = ["mixed_cube", "mixed_cube_permuted", "square_mixed.neu", "cube_Tet.neu", "flagged_triAMR", "fan"]


def host_plan(ctx, level, fe, K):
    geom, ed = args_of(level[0], level[1])
    return capi.GenericAssembler(ctx, geom, fe, ed, level[2], K)


def same_plan(a, b):
    assert len(a) == len(b) == 3
    for x, y, what in zip(a, b, ("adj_ptr", "adj", "pos")):
        assert x.dtype == y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), what


@pytest.mark.parametrize("case", PLAN_CASES)
def test_the_plan_and_the_assembly_from_the_resident_mesh_are_the_host_s(ctx, case):
    m, level, dev = plan_case(ctx, case)
    kind = level[0]
    if case.startswith("mixed_cube"):
        assert len(set(kind.tolist())) == 3
        first = list(dict.fromkeys(kind.tolist()))
        assert (first != sorted(first)) or case == "mixed_cube"
    f = capi.Expr(SOURCE[level[2].shape[1]][0], "x,y,z,t")
    try:
        for fe in FAMILIES:
            n = level[4][FAM[fe]]
            Kd, Kh = m.matrix(fe), host_pattern(ctx, level, fe)
            gd, gh = capi.GenericAssembler.from_mesh(m, fe, Kd), host_plan(ctx, level, fe, Kh)
            try:
                same_plan(gd.plan(), gh.plan())
                if case == "mixed_cube_permuted":                 # rows of a dof ascend by element, which is not by id where shapes interleave
                    ptr, adj, _ = gd.plan()
                    assert any(np.any(np.diff(adj[ptr[d]:ptr[d + 1]]) < 0) for d in range(n))
                id_, ih = gd.info(), gh.info()
                assert id_["elems_per_workgroup"] == ih["elems_per_workgroup"] and id_["algorithmic_bytes"] == ih["algorithmic_bytes"]
                assert list(id_["elems_per_workgroup"]) == list(ih["elems_per_workgroup"])
                u = np.random.default_rng(11).uniform(-1, 1, n)
                SOL, Rd, Rh = ctx.vector_from(u), ctx.vector(n), ctx.vector(n)
                gd.assemble(Kd, Rd, sol=SOL, source=f)
                gh.assemble(Kh, Rh, sol=SOL, source=f)
                vd, vh = Kd.values(), Kh.values()
                assert np.abs(vh).max() > 0 and np.abs(Rh.to_numpy()).max() > 0
                assert np.array_equal(vd.view(np.uint64), vh.view(np.uint64)), "K"
                assert np.array_equal(Rd.to_numpy().view(np.uint64), Rh.to_numpy().view(np.uint64)), "RES"
                destroy(SOL, Rd, Rh)
            finally:
                destroy(gd, gh, Kd, Kh)
    finally:
        f.destroy()
        destroy(dev)


def test_four_builds_of_the_plan_are_identical_one_poisoned_and_the_mesh_may_go(ctx):
    m, level, dev = plan_case(ctx, "mixed_cube_permuted")
    fe, n = "biquadratic", level[4][2]
    K, Kh = m.matrix(fe), host_pattern(ctx, level, fe)
    gh = host_plan(ctx, level, fe, Kh)
    gens = []
    try:
        want = gh.plan()
        for k in range(4):
            ctx.set_option("debug_poison", 1 if k == 3 else int(os.environ.get("FEMUS_HIP_POISON", "0")))
            gens.append(capi.GenericAssembler.from_mesh(m, fe, K))
            same_plan(gens[-1].plan(), want)
        destroy(dev)                                              # the plan holds its own copy of the coordinates
        dev = []
        f = capi.Expr(SOURCE[3][0], "x,y,z,t")
        SOL, R, Rh = ctx.vector_from(np.random.default_rng(11).uniform(-1, 1, n)), ctx.vector(n), ctx.vector(n)
        gh.assemble(Kh, Rh, sol=SOL, source=f)
        want_bits = Kh.values().view(np.uint64).copy(), Rh.to_numpy().view(np.uint64).copy()
        for g in gens:                                            # the poisoned one last
            K.zero()
            g.assemble(K, R, sol=SOL, source=f)
            assert np.array_equal(K.values().view(np.uint64), want_bits[0]) and np.array_equal(R.to_numpy().view(np.uint64), want_bits[1])
        f.destroy()
        destroy(SOL, R, Rh)
    finally:
        ctx.set_option("debug_poison", int(os.environ.get("FEMUS_HIP_POISON", "0")))      # what a context starts with
        destroy(gens, gh, K, Kh, dev)


# ---- 5. boundary lists -----------------------------------------------------------------------------------------------------------------------------------
def same_boundary_lists(m, level, fe, sub):
    got, want = m.boundary_faces(fe, sub), mixed_mesh.boundary_faces(level, fe, sub)
    for g, w, what in zip(got, want, ("elem", "face", "nodes", "nn")):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, fe, sub)
    dofs, owner, xy = m.boundary_owners(fe, sub)
    wd, wo, wx = mixed_mesh.boundary_owners(level, fe, sub)
    assert dofs.dtype == owner.dtype == np.int32 and np.array_equal(dofs, wd) and np.array_equal(owner, wo), (fe, sub)
    assert xy.shape == wx.shape and np.array_equal(np.ascontiguousarray(xy).view(np.uint64), np.ascontiguousarray(wx).view(np.uint64)), (fe, sub)
    assert np.array_equal(dofs, m.boundary_dofs(fe, sub))
    return dofs.size


@pytest.mark.parametrize("name", MESHES)
def test_boundary_faces_and_owners(ctx, name):
    chain = host_chain(name, True)
    flags, subs = flag_subsets(chain[0])
    dev = resident_chain(ctx, chain[0])
    try:
        for level, m in zip(chain, dev):
            for fe in FAMILIES:
                sizes = [same_boundary_lists(m, level, fe, sub) for sub in subs]
                assert sizes[-1] == sizes[-2] == 0 and max(sizes) == sizes[-3] > 0          # (), a flag no face carries, all flags
    finally:
        destroy(dev)


def test_boundary_lists_of_a_flagged_level(ctx):
    chain = flagged_chain("triAMR.neu", True)
    flags, subs = flag_subsets(chain[0])
    dev = resident_flagged_chain(ctx, chain)
    try:
        for level, m in zip(chain[1:], dev[1:]):
            for fe in FAMILIES:
                for sub in subs:
                    same_boundary_lists(m, level[:5], fe, sub)
    finally:
        destroy(dev)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------------
def _refused(call, words):
    with pytest.raises(capi.FemusHipError) as err:
        call()
    assert words in str(err.value), str(err.value)


def test_refusals(ctx):
    m, level, dev = plan_case(ctx, "mixed_cube_permuted")
    kind, ed = level[0], level[1]
    K2, K0 = m.matrix(2), m.matrix(0)
    # the linear family's pattern on the biquadratic family's rows: every pair with a dof beyond the vertices is missing
    rp0, col0 = pattern_of(K0)
    n2 = level[4][2]
    rp = np.concatenate([rp0, np.full(n2 - K0.m_, rp0[-1])])
    Kmiss = capi.Mat.from_csr(ctx, n2, n2, rp, col0)
    ctx2 = femus_amd.Context(0)
    Kother = capi.Mat.from_csr(ctx2, n2, n2, *pattern_of(K2))
    try:
        _refused(lambda: capi.GenericAssembler.from_mesh(m, 3, K2), "fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic)")
        _refused(lambda: m.matrix(3), "fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic)")
        _refused(lambda: m.boundary_faces(3, [-2]), "fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic)")
        _refused(lambda: m.boundary_owners(-1, [-2]), "fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic)")
        _refused(lambda: capi.GenericAssembler.from_mesh(m, 2, K0), "it must be square of the %d dofs the family owns" % n2)
        _refused(lambda: capi.GenericAssembler.from_mesh(m, 2, Kother), "different contexts")
        # the miss: shapes in the order of their first elements, slots ascending, rows, then columns -- the first entry whose pair the pattern lacks
        shapes = list(dict.fromkeys(kind.tolist()))
        s0 = shapes[0]
        nc, nv = mixed_mesh.CLASSES[s0][2], mixed_mesh.CLASSES[s0][0]
        e = int(np.nonzero(kind == s0)[0][0])
        pairs = {(int(r), int(c)) for r in range(K0.m_) for c in col0[rp0[r]:rp0[r + 1]]}
        i, j = next((i, j) for i in range(nc) for j in range(nc) if (int(ed[e, i]), int(ed[e, j])) not in pairs)
        assert (i, j) == (0, nv)
        _refused(lambda: capi.GenericAssembler.from_mesh(m, 2, Kmiss),
                 "element %d: the pair (%d, %d) = dofs (%d, %d) is not in the pattern of the matrix" % (e, i, j, ed[e, i], ed[e, j]))
        g = capi.GenericAssembler.from_mesh(m, 2, K2)             # and everything goes on working
        g.destroy()
    finally:
        destroy(K2, K0, Kmiss, Kother, dev)
        ctx2.close()


# ---- 7. the application ----------------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _both_ways(p, monkeypatch, **kw):
    host = p.run_elements(mesh_data="host", **kw)
    with monkeypatch.context() as mp:
        def no_download(self):
            raise AssertionError("ElementMesh.arrays was called with mesh_data=\"device\"")
        mp.setattr(capi.ElementMesh, "arrays", no_download)
        dev = p.run_elements(mesh_data="device", **kw)
    assert "levels" in host and "levels" not in dev
    assert dev["converged"] and len(dev["history"]) > 1 and dev["dofs"] == host["dofs"]
    assert [k for k, _ in dev["history"]] == [k for k, _ in host["history"]]
    assert np.array_equal(_bits(np.array([r for _, r in dev["history"]])), _bits(np.array([r for _, r in host["history"]])))
    assert np.array_equal(_bits(dev["solution"]), _bits(host["solution"])) and np.array_equal(_bits(dev["coords"]), _bits(host["coords"]))
    assert set(dev) == set(host) - {"levels"}
    return dev, host


@pytest.mark.parametrize("case", [_tet, _mixed, _tri], ids=["input3D_Tet_second", "input3D", "tri6_box"])
def test_the_application_with_device_and_host_mesh_data(ctx, tmp_path, monkeypatch, case):
    cfg, mesh = case(tmp_path)
    if mesh is not None:
        os.makedirs(tmp_path / "input")
        (tmp_path / "input" / os.path.basename(mesh)).write_bytes(open(mesh, "rb").read())
    p = app.Poisson001(ctx, cfg, base_dir=str(tmp_path))
    try:
        assert p.nlevels == 2 and p.fe == "biquadratic" and p.geom is not None
        _both_ways(p, monkeypatch)
        with pytest.raises(ValueError):
            p.run_elements(mesh_data="device", transfers="host")
        with pytest.raises(ValueError):
            p.run_elements(mesh_data="somewhere")
    finally:
        p.destroy()


def test_the_application_on_a_flagged_level_with_device_mesh_data(ctx, tmp_path, monkeypatch):
    os.makedirs(tmp_path / "input")
    (tmp_path / "input" / "triAMR.neu").write_bytes(open(os.path.join(HERE, "golden", "triAMR.neu"), "rb").read())
    p = app.Poisson001(ctx, EX4_CONFIG, base_dir=str(tmp_path))
    try:
        dev, host = _both_ways(p, monkeypatch, selective_levels=1, flag=EX4)
    finally:
        p.destroy()
    assert dev["hanging"].size > 0 and np.array_equal(dev["hanging"], host["hanging"]) and np.array_equal(dev["elem_levels"], host["elem_levels"])
