"""capi.ElementMesh.prolongator / boundary_dofs (fh_elem_mesh_prolongator, fh_elem_mesh_boundary_dofs; femus_amd/csrc/fh_elemtransfer.hip): the transfer of a
resident element mesh and its boundary lists, built on the device, against the host builder app_poisson._prolongator_from_children (pinned to its rule by
tests/test_element_transfer_host.py) and the face loop of run_elements -- integers equal, values equal as bits.  Host matrices are computed once per (mesh,
family, level) and shared, read-only."""
import itertools
import os

import numpy as np
import pytest

import femus_amd
from femus_amd import app_poisson as app
from femus_amd import capi, mixed_mesh
from test_element_transfer_host import FAM, FAMILIES, host_prolongator, host_transfer
from test_gpu_element_mesh import MESHES, MIXED_CUBE, host_chain

pytestmark = pytest.mark.gpu
OPTION, DEFAULT_CAP = "elem_transfer_lds_rows", 1024


def resident_chain(ctx, mesh, n=2):
    dev = [capi.ElementMesh.from_arrays(ctx, *mesh)]
    for _ in range(n):
        dev.append(dev[-1].refine())
    return dev


def destroy(*things):
    for t in things:
        for m in (t if isinstance(t, (list, tuple)) else [t]):
            m.destroy()


def csr(P):
    rp, col = P.pattern()
    return rp.astype(np.int64), col.astype(np.int64), P.values()


def same_bits(got, want):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), "rowptr"
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), "col"
    assert got[2].shape == want[2].shape and np.array_equal(np.ascontiguousarray(got[2]).view(np.uint64), np.ascontiguousarray(want[2]).view(np.uint64)), "val"


def device_transfer(coarse, fine, fe):
    P = coarse.prolongator(fine, fe)
    assert (P.m_, P.n_) == (fine.own[FAM[fe]], coarse.own[FAM[fe]])
    out = csr(P)
    P.destroy()
    return out


# ---- 1. bits ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_the_device_transfer_has_the_host_builder_s_bits(ctx, name):
    """the seven meshes as read x three families x levels 0 -> 1 and 1 -> 2"""
    dev = resident_chain(ctx, host_chain(name, False)[0])
    try:
        for fe in FAMILIES:
            for level in (0, 1):
                same_bits(device_transfer(dev[level], dev[level + 1], fe), host_transfer(name, fe, level))
    finally:
        destroy(dev)


# ---- 2. high valence -------------------------------------------------------------------------------------------------------------------------------------
def fan(n=64):
    """n TRI6 elements around one vertex, as mixed_mesh holds a mesh (the recipe of mixed_mesh.tri_box): vertex 0 the centre, 1 .. n the ring, then the middles
    of the spokes, of the rim, and the elements' centres; the rim carries flag -2"""
    ang = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    nxt = (np.arange(n) + 1) % n
    xy = np.concatenate([np.zeros((1, 2)), ring, 0.5 * ring, 0.5 * (ring + ring[nxt])])
    raw = np.full((n, 27), -1, dtype=np.int64)
    e = np.arange(n)
    raw[:, 0], raw[:, 1], raw[:, 2] = 0, 1 + e, 1 + nxt
    raw[:, 3], raw[:, 4], raw[:, 5] = 1 + n + e, 1 + 2 * n + e, 1 + n + nxt
    raw[:, 6] = xy.shape[0] + e
    centres = np.zeros((n, 2))
    for i in range(6):
        centres += xy[raw[:, i]] * mixed_mesh.ADDED["tri"][0][i]
    coords = np.concatenate([xy, centres])
    new, own = mixed_mesh._renumber(np.full(n, mixed_mesh.SHAPES.index("tri")), raw, coords.shape[0])
    xs = np.empty_like(coords)
    xs[new] = coords
    ff = np.full((n, 6), -1, dtype=np.int64)
    ff[:, 1] = -2
    return np.full(n, "tri"), mixed_mesh._apply(new, raw), xs, ff, own


@pytest.fixture(scope="module")
def fan_levels():
    chain = [fan()]
    for _ in range(2):
        chain.append(mixed_mesh.refine(*chain[-1][:4]))
    return chain


@pytest.mark.parametrize("cap", [DEFAULT_CAP, 27, 0], ids=["default", "one_element", "no_lds"])
def test_a_vertex_of_64_triangles(ctx, fan_levels, cap):
    """the centre of the fan sits in 64 fine elements: 64 x 27 slots, 64 x 7 biquadratic candidates -- beyond the wave's LDS at the default capacity.  With the
    capacity at 27 slots only the rows of one element (centres, middles on the rim) stay in LDS: an ordinary vertex of six triangles has 6 x 27 slots, a middle
    of two 2 x 27; at 0 none does.  Every setting gives the host's bits"""
    lv1, lv2 = fan_levels[1], fan_levels[2]
    centre = int(np.nonzero((lv2[2] == 0.0).all(axis=1))[0][0])
    assert centre < lv2[4][0] and (lv1[2][centre] == 0.0).all()
    assert (lv2[1][:, :3] == centre).sum() == 64 and lv2[0].shape[0] == 1024
    dev = resident_chain(ctx, fan_levels[0])
    ctx.set_option(OPTION, cap)
    try:
        for fe in FAMILIES:
            want = host_prolongator(fe, lv1, lv2)
            if fe == "biquadratic":
                n_elems = np.bincount(lv2[1][:, :7].ravel(), minlength=lv2[4][2])
                assert n_elems[centre] * 27 > DEFAULT_CAP and (n_elems * 27 > 27).sum() > 0.4 * n_elems.size
            same_bits(device_transfer(dev[1], dev[2], fe), want)
            same_bits(device_transfer(dev[0], dev[1], fe), host_prolongator(fe, fan_levels[0], lv1))
    finally:
        ctx.set_option(OPTION, DEFAULT_CAP)
        destroy(dev)


# ---- 3. order independence -------------------------------------------------------------------------------------------------------------------------------
def test_four_builds_are_identical_one_of_them_poisoned(ctx):
    dev = resident_chain(ctx, host_chain(MIXED_CUBE, False)[0])
    want = host_transfer(MIXED_CUBE, "biquadratic", 1)
    try:
        for _ in range(3):
            same_bits(device_transfer(dev[1], dev[2], "biquadratic"), want)
        ctx.set_option("debug_poison", 1)
        same_bits(device_transfer(dev[1], dev[2], "biquadratic"), want)
        ctx.set_option(OPTION, 27)                        # and the workgroup path's scratch
        same_bits(device_transfer(dev[1], dev[2], "biquadratic"), want)
    finally:
        ctx.set_option(OPTION, DEFAULT_CAP)
        ctx.set_option("debug_poison", int(os.environ.get("FEMUS_HIP_POISON", "0")))      # what a context starts with
        destroy(dev)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, call, words):
    with pytest.raises(capi.FemusHipError) as err:
        call()
    assert words in str(err.value), str(err.value)
    dev = resident_chain(ctx, host_chain("tri2.neu", False)[0], 1)              # and the context goes on working
    try:
        same_bits(device_transfer(dev[0], dev[1], "biquadratic"), host_transfer("tri2.neu", "biquadratic", 0))
    finally:
        destroy(dev)


def test_refusals(ctx):
    sq = host_chain("square_mixed.neu", False)[0]
    dev = resident_chain(ctx, sq)
    perm = np.random.default_rng(7).permutation(sq[0].shape[0])
    assert not np.array_equal(sq[0][perm], sq[0])
    other = resident_chain(ctx, (sq[0][perm], sq[1][perm], sq[2], sq[3][perm], sq[4]), 1)           # the same shapes in another order
    tris = resident_chain(ctx, mixed_mesh.tri_box(1, 3, (0, 0), (1, 1)), 1)                            # 6 -> 24 elements, triangles alone
    assert tris[1].nel == other[1].nel == dev[1].nel == 24
    ctx2 = femus_amd.Context(0)
    dev2 = resident_chain(ctx2, sq, 1)
    try:
        _refused(ctx, lambda: dev[0].prolongator(dev[1], 3), "fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic)")
        _refused(ctx, lambda: dev[0].prolongator(dev[2], "biquadratic"), "not its refinement")
        _refused(ctx, lambda: dev[1].prolongator(dev[0], "biquadratic"), "not its refinement")
        _refused(ctx, lambda: dev[0].prolongator(tris[1], "biquadratic"), "are not the children of")
        _refused(ctx, lambda: dev[0].prolongator(other[1], "biquadratic"), "not its refinement")
        _refused(ctx, lambda: dev[0].prolongator(dev2[1], "biquadratic"), "different contexts")
        _refused(ctx, lambda: dev[0].boundary_dofs(3, [-2]), "fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic)")
    finally:
        destroy(dev, other, tris, dev2)
        ctx2.close()


# ---- 5. boundary dofs ------------------------------------------------------------------------------------------------------------------------------------
def host_boundary_sets(level, fe):
    """flag -> the dofs the face loop of run_elements visits on the faces of that flag"""
    kind, ed, _, ff, _ = level
    fn_by = {s: [capi.fe_face_nodes(s, fe, f) for f in range(mixed_mesh.NFACES[s])] for s in sorted(set(kind.tolist()))}
    out = {}
    for iel, f in zip(*np.nonzero(ff < -1)):
        out.setdefault(int(ff[iel, f]), set()).update(int(d) for d in ed[iel, fn_by[kind[iel]][f]])
    return out


@pytest.mark.parametrize("name", MESHES)
def test_boundary_dofs(ctx, name):
    chain = host_chain(name, False)
    flags = sorted({int(f) for f in np.unique(chain[0][3]) if f < -1})
    subsets = list(itertools.islice((c for r in range(1, len(flags) + 1) for c in itertools.combinations(flags, r)), 15))
    assert flags and subsets
    dev = resident_chain(ctx, chain[0])
    try:
        for level, m in zip(chain, dev):
            for fe in FAMILIES:
                by_flag = host_boundary_sets(level, fe)
                assert sorted(by_flag) == flags and all(max(s) < level[4][FAM[fe]] for s in by_flag.values())
                for sub in subsets:
                    got = m.boundary_dofs(fe, sub)
                    want = np.array(sorted(set().union(*(by_flag[f] for f in sub))), dtype=np.int32)
                    assert got.dtype == np.int32 and np.array_equal(got, want), (level[0].shape[0], fe, sub)
                assert m.boundary_dofs(fe, []).size == 0
                assert m.boundary_dofs(fe, [-1000]).size == 0              # a flag no face carries
    finally:
        destroy(dev)


# ---- 6. the matrix is a full citizen ---------------------------------------------------------------------------------------------------------------------
class _Ctx:
    def __init__(self, ctx):
        self.ctx = ctx


def test_the_device_built_transfer_in_the_galerkin_chain(ctx):
    """mat_zero_rows, zero_cols and ptap on the device-built P give the bits they give on the host-built one; a second ptap_numeric after another zero_cols
    follows the edit (the derived-state rule of tests/test_gpu_state_sequences.py)"""
    chain = host_chain(MIXED_CUBE, False)
    fe, fam = "biquadratic", 2
    dev = resident_chain(ctx, chain[0], 1)
    flags = sorted({int(f) for f in np.unique(chain[0][3]) if f < -1 and f != -4})
    bd_c, bd_f = dev[0].boundary_dofs(fe, flags), dev[1].boundary_dofs(fe, flags)
    assert bd_c.size and bd_f.size
    kind, ed = chain[1][0], chain[1][1]
    eds = [ed[kind == s][:, :mixed_mesh.CLASSES[s][fam]] for s in sorted(set(kind.tolist()))]
    more = np.setdiff1d(np.arange(chain[0][4][fam], dtype=np.int32), bd_c)[::3]
    results = []
    for P in (dev[0].prolongator(dev[1], fe), capi.Mat.from_csr(ctx, chain[1][4][fam], chain[0][4][fam], *host_transfer(MIXED_CUBE, fe, 0))):
        K = app.Poisson001._pattern_from_elements(_Ctx(ctx), eds, chain[1][4][fam])
        K.set_values(np.random.default_rng(3).uniform(0.5, 1.5, K.nnz))
        P.mat_zero_rows(bd_f, 0.0)
        P.zero_cols(bd_c)
        A = capi.Mat.ptap(P, K)
        first = csr(P), csr(A)
        P.zero_cols(more)
        A.ptap_numeric(P, K)
        results.append(first + (csr(P), csr(A)))
        destroy(A, K, P)
    destroy(dev)
    d, h = results
    for a, b in zip(d, h):
        same_bits(a, b)
    assert not np.array_equal(d[1][2], d[3][2])               # the second product saw the emptied columns
    cols = np.zeros(chain[0][4][fam], bool)
    cols[more] = True
    cols[bd_c] = True
    rp, col, val = d[3]
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    assert np.all(val[cols[col] | cols[rows]] == 0.0) and np.any(val != 0.0)


# ---- 7. the application ----------------------------------------------------------------------------------------------------------------------------------
def _tet(tmp_path):
    from test_tet_3d import MESH, _shipped
    return _shipped("second", 2), MESH


def _mixed(tmp_path):
    from test_mixed_3d import MESH, _shipped
    return _shipped("second", 2), MESH


def _tri(tmp_path):
    from test_tri_2d import TRI_INPUT
    cfg = app.load_config(TRI_INPUT)
    cfg["multilevel_problem"]["multilevel_mesh"]["first"]["system"]["poisson"]["linear_solver"]["type"]["multigrid"]["nlevels"] = 2
    return cfg, None


@pytest.mark.parametrize("case", [_tet, _mixed, _tri], ids=["input3D_Tet_second", "input3D", "tri6_box"])
def test_the_application_with_device_and_host_transfers(ctx, tmp_path, case):
    cfg, mesh = case(tmp_path)
    if mesh is not None:
        os.makedirs(tmp_path / "input")
        (tmp_path / "input" / os.path.basename(mesh)).write_bytes(open(mesh, "rb").read())
    p = app.Poisson001(ctx, cfg, base_dir=str(tmp_path))
    assert p.nlevels == 2 and p.fe == "biquadratic" and p.geom is not None
    out = {t: p.run_elements(transfers=t) for t in ("device", "host")}
    with pytest.raises(ValueError):
        p.run_elements(transfers="somewhere")
    p.destroy()
    d, h = out["device"], out["host"]
    assert d["converged"] and len(d["history"]) > 1
    assert [k for k, _ in d["history"]] == [k for k, _ in h["history"]]
    assert np.array_equal(np.array([r for _, r in d["history"]]).view(np.uint64), np.array([r for _, r in h["history"]]).view(np.uint64))
    assert np.array_equal(d["solution"].view(np.uint64), h["solution"].view(np.uint64))
