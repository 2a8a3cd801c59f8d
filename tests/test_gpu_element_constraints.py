"""capi.ElementMesh.amr_constraints / amr_prolongator (fh_elem_mesh_amr_*): the hanging-node constraints of a resident flagged level, searched on the device, against
the host rule mixed_mesh.amr_constraints (tests/test_element_constraints_host.py) -- integers equal, weights to rounding (the kernels run the host's basis code
but may contract products and sums differently); then what the constraints are for: a patch test through P_amr, and Poisson001.run_elements on flagged levels.

Bounds.  Device against host weights: both Newton iterations stop below 1e-14 * scale, basis gradients O(10) -- 1e-12 as in the host test.  Patch test: the constrained
space holds the quadratic exactly and a direct solve of a few thousand unknowns leaves about 1e-13 -- 1e-10 max|u|.  The application: the residual stop is 1e-10 and the
smallest eigenvalue of these stiffness matrices (h about 1/8) a few tenths, which gives about 1e-9 -- 1e-8."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from femus_amd import app_poisson as app
from femus_amd import capi, mixed_mesh
from oracle import femus_oracle_mixed as fom
from test_element_constraints_host import FAMILIES3, MODES, constraints, warped_chain
from test_element_refine_flagged_host import EX4, flagged_chain, straight_chain
from test_element_transfer_host import FAM
from test_gpu_element_mesh import MESHES, MIXED_CUBE
from test_gpu_element_mesh_flagged import resident_flagged_chain
from test_gpu_element_transfer import destroy

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OPTION = "elem_constraints_host"


def same_lists(got, want, tol=1e-12):
    assert all(np.array_equal(got[k], want[k]) for k in range(3)), [(got[k].shape, want[k].shape) for k in range(3)]
    err = float(np.abs(got[3] - want[3]).max()) if want[3].size else 0.0
    assert err <= tol, err
    return err


def p_amr_of(c, n):
    """P_amr (n x n) from the lists: identity rows, a hanging dof's row = its masters plus an explicit zero on the diagonal"""
    hang, ptr, master, w = c
    regular = np.setdiff1d(np.arange(n), hang)
    rows = np.concatenate([regular, hang, np.repeat(hang, np.diff(ptr))])
    cols = np.concatenate([regular, hang, master])
    vals = np.concatenate([np.ones(regular.size), np.zeros(hang.size), w])
    P = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    P.sort_indices()
    return P


# ---- 5. device against the host rule ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["straight", "warped"])
@pytest.mark.parametrize("name", MESHES)
def test_the_device_search_equals_the_host_rule(ctx, name, geometry):
    chain = flagged_chain(name, False) if geometry == "straight" else warped_chain(name)
    dev = resident_flagged_chain(ctx, chain)
    try:
        for level in (1, 2):
            for fe in FAMILIES3:
                for mode in MODES:
                    want = constraints(chain[level], fe, mode)
                    err = same_lists(dev[level].amr_constraints(fe, mode), want)
                    print("%s %s level %d %s %s: %d hanging dofs, %d entries, max |w_device - w_host| = %.2e" % (name, geometry, level, fe, mode, want[0].size, want[2].size, err))
                    assert want[0].size > 0
    finally:
        destroy(dev)


# ---- 6. bitwise ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_the_search_repeats_its_bits_and_the_host_switch_agrees(ctx, name):
    chain = warped_chain(name)
    dev = resident_flagged_chain(ctx, chain)
    try:
        for mode in MODES:
            a = dev[2].amr_constraints("biquadratic", mode)
            b = dev[2].amr_constraints("biquadratic", mode)
            assert all(np.array_equal(a[k], b[k]) for k in range(3)) and np.array_equal(a[3].view(np.int64), b[3].view(np.int64))
            ctx.set_option(OPTION, 1)
            try:
                h = dev[2].amr_constraints("biquadratic", mode)
            finally:
                ctx.set_option(OPTION, 0)
            same_lists(a, h)
            same_lists(h, constraints(chain[2], "biquadratic", mode), 0.0)          # the switch runs the host rule itself
    finally:
        destroy(dev)


def test_the_search_under_poisoned_work_buffers(ctx):
    chain = flagged_chain(MIXED_CUBE, False)
    dev = resident_flagged_chain(ctx, chain)
    try:
        ctx.set_option("debug_poison", 1)
        same_lists(dev[2].amr_constraints("biquadratic", "coarsest"), constraints(chain[2], "biquadratic", "coarsest"))
    finally:
        ctx.set_option("debug_poison", int(os.environ.get("FEMUS_HIP_POISON", "0")))      # what a context starts with
        destroy(dev)


# ---- 7. P_amr ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["triAMR.neu", MIXED_CUBE])
def test_p_amr_is_the_matrix_of_the_lists(ctx, name):
    chain = flagged_chain(name, False)
    dev = resident_flagged_chain(ctx, chain)
    try:
        for fe in FAMILIES3:
            for mode in MODES:
                n = chain[2][4][FAM[fe]]
                c = dev[2].amr_constraints(fe, mode)
                P = dev[2].amr_prolongator(fe, mode)
                try:
                    got = P.to_scipy().tocsr()
                finally:
                    P.destroy()
                got.sort_indices()
                want = p_amr_of(c, n)
                assert got.shape == (n, n) and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
                assert np.array_equal(got.data.view(np.int64), want.data.view(np.int64))
                diag = got[c[0], c[0]]
                assert got.nnz == n + c[2].size and (np.asarray(diag).ravel() == 0.0).all()         # the zero diagonals are in the pattern
        # a homogeneous mesh: empty lists, the identity
        c = dev[0].amr_constraints("biquadratic")
        assert [a.size for a in c] == [0, 1, 0, 0]
        P = dev[0].amr_prolongator("biquadratic")
        try:
            I = P.to_scipy().tocsr()
        finally:
            P.destroy()
        n = chain[0][4][2]
        assert I.shape == (n, n) and I.nnz == n and np.array_equal(I.indices, np.arange(n)) and (I.data == 1.0).all()
    finally:
        destroy(dev)


def test_refusals(ctx):
    chain = flagged_chain("triAMR.neu", False)
    dev = resident_flagged_chain(ctx, chain)
    loose = capi.ElementMesh.from_arrays(ctx, *chain[1][:5])              # a flagged level from host arrays whose levels nobody set
    try:
        for call in (dev[1].amr_constraints, dev[1].amr_prolongator):
            with pytest.raises(capi.FemusHipError, match="fe must be 0"):
                call(3)
            with pytest.raises(capi.FemusHipError, match="mode must be"):
                call("biquadratic", "finest")
            with pytest.raises(capi.FemusHipError, match="mode must be 0"):
                n, nnz, h = capi.ctypes.c_int(0), capi.ctypes.c_int(0), capi.ctypes.c_void_p()
                if call == dev[1].amr_constraints:
                    capi._chk(ctx.L.fh_elem_mesh_amr_constraints(dev[1].h, 2, 2, capi.ctypes.byref(n), capi.ctypes.byref(nnz), None, None, None, None))
                else:
                    capi._chk(ctx.L.fh_elem_mesh_amr_prolongator(dev[1].h, 2, 2, capi.ctypes.byref(h)))
        with pytest.raises(capi.FemusHipError, match="levels of its elements were never set"):
            loose.amr_constraints("biquadratic")
        with pytest.raises(capi.FemusHipError, match="levels of its elements were never set"):
            loose.amr_prolongator("linear", "coarsest")
        loose.set_levels(chain[1][5])
        same_lists(loose.amr_constraints("biquadratic"), constraints(chain[1], "biquadratic", "reference"))
    finally:
        destroy(dev, loose)


# ---- 8. the patch test, direct -------------------------------------------------------------------------------------------------------------------------------------
def quadratic(x):
    """1 + 2x - y + x^2 - 3xy + 2y^2 (+ z^2 - xz); its Laplacian is 6 (8 in three dimensions)"""
    u = 1.0 + 2.0 * x[:, 0] - x[:, 1] + x[:, 0] ** 2 - 3.0 * x[:, 0] * x[:, 1] + 2.0 * x[:, 1] ** 2
    return u + (x[:, 2] ** 2 - x[:, 0] * x[:, 2] if x.shape[1] == 3 else 0.0)


def constrained_solve(K, b, P, fixed, values):
    """P^T K P U = P^T b with unit rows at `fixed` (U = values there), solved directly; P U"""
    A = (P.T @ K @ P).tolil()
    rhs = P.T @ b
    A[fixed, :] = 0.0
    A[fixed, fixed] = 1.0
    rhs[fixed] = values
    return P @ spla.splu(A.tocsc()).solve(rhs)


@pytest.mark.parametrize("name", ["triAMR.neu", "square_mixed.neu", "cube_Wedge.neu", MIXED_CUBE])
def test_the_constrained_space_holds_a_quadratic(ctx, name):
    """assembled with the fifth-order rules, which integrate every product of this test exactly (degree <= 4 on the simplices, <= 3 per direction on the tensor
    shapes).  NOT with the default "seventh": the reference's 31-point rule of the tetrahedron, kept digit for digit, sums to 1/6 - 1.07e-9
    (tests/test_element_constraints_host.py holds that figure), so a mesh with tetrahedra -- the mixed cube -- misses any patch test by about 1e-8 with it, refined
    uniformly or not: measured 2.3e-8 on this level, 3.7e-8 on the uniform level 1 through the oracle's own element loop, 3.8e-14 and 4.9e-15 with the fifth-order rules"""
    from test_gpu_generic_assembler import args_of, pattern
    chain = straight_chain(name)
    kind, ed, xs, ff, own = chain[2][:5]
    n, dim = own[2], xs.shape[1]
    dev = resident_flagged_chain(ctx, chain)
    things = []
    try:
        Pm = dev[2].amr_prolongator("biquadratic", "coarsest")
        things.append(Pm)
        hang = dev[2].amr_constraints("biquadratic", "coarsest")[0]
        boundary = dev[2].boundary_dofs("biquadratic", sorted(set(ff[ff < -1].tolist())))
        P = Pm.to_scipy().tocsr()
        K, _ = pattern(ctx, kind, ed, "biquadratic", n)
        things.append(K)
        RES = ctx.vector(n)
        geom, edw = args_of(kind, ed)
        f = capi.Expr("-6." if dim == 2 else "-8.", "x,y,z,t")            # f = -Laplace u, the sign of the generic assembler's residual f phi - grad phi . grad u
        things.append(f)
        gen = capi.GenericAssembler(ctx, geom, "biquadratic", edw, xs, K, order="fifth")
        things.append(gen)
        gen.assemble(K, RES, source=f)
        Kh, b = K.to_scipy().tocsr(), RES.to_numpy()
    finally:
        destroy(dev, things)
    u = quadratic(xs[:n])
    assert hang.size > 0 and boundary.size > 0 and n <= 20000
    fixed = np.union1d(boundary, hang)
    values = np.where(np.isin(fixed, boundary), u[fixed], 0.0)            # u on the boundary; a hanging dof (one on the boundary too: P overwrites it) is no unknown
    U = constrained_solve(Kh, b, P, fixed, values)
    err = np.abs(U - u).max()
    print("%s: %d dofs, %d hanging, max |U - u| = %.2e of max |u| = %.2e" % (name, n, hang.size, err, np.abs(u).max()))
    assert err <= 1e-10 * np.abs(u).max()


# ---- 9. the application on a box of triangles ------------------------------------------------------------------------------------------------------------------------
U2 = "1.+2.*x-y+x*x-3.*x*y+2.*y*y"
BOX_FLAG = "if(level<0.5, x>0.5, (x>0.5)&(y>0.5))"


def box_config():
    return {"multilevel_mesh": {"first": {"type": {"box": {"nx": 2, "ny": 3, "nz": 0, "xa": 0., "xb": 1., "ya": 0., "yb": 1., "za": 0., "zb": 0., "elem_type": "Tri6"}}}},
            "multilevel_solution": {"multilevel_mesh": {"first": {"variable": {"first": {
                "name": "T", "fe_order": "second", "init_func": "0.", "func_source": "-6.",
                "boundary_conditions": [{"facename": n, "bdc_type": "dirichlet", "bdc_func": U2} for n in ("left", "right", "top", "bottom")]}}}}},
            "multilevel_problem": {"multilevel_mesh": {"first": {"system": {"poisson": {"linear_solver": {
                "max_number_linear_iteration": 12, "abs_conv_tol": 1.e-10,
                "type": {"multigrid": {"nlevels": 3, "npresmoothing": 1, "npostsmoothing": 1, "mgtype": "V_cycle"}}}}}}}}}


@pytest.mark.parametrize("amr_mode", MODES)
def test_the_application_on_flagged_levels_of_a_box(ctx, amr_mode):
    p = app.Poisson001(ctx, box_config())
    try:
        assert p.nlevels == 3 and p.fe == "biquadratic" and p.geom == "tri"
        out = p.run_elements(selective_levels=2, flag=BOX_FLAG, amr_mode=amr_mode)
        plain, again = p.run_elements(selective_levels=0), p.run_elements()
        with pytest.raises(ValueError, match="transfers must be"):
            p.run_elements(transfers="host", selective_levels=2, flag=BOX_FLAG)
    finally:
        p.destroy()
    u = quadratic(out["coords"])
    err = np.abs(out["solution"] - u).max()
    print("flagged box, %s: %d dofs, %d hanging, history %s, max |T - u| = %.2e" % (amr_mode, out["dofs"], out["hanging"].size, out["history"], err))
    assert out["converged"] and out["hanging"].size > 0 and set(out["elem_levels"].tolist()) == {0, 1, 2}
    assert out["elem_levels"].shape == (out["levels"][-1][0].shape[0],)
    assert err <= 1e-8
    # without flagged levels nothing of this is touched: the keys and the bits of the call without the new arguments
    assert "hanging" not in plain and plain["converged"] and plain["dofs"] == 17 * 25 + 2 * 96
    assert np.array_equal(plain["solution"].view(np.uint64), again["solution"].view(np.uint64)) and plain["history"] == again["history"]
    assert np.abs(plain["solution"] - quadratic(plain["coords"])).max() <= 1e-8


# ---- 10. ex4 on triAMR.neu ---------------------------------------------------------------------------------------------------------------------------------------------
EX4_CONFIG = """
{
    "multilevel_mesh" : { "first" : { "type" : { "filename" : "input/triAMR.neu" } } },
    "multilevel_solution" : { "multilevel_mesh" : { "first" : { "variable" : { "first" : {
              "name" : "T", "fe_order" : "second", "init_func" : "0.", "func_source": "1." } } } } },
    "multilevel_problem" : { "multilevel_mesh" : { "first" : { "system" : { "poisson" : { "linear_solver" : {
                "max_number_linear_iteration" : 12, "abs_conv_tol" : 1.e-10,
                "type" : { "multigrid" : { "nlevels" : 3, "npresmoothing" : 1, "npostsmoothing" : 1, "mgtype" : "V_cycle" } } } } } } } }
}
"""


@pytest.mark.parametrize("amr_mode", MODES)
def test_ex4_on_triAMR(ctx, tmp_path, amr_mode):
    """applications/MGAMR/ex4's refinement rule on its mesh, with the boundary conditions this application gives a mesh file (Dirichlet 0, flux 0.2 on face name 3):
    the solution is the direct solve of the same constrained system, built from the oracle's element loop and the host rule's P_amr"""
    os.makedirs(tmp_path / "input")
    (tmp_path / "input" / "triAMR.neu").write_bytes(open(os.path.join(HERE, "golden", "triAMR.neu"), "rb").read())
    p = app.Poisson001(ctx, EX4_CONFIG, base_dir=str(tmp_path))
    try:
        assert p.nlevels == 3 and p.fe == "biquadratic" and p.geom == "mixed"
        out = p.run_elements(selective_levels=2, flag=EX4, amr_mode=amr_mode)
    finally:
        p.destroy()
    ed, xs, ff = out["levels"][-1]
    kind, lev, n = np.full(ed.shape[0], "tri"), out["elem_levels"], out["dofs"]
    top = flagged_chain("triAMR.neu", False)[2]                           # the chain the host rule refines with ex4 is this level
    assert np.array_equal(ed, top[1]) and np.array_equal(lev, top[5]) and np.array_equal(ff, top[3]) and n == xs.shape[0]
    c = mixed_mesh.amr_constraints(kind, ed, xs, ff, lev, "biquadratic", amr_mode)
    assert np.array_equal(out["hanging"], c[0]) and c[0].size == 14
    K, F = fom.assemble(kind, ed, xs, "biquadratic", lambda x: 1.0)
    F = F + fom.neumann(kind, ed, xs, ff, "biquadratic", {-4: 0.2}, n)
    fixed = np.union1d(fom.dirichlet(kind, ed, ff, "biquadratic", {-2, -3}), c[0])
    want = constrained_solve(sp.csr_matrix(K), F, p_amr_of(c, n), fixed, 0.0)
    err = np.abs(out["solution"] - want).max()
    print("ex4 on triAMR.neu, %s: %d dofs, history %s, max |T - direct| = %.2e of %.2e" % (amr_mode, n, out["history"], err, np.abs(want).max()))
    assert out["converged"] and np.abs(want).max() > 1e-3
    assert err <= 1e-8
