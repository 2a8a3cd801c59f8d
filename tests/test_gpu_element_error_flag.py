"""capi.ElementMesh.flag_by_error / error_indicators (fh_elem_mesh_error_flag, fh_elem_mesh_error_indicators): the flags of a resident element mesh from the error norm
of the last correction, against the host statement capi.error_flag_host -- the element body is one text compiled for both sides, so err_i, vol_i, the sums and the
flags are compared bit for bit -- and against the literal walk of tests/amr_flag_reference.py, on the cases of tests/amr_flag_cases.py; then the adaptive driver
Poisson001.run_elements_adaptive on the 2 x 2 box of triangles and on triAMR.neu.

Bounds.  Sums against the literal walk: 2 N 2^-53 relative, N the number of (element, Gauss point) terms, as in tests/test_element_error_flag_host.py (check_sums).
The driver against a direct solve: 1e-8, the bound tests/test_gpu_element_constraints.py derives for the residual stop 1e-10 on these stiffness matrices."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import amr_flag_cases as ac
from femus_amd import app_poisson as app
from femus_amd import capi, mixed_mesh
from oracle import femus_oracle_mixed as fom
from test_element_error_flag_host import REFUSALS, check_sums, host
from test_gpu_element_constraints import EX4_CONFIG, constrained_solve, p_amr_of
from test_gpu_element_mesh import same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def resident(ctx, m):
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    dev = capi.ElementMesh.from_arrays(ctx, kind, ed, xs, ac.faces_of(*m[:3]), own)
    if m[2] == "b":
        dev.set_levels(lev)
    assert dev.level == level
    return dev


def device(ctx, dev, m, fe, norm, neighbor_threshold, threshold=None):
    s, e = ac.vectors(m, fe)
    S, E = ctx.vector_from(s), ctx.vector_from(e)
    try:
        thr = ac.THRESHOLD[ac.case_id((m, fe, norm))] if threshold is None else threshold
        d = dev.flag_by_error(fe, S, E, thr, norm, neighbor_threshold, m[3])
        d["err2"], d["vol"] = dev.error_indicators(fe, E, norm, m[3])
        return d
    finally:
        S.destroy()
        E.destroy()


def same_result(d, h):
    """device against host, or a call against its repetition: everything bit for bit"""
    assert np.array_equal(d["flags"], h["flags"]) and d["nflagged"] == h["nflagged"] and d["converged"] == h["converged"]
    assert np.array_equal(bits(d["err2"]), bits(h["err2"])) and np.array_equal(bits(d["vol"]), bits(h["vol"]))
    assert np.array_equal(bits(d["sums"]), bits(h["sums"])) and np.array_equal(bits(d["threshold"]), bits(h["threshold"]))


def compare_case(ctx, m, fe, norm, neighbor_threshold):
    r = ac.reference(m, fe, norm, neighbor_threshold)
    ac.check_inputs(m, fe, norm, neighbor_threshold, r)
    h = host(m, fe, norm, neighbor_threshold)
    dev = resident(ctx, m)
    try:
        d = device(ctx, dev, m, fe, norm, neighbor_threshold)
        again = device(ctx, dev, m, fe, norm, neighbor_threshold)
    finally:
        dev.destroy()
    same_result(d, h)
    same_result(again, d)
    assert np.array_equal(d["flags"], r["flags"]) and d["nflagged"] == r["nflagged"] and d["converged"] == r["converged"]
    check_sums(d["sums"], r, 2 * r["nterms"] * 2.0 ** -53)


# ---- 1. - 3. device against host and the literal walk, twice --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neighbor_threshold", ac.NEIGHBOR)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_the_device_equals_the_host_statement_and_repeats_its_bits(ctx, case, neighbor_threshold):
    compare_case(ctx, case[0], case[1], case[2], neighbor_threshold)


def test_sums_over_more_than_one_chunk_and_level(ctx):
    """3976 elements: four chunks of the fixed-shape sum; the comparison above holds their bits.  Here: a mesh with one refinable element and a correction that
    is nowhere zero -- that element alone is flagged at threshold 0, and the indicators of the others are zero"""
    m = ac.MESHES[0]
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    assert ac.mesh_of(*ac.MESHES[6][:3])[0].shape[0] > 3 * 1024
    dev = resident(ctx, m)
    s, e = ac.vectors(m, 2)
    e = 1.0 + 0.25 * e
    S, E = ctx.vector_from(s), ctx.vector_from(e)
    try:
        dev.set_levels(np.where(np.arange(kind.shape[0]) == 0, 1, 0))                  # the mesh's level becomes 1: element 0 alone is refinable
        d = dev.flag_by_error(2, S, E, 0.0, "H1")
        h = capi.error_flag_host(kind, ed, xs, np.where(np.arange(kind.shape[0]) == 0, 1, 0), 1, 2, s, e, 0.0, "H1")
        assert d["flags"].tolist() == [1] + [0] * (kind.shape[0] - 1) == h["flags"].tolist() and np.array_equal(bits(d["sums"]), bits(h["sums"]))
        err2, vol = dev.error_indicators(2, E)
        assert not err2[1:].any() and not vol[1:].any() and err2[0] > 0 and vol[0] > 0
    finally:
        S.destroy()
        E.destroy()
        dev.destroy()


# ---- 4. refine("resident") after flag_by_error -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [ac.MESHES[3], ac.MESHES[8], ac.MESHES[-1]], ids=ac.mesh_id)
def test_the_flags_stay_on_the_device_for_the_refinement(ctx, m):
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    fe = m[4][-1]
    dev = capi.ElementMesh.from_arrays(ctx, kind, ed, xs, ac.faces_of(*m[:3]), own)
    s, e = ac.vectors(m, fe)
    S, E = ctx.vector_from(s), ctx.vector_from(e)
    fine = []
    try:
        if m[2] == "b":
            dev.set_levels(lev)
        d = dev.flag_by_error(fe, S, E, ac.THRESHOLD[ac.case_id((m, fe, "H1"))], "H1", 0.0, m[3])
        assert 0 < d["nflagged"] < kind.shape[0]
        fine = [dev.refine("resident"), dev.refine(d["flags"])]
        same(fine[0].arrays(), fine[1].arrays())
        a, b = fine[0].elem_levels(), fine[1].elem_levels()
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and (a[0] == level + 1).sum() == d["nflagged"] * (4 if xs.shape[1] == 2 else 8)
    finally:
        for q in fine + [dev, S, E]:
            q.destroy()


# ---- 5. poisoned work buffers ------------------------------------------------------------------------------------------------------------------------------------------
POISON_CASES = [(ac.MESHES[3], 2, "H1", 0.25), (ac.MESHES[-1], 1, "L2", 0.0)]


def poison_child():
    """what the child process of the test below runs, with FEMUS_HIP_POISON=1 in its environment: the comparison of test 1 on two cases"""
    import femus_amd
    assert os.environ.get("FEMUS_HIP_POISON") == "1"
    ctx = femus_amd.Context(0)
    try:
        for c in POISON_CASES:
            compare_case(ctx, *c)
    finally:
        ctx.close()
    print("poisoned comparison passed")


def test_under_poisoned_work_buffers(ctx):
    """with the option on this context, and with FEMUS_HIP_POISON=1 in a fresh child process (the variable is read when a context is made)"""
    try:
        ctx.set_option("debug_poison", 1)
        for c in POISON_CASES:
            compare_case(ctx, *c)
    finally:
        ctx.set_option("debug_poison", int(os.environ.get("FEMUS_HIP_POISON", "0")))      # what a context starts with
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_element_error_flag as t; t.poison_child()" % (HERE, ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FEMUS_HIP_POISON="1"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "poisoned comparison passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change,message", REFUSALS, ids=[",".join("%s=%s" % kv for kv in c.items()) for c, _ in REFUSALS])
def test_refusals(ctx, change, message):
    kind, ed, xs, own, lev, level = ac.mesh_of("tri2.neu", False, "read")
    dev = capi.ElementMesh.from_arrays(ctx, kind, ed, xs, ac.faces_of("tri2.neu", False, "read"), own)
    a = dict(fe=2, norm="H1", order="seventh", threshold=0.1, neighbor_threshold=0.0)
    a.update({k: v for k, v in change.items() if k != "short"})
    n = own[2] - (1 if "short" in change else 0)
    S, E = ctx.vector_from(np.ones(n)), ctx.vector_from(np.ones(n))
    try:
        with pytest.raises(capi.FemusHipError) as e:
            dev.flag_by_error(a["fe"], S, E, a["threshold"], a["norm"], a["neighbor_threshold"], a["order"])
        assert message in str(e.value)
        if not set(change) & {"threshold", "neighbor_threshold"}:
            with pytest.raises(capi.FemusHipError) as e:
                dev.error_indicators(a["fe"], E, a["norm"], a["order"])
            assert message in str(e.value)
    finally:
        for q in (S, E, dev):
            q.destroy()


def test_a_vector_of_another_context_is_refused(ctx):
    import femus_amd
    kind, ed, xs, own, lev, level = ac.mesh_of("tri2.neu", False, "read")
    dev = capi.ElementMesh.from_arrays(ctx, kind, ed, xs, ac.faces_of("tri2.neu", False, "read"), own)
    other = femus_amd.Context(0)
    S, E = ctx.vector_from(np.ones(own[2])), other.vector_from(np.ones(own[2]))
    try:
        with pytest.raises(capi.FemusHipError, match="a vector of another context"):
            dev.flag_by_error(2, S, E, 0.1)
        with pytest.raises(capi.FemusHipError, match="a vector of another context"):
            dev.error_indicators(2, E)
    finally:
        for q in (S, E, dev):
            q.destroy()
        other.close()


# ---- the adaptive driver -------------------------------------------------------------------------------------------------------------------------------------------------
LAYER = "exp(-10.*((x-1.)*(x-1.)+(y-1.)*(y-1.)))"


def box_config():
    return {"multilevel_mesh": {"first": {"type": {"box": {"nx": 2, "ny": 2, "nz": 0, "xa": 0., "xb": 1., "ya": 0., "yb": 1., "za": 0., "zb": 0., "elem_type": "Tri6"}}}},
            "multilevel_solution": {"multilevel_mesh": {"first": {"variable": {"first": {
                "name": "T", "fe_order": "second", "init_func": "0.", "func_source": "40.*" + LAYER,
                "boundary_conditions": [{"facename": n, "bdc_type": "dirichlet", "bdc_func": LAYER} for n in ("left", "right", "top", "bottom")]}}}}},
            "multilevel_problem": {"multilevel_mesh": {"first": {"system": {"poisson": {"linear_solver": {
                "max_number_linear_iteration": 12, "abs_conv_tol": 1.e-10,
                "type": {"multigrid": {"nlevels": 2, "npresmoothing": 1, "npostsmoothing": 1, "mgtype": "V_cycle"}}}}}}}}}


def layer(x):
    return np.exp(-10. * ((x[..., 0] - 1.) ** 2 + (x[..., 1] - 1.) ** 2))


# name -> (source, Dirichlet flags, boundary values, flux by flag, threshold of the adaptive run: between 10 % and 60 % of the 32 elements at the first step)
PROBLEMS = {"box": (lambda x: 40. * layer(np.asarray(x)), {-2, -3, -4, -5}, layer, None, 0.7),
            "triAMR": (lambda x: 100. * np.exp(-50. * ((x[0] - 0.5) ** 2 + (x[1] - 0.5) ** 2)), {-2, -3}, lambda x: 0.0 * x[..., 0], {-4: 0.2}, 0.3)}


@pytest.fixture(params=["box", "triAMR"])
def problem(request, ctx, tmp_path):
    if request.param == "box":
        p = app.Poisson001(ctx, box_config())
    else:
        os.makedirs(tmp_path / "input")
        (tmp_path / "input" / "triAMR.neu").write_bytes(open(os.path.join(HERE, "golden", "triAMR.neu"), "rb").read())
        cfg = EX4_CONFIG.replace('"nlevels" : 3', '"nlevels" : 2').replace('"func_source": "1."', '"func_source": "100.*exp(-50.*((x-0.5)*(x-0.5)+(y-0.5)*(y-0.5)))"')
        p = app.Poisson001(ctx, cfg, base_dir=str(tmp_path))
    assert p.nlevels == 2 and p.fe == "biquadratic"
    yield request.param, p
    p.destroy()


def direct(name, mesh, amr_mode="reference"):
    """the direct solve of the constrained system of a level (kind, ed, xs, ff, lev, level), from the oracle's element loop and the host rule's P_amr"""
    source, dirichlet, g, flux, _ = PROBLEMS[name]
    kind, ed, xs, ff, lev, level = mesh
    n = int(max(ed[kind == s][:, :mixed_mesh.CLASSES[s][2]].max() for s in set(kind.tolist()))) + 1
    K, F = fom.assemble(kind, ed, xs, "biquadratic", source)
    if flux:
        F = F + fom.neumann(kind, ed, xs, ff, "biquadratic", flux, n)
    c = mixed_mesh.amr_constraints(kind, ed, xs, ff, lev, "biquadratic", amr_mode)
    boundary = fom.dirichlet(kind, ed, ff, "biquadratic", dirichlet)
    fixed = np.union1d(boundary, c[0])
    values = np.where(np.isin(fixed, boundary), g(xs[fixed]), 0.0)      # a hanging dof is no unknown (one on the boundary too: P overwrites it)
    return constrained_solve(sp.csr_matrix(K), F, p_amr_of(c, n), fixed, values), c[0]


def test_nothing_flagged_is_the_plain_run(problem):
    name, p = problem
    out = p.run_elements_adaptive(3, 1.0e3)
    plain = p.run_elements(mesh_data="device")
    assert len(out["amr_history"]) == 1 and out["amr_history"][0]["converged"] and out["amr_history"][0]["nflagged"] == 0 and out["nlevels"] == 2
    assert out["amr_history"][0]["threshold_out"] == 1.0 and out["amr_history"][0]["nel"] == 32
    assert np.array_equal(bits(out["solution"]), bits(plain["solution"])) and np.array_equal(bits(out["coords"]), bits(plain["coords"]))
    assert out["history"] == plain["history"] and out["converged"] and out["hanging"].size == 0 and np.array_equal(out["elem_levels"], np.full(32, 1))
    assert p.nlevels == 2


def test_threshold_zero_refines_everything(problem):
    name, p = problem
    out = p.run_elements_adaptive(1, 0.0, keep_steps=True)
    assert out["amr_history"][0]["nflagged"] == 32 and [h["nel"] for h in out["amr_history"]] == [32, 128] and out["amr_history"][0]["threshold_out"] == 0.0
    assert not out["amr_history"][0]["converged"] and out["nlevels"] == 3 and out["hanging"].size == 0
    mesh = out["steps"][-1]["mesh"]
    level0 = mixed_mesh.tri_box(2, 2, (0., 0.), (1., 1.)) if name == "box" else mixed_mesh.read_gambit(os.path.join(HERE, "golden", "triAMR.neu"))
    uniform = mixed_mesh.refine(*mixed_mesh.refine(*level0[:4])[:4])
    assert np.array_equal(mesh[1], uniform[1]) and np.array_equal(bits(mesh[2]), bits(uniform[2])) and np.array_equal(mesh[3], uniform[3])
    assert np.array_equal(out["elem_levels"], np.full(128, out["elem_levels"][0])) and np.array_equal(mesh[4], out["elem_levels"])
    want, hang = direct(name, mesh)
    err = np.abs(out["solution"] - want).max()
    print("%s, everything refined: %d dofs, history %s, max |T - direct| = %.2e of %.2e" % (name, out["dofs"], out["history"], err, np.abs(want).max()))
    assert out["converged"] and hang.size == 0 and np.abs(want).max() > 1e-3 and err <= 1e-8


def test_an_adaptive_run(problem):
    name, p = problem
    thr = PROBLEMS[name][4]
    out = p.run_elements_adaptive(2, thr, keep_steps=True)
    hist = out["amr_history"]
    print("%s: %s" % (name, [(h["nflagged"], h["nel"], h["threshold_in"], h["threshold_out"], h["converged"]) for h in hist]))
    assert 0.1 * 32 <= hist[0]["nflagged"] <= 0.6 * 32 and hist[0]["nel"] == 32 and hist[0]["threshold_in"] == thr
    assert len(hist) >= 2 and len(hist) == len(out["steps"]) and out["nlevels"] == 2 + len(hist) - 1 <= 4
    for k, (h, st) in enumerate(zip(hist, out["steps"])):
        kind, ed, xs, ff, lev, level = st["mesh"]
        assert h["nel"] == kind.shape[0] and (k == 0 or h["threshold_in"] == hist[k - 1]["threshold_out"])
        host_step = capi.error_flag_host(kind, ed, xs, lev, level, 2, st["sol"], st["eps"], h["threshold_in"], "H1", 0.0)
        assert host_step["nflagged"] == h["nflagged"] and np.array_equal(host_step["flags"], st["flags"]) and host_step["converged"] == h["converged"]
        assert np.array_equal(bits(host_step["sums"]), bits(h["sums"])) and np.array_equal(bits(host_step["threshold"]), bits(h["threshold_out"]))
    mesh = out["steps"][-1]["mesh"]
    assert len(set(mesh[4].tolist())) > 1 and np.array_equal(mesh[4], out["elem_levels"])
    if name == "triAMR":                                              # two levels are added: elements of three levels, a transfer through P_amr of the level below
        assert len(hist) == 3 and hist[1]["nflagged"] > 0 and sorted(set(mesh[4].tolist())) == [1, 2, 3]
    want, hang = direct(name, mesh)
    assert out["hanging"].size > 0 and np.array_equal(out["hanging"], hang)
    err = np.abs(out["solution"] - want).max()
    print("%s, adaptive: %d dofs, %d hanging, history %s, max |T - direct| = %.2e of %.2e" % (name, out["dofs"], hang.size, out["history"], err, np.abs(want).max()))
    assert out["converged"] and np.abs(want).max() > 1e-3 and err <= 1e-8
    # no level added: the first estimate alone
    first = p.run_elements_adaptive(0, thr)
    assert len(first["amr_history"]) == 1 and first["nlevels"] == 2 and first["amr_history"][0]["nflagged"] == hist[0]["nflagged"]
    assert np.array_equal(bits(first["amr_history"][0]["sums"]), bits(hist[0]["sums"])) and first["dofs"] == out["steps"][0]["sol"].size
