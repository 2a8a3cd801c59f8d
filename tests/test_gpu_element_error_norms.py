"""capi.ElementMesh.error_norms (fh_elem_mesh_error_norms): the L2 norm and the H1 semi-norm of a resident mesh's discrete function minus a known one, against the
host statement capi.error_norms_host -- the element body is one text compiled for both sides, so l2_i, h1_i and the norms are compared bit for bit wherever the
expressions are made of + - * / (and always against a second vector), and within the bound derived at test 2 for cos -- then the reports of the adaptive driver
Poisson001.run_elements_adaptive(exact=...)."""
import functools
import math
import os

import numpy as np
import pytest

import amr_flag_cases as ac
import error_norm_reference as enr
from femus_amd import app_poisson as app
from femus_amd import capi
from test_element_error_norms_host import CUBIC, MODES, REFUSALS, REFUSAL_IDS, TOL, refusal_arguments, vectors
from test_gpu_element_constraints import EX4_CONFIG
from test_gpu_element_error_flag import PROBLEMS, bits, box_config, resident

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# Each case hits one way the kernel can go wrong: L = 16 and elements of an older level; two shapes in one workgroup; the third-order rule; prisms; L = 64
# with the largest nc; three shapes with different nc and ng side by side; more than 1024 elements, so that the reduction takes two passes
HEX_B_SEVENTH = ("cube_Hex.neu", False, "b", "seventh", (2,))
DEVICE_CASES = [(ac.MESHES[1], fe) for fe in (0, 1, 2)] + [(ac.MESHES[3], 2), (ac.MESHES[5], 1), (ac.MESHES[8], 1), (HEX_B_SEVENTH, 2)] + \
               [(ac.MESHES[-1], fe) for fe in (0, 1, 2)] + [(ac.MESHES[6], 0)]


def device_case_id(c):
    return "%s-fe%d" % (ac.mesh_id(c[0]), c[1])


def arguments(dim, mode, table=CUBIC):
    ex, gr = table[dim]
    return {enr.QP: dict(exact=ex, gradient=gr), enr.DOFS: dict(exact=ex), enr.VECTOR: {}}[mode]


def both(ctx, dev, mesh, fe, order, sol, other, mode, table=CUBIC):
    """(device twice, host) for one call; mesh = (kind, ed, xs)"""
    kind, ed, xs = mesh
    a = arguments(xs.shape[1], mode, table)
    S = ctx.vector_from(sol)
    O = ctx.vector_from(other) if mode == enr.VECTOR else None
    try:
        d = [dev.error_norms(fe, S, against=O, order=order, per_element=True, **a) for _ in range(2)]
    finally:
        S.destroy()
        if O is not None:
            O.destroy()
    return d[0], d[1], capi.error_norms_host(kind, ed, xs, fe, sol, against=other if mode == enr.VECTOR else None, order=order, **a)


def same_bits(d, h):
    assert np.array_equal(bits(d["elem_l2"]), bits(h["elem_l2"])) and np.array_equal(bits(d["elem_h1"]), bits(h["elem_h1"]))
    assert np.array_equal(bits([d["l2"], d["h1"]]), bits([h["l2"], h["h1"]]))


def compare_case(ctx, m, fe):
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    s, o = vectors(m, fe)
    dev = resident(ctx, m)
    try:
        for mode in MODES:
            d, again, h = both(ctx, dev, (kind, ed, xs), fe, m[3], s, o, mode)
            same_bits(d, h)
            same_bits(again, d)
            assert h["l2"] > 0 and h["h1"] > 0 and np.isfinite(d["elem_l2"]).all() and np.isfinite(d["elem_h1"]).all()
    finally:
        dev.destroy()


# ---- 1. device = host statement, and a call repeats its bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DEVICE_CASES, ids=device_case_id)
def test_the_device_equals_the_host_statement_and_repeats_its_bits(ctx, case):
    if case[0] is ac.MESHES[6]:
        assert ac.mesh_of(*case[0][:3])[0].shape[0] > 3 * 1024          # four chunks of the fixed-shape sum, then a second pass over them
    compare_case(ctx, *case)


def one_triangle():
    """a mesh of one TRI7 element: every other sub-group of its workgroup is a tail"""
    v = np.array([[0.1, 0.2], [1.3, 0.1], [0.4, 1.1]])
    xs = np.vstack([v, (v[0] + v[1]) / 2, (v[1] + v[2]) / 2, (v[2] + v[0]) / 2, v.mean(axis=0)])
    ed = np.full((1, 27), -1, dtype=np.int64)
    ed[0, :7] = np.arange(7)
    ff = np.full((1, 6), -1, dtype=np.int64)
    ff[0, :3] = -2
    return np.array(["tri"]), ed, xs, ff, [3, 6, 7]


def test_a_mesh_of_one_element(ctx):
    kind, ed, xs, ff, own = one_triangle()
    dev = capi.ElementMesh.from_arrays(ctx, kind, ed, xs, ff, own)
    try:
        for fe in (0, 1, 2):
            s = 1.0 + np.arange(own[fe]) * 0.37
            for mode in MODES:
                d, again, h = both(ctx, dev, (kind, ed, xs), fe, "seventh", s, 0.5 * s[::-1], mode)
                same_bits(d, h)
                same_bits(again, d)
                assert d["elem_l2"].shape == (1,) and d["l2"] > 0 and d["l2"] == math.sqrt(d["elem_l2"][0]) and d["h1"] == math.sqrt(d["elem_h1"][0])
    finally:
        dev.destroy()


# ---- 2. a transcendental exact solution ----------------------------------------------------------------------------------------------------------------------------------
COSINES = {2: ("cos(pi*x)*cos(pi*y)", ["0-pi*sin(pi*x)*cos(pi*y)", "0-pi*cos(pi*x)*sin(pi*y)"]),
           3: ("cos(pi*x)*cos(pi*y)*cos(pi*z)", ["0-pi*sin(pi*x)*cos(pi*y)*cos(pi*z)", "0-pi*cos(pi*x)*sin(pi*y)*cos(pi*z)", "0-pi*cos(pi*x)*cos(pi*y)*sin(pi*z)"])}
# ulps of one factor: the device's bound for sin and cos alike (4) plus the host's (1)
ULPS_PER_FACTOR = 4 + 1


def cosine_arrays(dim):
    """the exact solution and its gradient on arrays of points [..., dim]"""
    def exact(x):
        return np.cos(np.pi * x).prod(axis=-1)

    def gradient(x):
        c, sn = np.cos(np.pi * x), np.sin(np.pi * x)
        return np.stack([-np.pi * np.where(np.arange(dim) == j, sn, c).prod(axis=-1) for j in range(dim)], axis=-1)
    return exact, gradient


@functools.lru_cache(maxsize=None)
def cosine_bounds(m, fe, mode):
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    ex, gr = cosine_arrays(xs.shape[1])
    return enr.magnitude_bounds(kind, ed, xs, fe, vectors(m, fe)[0], mode, ex, gr, None, m[3])


@pytest.mark.parametrize("mode", [enr.QP, enr.DOFS])
@pytest.mark.parametrize("case", DEVICE_CASES, ids=device_case_id)
def test_a_transcendental_exact_solution(ctx, case, mode):
    """|dev - host| <= (TOL + 2 K 2^-52) B_i per element, K = 5 dim.
    The two sides differ in the values of the programs alone: the arguments pi * x are products, the same bits on both.  Every value u (the exact solution or a
    component of its gradient) is a product of dim factors sin or cos, each within 4 ulp of the true value on the device and within 1 ulp on the
    host, so the two values of u differ by at most K 2^-52 |u| with K = (4 + 1) dim to first order (one ulp is at most 2^-52 relative; the products' own
    roundings are the same operations on both sides and amplify nothing).  A term (h - u)^2 w then differs by at most 2 |h - u| |du| w <= 2 K 2^-52 (|h| + |u|)
    |u| w <= 2 K 2^-52 (sum |phi_i sol_i| + |u|)^2 w, which is 2 K 2^-52 times the term's share of B_i; in mode dofs u = sum phi_i U_i and |du| <= K 2^-52 sum
    |phi_i U_i|, which is what B_i holds there.  What is of second order in du, and the common roundings after the difference, are within TOL B_i, the host
    statement's own bound (TOL is the larger part of the factor: 6.1e-14 of 6.5e-14 in two dimensions).  Largest ratio seen on an MI355X: 2.1e-16.
    The norms: the squared totals within the same factor of sum B_i plus 2 N 2^-53 of the total for the order of the sums."""
    m, fe = case
    kind, ed, xs, own, lev, level = ac.mesh_of(*m[:3])
    dim = xs.shape[1]
    s, o = vectors(m, fe)
    r = cosine_bounds(m, fe, mode)
    dev = resident(ctx, m)
    try:
        d, again, h = both(ctx, dev, (kind, ed, xs), fe, m[3], s, o, mode, COSINES)
    finally:
        dev.destroy()
    same_bits(again, d)
    factor = TOL + 2 * ULPS_PER_FACTOR * dim * 2.0 ** -52
    worst = 0.0
    for key, B, n in (("l2", r["B_l2"], r["N_l2"]), ("h1", r["B_h1"], r["N_h1"])):
        dist = np.abs(d["elem_" + key] - h["elem_" + key])
        assert (B > 0).all()
        worst = max(worst, float((dist / B).max()))
        assert (dist <= factor * B).all(), key
        assert abs(d[key] ** 2 - h[key] ** 2) <= factor * B.sum() + 2 * n * 2.0 ** -53 * h[key] ** 2, key
    print("largest |dev - host| / B = %.3e of %.3e" % (worst, factor))


# ---- 3. poisoned work buffers --------------------------------------------------------------------------------------------------------------------------------------------
def test_under_poisoned_work_buffers(ctx):
    try:
        ctx.set_option("debug_poison", 1)
        compare_case(ctx, ac.MESHES[3], 2)
        compare_case(ctx, ac.MESHES[6], 0)
    finally:
        ctx.set_option("debug_poison", int(os.environ.get("FEMUS_HIP_POISON", "0")))      # what a context starts with


# ---- 4. the driver, uniform levels ---------------------------------------------------------------------------------------------------------------------------------------
# polynomials that vanish on the boundary of the unit square / cube, outside every family's space; the source is minus their Laplacian
BUBBLE = {2: ("x*(1-x)*y*(1-y)", ["(1-2*x)*y*(1-y)", "x*(1-x)*(1-2*y)"], "2*(y*(1-y)+x*(1-x))"),
          3: ("x*(1-x)*y*(1-y)*z*(1-z)", ["(1-2*x)*y*(1-y)*z*(1-z)", "x*(1-x)*(1-2*y)*z*(1-z)", "x*(1-x)*y*(1-y)*(1-2*z)"],
              "2*(y*(1-y)*z*(1-z)+x*(1-x)*z*(1-z)+x*(1-x)*y*(1-y))")}


def uniform_problem(ctx, name, nlevels, tmp_path):
    if name == "box":
        cfg = box_config()
        var = cfg["multilevel_solution"]["multilevel_mesh"]["first"]["variable"]["first"]
        var["func_source"] = BUBBLE[2][2]
        for bc in var["boundary_conditions"]:
            bc["bdc_func"] = "0."
        cfg["multilevel_problem"]["multilevel_mesh"]["first"]["system"]["poisson"]["linear_solver"]["type"]["multigrid"]["nlevels"] = nlevels
        return app.Poisson001(ctx, cfg)
    os.makedirs(tmp_path / "input", exist_ok=True)
    (tmp_path / "input" / "cube_Tet.neu").write_bytes(open(os.path.join(HERE, "golden", "cube_Tet.neu"), "rb").read())
    cfg = EX4_CONFIG.replace("triAMR.neu", "cube_Tet.neu").replace('"nlevels" : 3', '"nlevels" : %d' % nlevels).replace('"func_source": "1."',
                                                                                                                   '"func_source": "%s"' % BUBBLE[3][2])
    p = app.Poisson001(ctx, cfg, base_dir=str(tmp_path))
    p.file_flux = {}                # every face of the cube is Dirichlet 0: the bubble is the solution
    return p


@pytest.mark.parametrize("name,levels", [("box", (2, 3, 4)), ("cube_Tet", (2, 3))])
def test_the_driver_reports_the_errors_of_uniform_levels(ctx, tmp_path, name, levels):
    """max_amr_levels = 0: one solve on nlevels uniform levels, the row of ex02's convergence table.  The expressions are polynomials: the report is the host
    statement on the downloaded level bit for bit (the rule of test 1).  Both errors fall strictly from level to level; the orders are printed, not asserted"""
    dim = 2 if name == "box" else 3
    ex, gr, _ = BUBBLE[dim]
    rows = []
    for nl in levels:
        p = uniform_problem(ctx, name, nl, tmp_path)
        try:
            assert p.nlevels == nl and p.fe == "biquadratic"
            out = p.run_elements_adaptive(0, 1.0e3, keep_steps=True, exact=ex, exact_gradient=gr)
        finally:
            p.destroy()
        assert len(out["amr_history"]) == 1
        hist, st = out["amr_history"][0], out["steps"][0]
        kind, ed, xs, ff, lev, level = st["mesh"]
        assert abs(xs.min()) <= 1e-12 and abs(xs.max() - 1.0) <= 1e-12          # the unit square / cube: the bubble vanishes on its boundary
        h = capi.error_norms_host(kind, ed, xs, 2, st["sol"], exact=ex, gradient=gr)
        assert np.array_equal(bits([hist["l2_error"], hist["h1_error"]]), bits([h["l2"], h["h1"]]))
        rows.append((kind.shape[0], hist["l2_error"], hist["h1_error"]))
    for a, b in zip(rows, rows[1:]):
        print("%s: %d -> %d elements, L2 %.3e -> %.3e (order %.2f), H1 %.3e -> %.3e (order %.2f)" % (name, a[0], b[0], a[1], b[1], math.log2(a[1] / b[1]), a[2], b[2],
                                                                                                  math.log2(a[2] / b[2])))
        assert 0 < b[1] < a[1] and 0 < b[2] < a[2]


# ---- 5. the driver, adaptive -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["box", "triAMR"])
def problem(request, ctx, tmp_path):
    """the problems of test_gpu_element_error_flag.test_an_adaptive_run"""
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


HISTORY_KEYS = {"nflagged", "nel", "threshold_in", "threshold_out", "sums", "converged"}


def test_the_adaptive_driver_reports_the_errors_of_every_step(problem):
    """the comparison function is a polynomial (the host statement's bits; it need not be the problem's solution for that): with its gradient the report is mode
    qp, without it mode dofs.  Without exact the history has the keys it had before, and the same flags"""
    name, p = problem
    thr = PROBLEMS[name][4]
    ex, gr = CUBIC[2]
    plain = p.run_elements_adaptive(2, thr)
    assert len(plain["amr_history"]) >= 2 and all(set(h) == HISTORY_KEYS for h in plain["amr_history"])
    for gradient in (gr, None):
        out = p.run_elements_adaptive(2, thr, keep_steps=True, exact=ex, exact_gradient=gradient)
        hist = out["amr_history"]
        assert len(hist) == len(out["steps"]) == len(plain["amr_history"])
        for h, st, q in zip(hist, out["steps"], plain["amr_history"]):
            assert set(h) == HISTORY_KEYS | {"l2_error", "h1_error"}
            assert all(np.array_equal(h[k], q[k]) for k in HISTORY_KEYS)
            kind, ed, xs, ff, lev, level = st["mesh"]
            host = capi.error_norms_host(kind, ed, xs, 2, st["sol"], exact=ex, gradient=gradient)
            assert np.array_equal(bits([h["l2_error"], h["h1_error"]]), bits([host["l2"], host["h1"]])) and host["l2"] > 0 and host["h1"] > 0
        assert len(set(out["steps"][-1]["mesh"][4].tolist())) > 1          # the last level holds elements of more than one level
        assert np.array_equal(bits(out["solution"]), bits(plain["solution"]))


# ---- 6. refusals on the device path ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change,message", REFUSALS, ids=REFUSAL_IDS)
def test_refusals(ctx, change, message):
    kind, ed, xs, own, lev, level = ac.mesh_of("tri2.neu", False, "read")
    dev = capi.ElementMesh.from_arrays(ctx, kind, ed, xs, ac.faces_of("tri2.neu", False, "read"), own)
    vecs = []

    def vector(a):
        vecs.append(ctx.vector_from(a))
        return vecs[-1]
    a, made = refusal_arguments(change, own[2], vector)
    try:
        with pytest.raises(capi.FemusHipError) as e:
            dev.error_norms(a["fe"], a["sol"], a["exact"], a["gradient"], a["against"], a["order"])
        assert message in str(e.value)
    finally:
        for q in made + vecs + [dev]:
            q.destroy()


def test_a_vector_of_another_context_is_refused(ctx):
    import femus_amd
    kind, ed, xs, own, lev, level = ac.mesh_of("tri2.neu", False, "read")
    dev = capi.ElementMesh.from_arrays(ctx, kind, ed, xs, ac.faces_of("tri2.neu", False, "read"), own)
    other = femus_amd.Context(0)
    S, E = ctx.vector_from(np.ones(own[2])), other.vector_from(np.ones(own[2]))
    try:
        with pytest.raises(capi.FemusHipError, match="other is a vector of another context than the mesh's"):
            dev.error_norms(2, S, against=E)
        with pytest.raises(capi.FemusHipError, match="sol is a vector of another context than the mesh's"):
            dev.error_norms(2, E, exact="x")
    finally:
        for q in (S, E, dev):
            q.destroy()
        other.close()
