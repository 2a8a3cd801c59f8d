"""tests/quasilinear_reference.py, the yardstick of the quasilinear kernel, checked on the host before anything is measured with it:
(a) with f alone it is the Poisson callback: the oracles' element loops on the meshes of tests/test_gpu_generic_assembler.py (unrefined, curved), to that
    file's bound, 1e-12 of the largest entry;
(b) its Jacobian is the derivative of its residual: K delta against the five-point central difference of -RES along delta."""
import numpy as np
import pytest
import scipy.sparse as sp

import quasilinear_reference as qr
from test_gpu_generic_assembler import CASES, FES, SOURCE, args_of, curved, mesh

_MESH = {}


def setup(case):
    if case not in _MESH:
        kind, ed, xs, own = mesh(case, refinements=0)
        _MESH[case] = (kind, ed, curved(xs), own)
    return _MESH[case]


@pytest.mark.parametrize("fe", FES)
@pytest.mark.parametrize("case", CASES)
def test_with_f_alone_it_is_the_oracles_poisson_loop(case, fe):
    from oracle import femus_oracle_mixed as om, femus_oracle_tet as oq, femus_oracle_tri as ot, femus_oracle_wedge as ow
    kind, ed_full, xs, own = setup(case)
    ndof = own[qr.FAM[fe]]
    u = np.random.default_rng(11).uniform(-1, 1, ndof)
    src = SOURCE[xs.shape[1]][1]
    geom, ed = args_of(kind, ed_full)
    if case in ("mixed3d", "mixed2d"):
        Ko, Fo = om.assemble(kind, ed_full, xs, fe, src, u)
    else:
        Ko, Fo = {"tri": ot, "tet": oq, "wedge": ow}[case].assemble(ed, xs, fe, src, u)
    Ko, Fo = sp.csr_matrix(Ko), np.asarray(Fo)
    K, F = qr.assemble(kind, ed_full, xs, fe, {"f": lambda v: src(v[:3])}, u)
    dK, dF = abs(K - Ko).max(), np.abs(F - Fo).max()
    print("%s %s: |K - oracle| = %.3e of %.3e, |RES - oracle| = %.3e of %.3e" % (case, fe, dK, abs(Ko).max(), dF, np.abs(Fo).max()))
    assert dK <= 1e-12 * abs(Ko).max()
    assert dF <= 1e-12 * np.abs(Fo).max()


# the step of the difference per form: 2^-3 where RES is a cubic in u, so that the five-point formula is exact up to rounding
FORMS = {"A": (qr.form_a, 2.0 ** -3), "B-diffusivity": (lambda dim: tuple({k: d[k] for k in ("a", "a_u")} for d in qr.form_b(dim)), 2.0 ** -3),
         "B": (qr.form_b, 2.0 ** -10)}
JACOBIAN_TOL = 4.4e-12     # 10 x the largest defect seen over the cases below (4.324e-13 of max |K delta|: "B", mixed2d, linear; 3.0e-15 at h = 2^-3), far below the 1e-9 that is asked


@pytest.mark.parametrize("name", list(FORMS))
@pytest.mark.parametrize("fe", ["linear", "biquadratic"])
@pytest.mark.parametrize("case", CASES)
def test_the_jacobian_is_the_derivative_of_the_residual(case, fe, name):
    """K(u) delta = d(-RES)(u + t delta)/dt at t = 0, the derivative by (R(-2h) - 8 R(-h) + 8 R(h) - R(2h)) / 12h.
    Form A (ex03) and the diffusivity of form B (ex03b: a = 1 + u^2) make RES a cubic in u: at h = 2^-3 the formula has no truncation error and the steps are
    exact in binary.  The reaction of the full form B, sqrt(1 + u^2), is not a polynomial, so the full form is differenced at h = 2^-10: truncation
    h^4 |c^(5)| / 30 < 1e-12 of |c| (|c^(5)| <= 15 for this c), rounding about 2^-53 |RES| / h = 1e-13 |RES|.  Both far below the bound 1e-9 max |K delta|.
    Largest defect seen over all cases: 4.324e-13 of max |K delta| (the full form B at h = 2^-10; 3.0e-15 for the two forms at h = 2^-3); JACOBIAN_TOL is ten
    times that."""
    kind, ed_full, xs, own = setup(case)
    dim = xs.shape[1]
    make, h = FORMS[name]
    _, form = qr.with_source(make(dim), dim)
    ndof = own[qr.FAM[fe]]
    rng = np.random.default_rng(11)
    u, delta = rng.uniform(-1, 1, ndof), rng.uniform(-1, 1, ndof)
    K, _ = qr.assemble(kind, ed_full, xs, fe, form, u)
    R = {t: qr.assemble(kind, ed_full, xs, fe, form, u + t * h * delta)[1] for t in (-2, -1, 1, 2)}
    dR = (R[-2] - 8 * R[-1] + 8 * R[1] - R[2]) / (12 * h)
    Kd = K @ delta
    defect = np.abs(Kd + dR).max() / np.abs(Kd).max()
    print("%s %s form %s: |K delta + dRES| = %.3e of max |K delta|" % (case, fe, name, defect))
    assert JACOBIAN_TOL < 1e-9
    assert defect <= JACOBIAN_TOL
    if name == "A":
        assert abs(K - K.T).max() > 1e-3 * abs(K).max()          # the advection term: nothing symmetric about this Jacobian
