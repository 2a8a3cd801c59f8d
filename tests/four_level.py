"""A shipped input of applications/001_Poisson on all four of its levels against the oracle, without a fixture: used by test_tet_3d.py, test_wedge_3d.py and
test_mixed_3d.py."""
import os

import numpy as np

from oracle import femus_oracle_mixed as om


def parity(ctx, tmp_path, mesh_file, config, fe, oracle, geom):
    """a shipped input on all four of its levels.  Operator: mixed_mesh.refine's finest mesh is the oracle's refine, integer for integer; the generic (or
    mixed) kernel's K and residual at a non-zero state and source equal the batched oracle entry by entry (1e-12).  Solution: app_poisson solved tightly
    (max_linear 40, abs_tol 1e-13); the oracle's residual of that solution -- its element loop plus its Neumann load -- is below 1e-10 of the load on the
    rows that are not Dirichlet rows, and the Dirichlet nodes hold their value, 0, exactly"""
    from femus_amd import app_poisson as app, capi, mixed_mesh
    a = mixed_mesh.read_gambit(mesh_file)
    b = oracle.read_gambit(mesh_file)
    for _ in range(3):
        a = mixed_mesh.refine(*a[:4])
        b = oracle.refine(*b[:4]) if geom == "mixed" else oracle.refine(*b[:3])
    if geom == "mixed":
        kind, ed, xs, ff, own = b
        assert np.array_equal(a[0], kind) and np.array_equal(a[1], ed) and np.array_equal(a[3], ff)
        nc = None
    else:
        ed, xs, ff, own = b
        kind, nc = geom, ed.shape[1]
        assert (a[0] == geom).all() and np.array_equal(a[1][:, :nc], ed) and np.all(a[1][:, nc:] == -1) and np.array_equal(a[3][:, :ff.shape[1]], ff)
    assert a[4] == own and np.abs(a[2] - xs).max() < 2e-15 and ed.shape[0] == 8 ** 3 * oracle.read_gambit(mesh_file)[1 if geom == "mixed" else 0].shape[0]
    ndof = om.n_dofs(own, fe)
    u = np.random.default_rng(11).uniform(-1, 1, ndof)
    Ko, Fo = om.assemble_batched(kind, ed, xs, fe, lambda x: np.exp(x[0]) * (1 + x[1]) - x[2], sol=u)
    Ko.sort_indices()
    K = capi.Mat.from_csr(ctx, ndof, ndof, Ko.indptr, Ko.indices)
    RES, SOL = ctx.vector(ndof), ctx.vector_from(u)
    f = capi.Expr("exp(x)*(1+y)-z", "x,y,z,t")
    try:
        if geom == "mixed":
            capi.assemble_poisson_mixed(ctx, fe, kind, ed, xs, K, RES, sol=SOL, source=f)
        else:
            capi.assemble_poisson_rows(ctx, geom, fe, ed, xs, K, RES, sol=SOL, source=f)
        Kd = K.to_scipy()
        Kd.sort_indices()
        assert np.array_equal(Kd.indptr, Ko.indptr) and np.array_equal(Kd.indices, Ko.indices)
        assert np.abs(Kd.data - Ko.data).max() <= 1e-12 * np.abs(Ko.data).max()
        assert np.abs(RES.to_numpy() - Fo).max() <= 1e-12 * np.abs(Fo).max()
    finally:
        f.destroy(), K.destroy(), RES.destroy(), SOL.destroy()
    # the solution
    os.makedirs(tmp_path / "input")
    (tmp_path / "input" / os.path.basename(mesh_file)).write_bytes(open(mesh_file, "rb").read())
    p = app.Poisson001(ctx, config, base_dir=str(tmp_path))
    try:
        p.max_linear, p.abs_tol = 40, 1e-13
        out = p.run()
    finally:
        p.destroy()
    assert out["converged"] and out["dofs"] == ndof
    x = out["solution"]
    flags, flux = (-2, -3, -5, -6, -7), {-4: 0.2}
    if geom == "mixed":
        load, bdc = om.neumann(kind, ed, xs, ff, fe, flux, ndof), om.dirichlet(kind, ed, ff, fe, set(flags))
    else:
        load, bdc = oracle.neumann(ed, xs, ff, fe, flux), oracle.dirichlet(ed, ff, fe, set(flags))
    _, R = om.assemble_batched(kind, ed, xs, fe, lambda x: 0.0, sol=x)
    R = R + load
    free = np.ones(ndof, bool)
    free[bdc] = False
    assert bdc.size > 0 and np.all(x[bdc] == 0.0)
    assert np.linalg.norm(R[free]) <= 1e-10 * np.linalg.norm(load), (np.linalg.norm(R[free]), np.linalg.norm(load))
