"""Dev probe: the error norms of a resident element mesh's function against a known one (capi.ElementMesh.error_norms, fh_elem_mesh_error_norms) in each mode,
against the host statement of the same rule in the library (capi.error_norms_host, fh_elem_error_norms_host: the same element body, one thread) in the same
process, and against the computation a user without either would write: numpy on the downloaded arrays.

  python tests/perf_probe_element_error_norms.py                one JSON line; also written to profiles/element_error_norms_probe.json
  python tests/perf_probe_element_error_norms.py --device-only  without the host and numpy sides (and without writing the file)

The mesh is that of tests/perf_probe_element_error_flag.py: cube_Tet.neu refined three times on the device, flagged by the half-space x > 0.5 and refined once
more (254 464 TET15 elements of two levels), the 31-point rule.  sol is the nodal interpolant of cos(pi x) cos(pi y) cos(pi z) plus a small smooth
perturbation, `against` the interpolant itself.  Every device figure is a host clock around calls that end in a synchronisation: REPEATS runs after WARMUP
unmeasured ones; median, minimum and maximum in ms.
  device_ms   error_norms in the mode (the call uploads tables and programs, runs the element kernel and the sums, and brings back two doubles)
  host_ms     error_norms_host on the downloaded arrays, once
  numpy_ms    mode qp in array operations on the downloaded arrays (tables from the library), once"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "element_error_norms_probe.json")
MESH, NUNIFORM, EXPR = "cube_Tet.neu", 3, "x > 0.5"
WARMUP, REPEATS = 3, 11
FAMILIES = ["biquadratic", "linear"]
EXACT = "cos(pi*x)*cos(pi*y)*cos(pi*z)"
GRADIENT = ["0-pi*sin(pi*x)*cos(pi*y)*cos(pi*z)", "0-pi*cos(pi*x)*sin(pi*y)*cos(pi*z)", "0-pi*cos(pi*x)*cos(pi*y)*sin(pi*z)"]


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def timed(ctx, fn):
    out = []
    for k in range(WARMUP + REPEATS):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        t1 = time.perf_counter()
        if k >= WARMUP:
            out.append((t1 - t0) * 1e3)
    return stats(out)


def numpy_qp(capi, ed, xs, fe, sol):
    """(l2, h1) against the exact values at the Gauss points, in array operations over all elements at once"""
    phi, dphi = capi.fe_tables("tet", fe, "seventh")
    w = capi.fe_gauss("tet", "seventh")[0]
    nc = phi.shape[1]
    dof = ed[:, :nc]
    X, S = xs[dof], sol[dof]
    J = np.einsum("gna,enb->egab", dphi, X)
    weight = np.linalg.det(J) * w[None, :]
    gp = np.einsum("gnb,egab->egna", dphi, np.linalg.inv(J))
    uh, gh = np.einsum("gn,en->eg", phi, S), np.einsum("egna,en->ega", gp, S)
    xg = np.einsum("gn,enj->egj", phi, X)
    c, s = np.cos(np.pi * xg), np.sin(np.pi * xg)
    u = c.prod(axis=-1)
    g = np.stack([-np.pi * np.where(np.arange(3) == j, s, c).prod(axis=-1) for j in range(3)], axis=-1)
    return float(np.sqrt(((uh - u) ** 2 * weight).sum())), float(np.sqrt((((gh - g) ** 2).sum(axis=-1) * weight).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    import femus_amd
    from femus_amd import capi, mixed_mesh
    ctx = femus_amd.Context(0)
    dev = [capi.ElementMesh.from_arrays(ctx, *mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", MESH)))]
    for _ in range(NUNIFORM):
        dev.append(dev[-1].refine())
    dev[-1].flag(EXPR)
    dev.append(dev[-1].refine("resident"))
    c = dev[-1]
    xs = c.coords()
    exact, gradient = capi.Expr(EXACT), [capi.Expr(t) for t in GRADIENT]
    out = {"mesh": MESH, "nel": c.nel, "nnode": c.nnode, "level": c.level, "rule": "seventh", "warmup": WARMUP, "repeats": REPEATS, "cases": {}}
    if not a.device_only:
        kind, ed, xh, ff, own = c.arrays()
    for fe in FAMILIES:
        n = c.own[capi.FE[fe]]
        x = xs[:n]
        interp = np.cos(np.pi * x).prod(axis=1)
        sol = interp + 1e-3 * np.sin(3.0 * x[:, 0]) * x[:, 1] * (1.0 + x[:, 2])
        S, O = ctx.vector_from(sol), ctx.vector_from(interp)
        calls = {"qp": dict(exact=exact, gradient=gradient), "dofs": dict(exact=exact), "vector": dict(against=O)}
        host_args = {"qp": dict(exact=exact, gradient=gradient), "dofs": dict(exact=exact), "vector": dict(against=interp)}
        one = {}
        for mode, kw in calls.items():
            r = {"device_ms": timed(ctx, lambda: c.error_norms(fe, S, **kw))}
            d = c.error_norms(fe, S, **kw)
            r.update(l2=d["l2"], h1=d["h1"])
            if not a.device_only:
                t0 = time.perf_counter()
                h = capi.error_norms_host(kind, ed, xh, fe, sol, **host_args[mode])
                r["host_ms"] = (time.perf_counter() - t0) * 1e3
                r["host_l2"], r["host_h1"] = h["l2"], h["h1"]
                r["equal_bits"] = bool(h["l2"] == d["l2"] and h["h1"] == d["h1"])
                r["host_over_device"] = r["host_ms"] / r["device_ms"]["median"]
            one[mode] = r
        if not a.device_only:
            t0 = time.perf_counter()
            l2, h1 = numpy_qp(capi, ed, xh, fe, sol)
            one["numpy_qp"] = {"numpy_ms": (time.perf_counter() - t0) * 1e3, "l2": l2, "h1": h1}
        out["cases"][fe] = one
        S.destroy()
        O.destroy()
    for e in [exact] + gradient:
        e.destroy()
    for m in dev:
        m.destroy()
    ctx.close()
    if not a.device_only:
        with open(OUT, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
