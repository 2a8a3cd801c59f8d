"""Bit record of the Krylov solvers, for comparing two builds of the library (FEMUS_HIP_LIBRARY names the one to load).

    python tests/dev/krylov_bits.py dump OUT.json          one build, in a process of its own
    python tests/dev/krylov_bits.py compare A.json B.json OUT.json

dump: on the 2x2x2 HEX27 box with three levels, every outer solver (GMRES under gmres_device 1 and 0) with use_graph 1 and 0, and one V-cycle with the
GMRES level solver (restarts 3 and 30, the hierarchy of test_gmres_level_solver_matches_the_oracle); iterations, final residual and solution as uint64
words.  compare: exits non-zero unless every word of the two records is the same."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def words(a):
    import numpy as np
    return [int(w) for w in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)]


def dump(path):
    import numpy as np
    import femus_amd
    from femus_amd import capi
    from oracle import femus_oracle as fo

    H = fo.build_poisson_hierarchy(2, 2, 2, 3, "biquadratic", lambda xg: np.ones(xg.shape[:2]))
    n = H.A[-1].shape[0]
    ctx = femus_amd.Context(0)
    rec = {}

    def hierarchy(smoother=0, omega=2. / 3., npre=2, npost=2, level_restart=None):
        mg = capi.Multigrid(ctx, 3)
        mats = []
        for l in range(3):
            A = ctx.matrix_scipy(H.A[l])
            P = ctx.matrix_scipy(H.P[l]) if l > 0 else None
            mats += [A, P]
            mg.set_level(l, A, P, None, smoother, omega, npre, npost)
            if l > 0 and level_restart:
                mg.set_level_solver(l, "gmres", level_restart)
        mg.setup()
        return mg, mats

    for graph in (1, 0):
        ctx.set_option("use_graph", graph)
        for outer, dev in (("richardson", 1), ("cg", 1), ("gmres", 1), ("gmres", 0), ("fgmres", 1)):
            ctx.set_option("gmres_device", dev)
            mg, mats = hierarchy()
            b, x = ctx.vector_from(H.b), ctx.vector(n)
            its, rn = mg.solve(b, x, outer=outer, rtol=1e-12, maxit=60)
            rec["%s gmres_device=%d use_graph=%d" % (outer, dev, graph)] = {"iterations": int(its), "final_residual": words([rn])[0], "x": words(x.to_numpy())}
            if outer == "gmres":      # more iterations than one restart cycle
                mgw, matsw = hierarchy(omega=0.3, npre=1, npost=0)
                its, rn = mgw.solve(b, x, outer=outer, rtol=1e-11, maxit=200, restart=5)
                rec["%s restart=5 gmres_device=%d use_graph=%d" % (outer, dev, graph)] = {"iterations": int(its), "final_residual": words([rn])[0],
                                                                                         "x": words(x.to_numpy())}
                mgw.destroy()
            mg.destroy()
        ctx.set_option("gmres_device", 1)
        rhs = fo.lcg_fill(n, 21)
        for smoother in (capi.SMOOTH_JACOBI, capi.SMOOTH_SOR):
            for restart, npre, npost in ((3, 4, 4), (30, 2, 1)):
                mg, mats = hierarchy(smoother, 1.0, npre, npost, restart)
                b, x = ctx.vector_from(rhs), ctx.vector(n)
                for rep in range(2):
                    mg.vcycle(b, x)
                    rec["level gmres smoother=%d restart=%d use_graph=%d rep=%d" % (smoother, restart, graph, rep)] = {"x": words(x.to_numpy())}
                bb, xx = ctx.vector_from(H.b), ctx.vector(n)
                its, rn = mg.solve(bb, xx, outer="fgmres", rtol=1e-10, maxit=60)
                rec["fgmres around level gmres smoother=%d restart=%d use_graph=%d" % (smoother, restart, graph)] = {
                    "iterations": int(its), "final_residual": words([rn])[0], "x": words(xx.to_numpy())}
                mg.destroy()
    ctx.set_option("use_graph", 1)
    with open(path, "w") as f:
        json.dump({"library": os.environ.get("FEMUS_HIP_LIBRARY", "in-tree"), "device": ctx.device_name(), "records": rec}, f)
    print("krylov_bits: %d records written to %s" % (len(rec), path))
    ctx.close()


def compare(pa, pb, out):
    import hashlib
    A, B = json.load(open(pa)), json.load(open(pb))
    ra, rb = A["records"], B["records"]
    assert sorted(ra) == sorted(rb), "the two records hold different cases"
    cases, differ = [], 0
    for k in sorted(ra):
        same = ra[k] == rb[k]
        differ += not same
        nwords = len(ra[k]["x"]) + ("final_residual" in ra[k])
        cases.append({"case": k, "iterations": ra[k].get("iterations"), "final_residual_word": ra[k].get("final_residual"), "words": nwords,
                      "sha256_of_words": hashlib.sha256(json.dumps(ra[k], sort_keys=True).encode()).hexdigest(), "identical": same})
    json.dump({"what": "iterations, final residual and solution of the Krylov solvers as uint64 words, parent build against this one (tests/dev/krylov_bits.py)",
               "device": A["device"], "cases": len(cases), "words_compared": sum(c["words"] for c in cases), "cases_that_differ": differ, "records": cases},
              open(out, "w"), indent=1)
    print("krylov_bits: %d cases, %d differ" % (len(cases), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(*sys.argv[2:5]))
