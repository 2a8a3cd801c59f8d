"""Bit record of the block Schwarz smoothers (FH_SMOOTH_VANKA, FH_SMOOTH_ASM), for comparing two builds of the library (FEMUS_HIP_LIBRARY names
the one to load).

    python tests/dev/patch_bits.py dump OUT.json          one build, in a process of its own
    python tests/dev/patch_bits.py compare A.json B.json OUT.json

dump: on the 4x4 Navier-Stokes cavity with three levels at a non-trivial state, one V(2,2) cycle as uint64 words for: Vanka under vanka_persistent
0 / 1 / 2 and, unfused, under vanka_fused 0, each with patch_invert_lds 0 / 1; PCASM with 0 and 5 exact blocks under the Richardson and the GMRES level
solver, fused and unfused; a second preparation at another state on the same object; a set_level of the same Multigrid onto padded patterns.
compare: exits non-zero unless every word of the two records is the same."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def words(a):
    import numpy as np
    return [int(w) for w in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)]


def padded(M):
    """M on a larger stored pattern (one more position in every row that lacks it, holding an explicit zero)"""
    import numpy as np
    import scipy.sparse as sp
    M = M.tocsr()
    M.sort_indices()
    n = M.shape[0]
    ones = sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    extra = sp.coo_matrix((np.ones(n), (np.arange(n), (np.arange(n) * 7 + 3) % n)), shape=M.shape).tocsr()
    pat = (ones + extra).tocsr()
    pat.sort_indices()
    assert pat.nnz > M.nnz
    key = lambda A: np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr)) * n + A.indices
    full = sp.csr_matrix((np.zeros(pat.nnz), pat.indices.copy(), pat.indptr.copy()), shape=M.shape)
    full.data[np.searchsorted(key(pat), key(M))] = M.data
    return full


def dump(path):
    import numpy as np
    import femus_amd
    from femus_amd import capi
    from femus_amd.navier_stokes import NavierStokesMG
    from oracle import femus_oracle_ns as ns

    nu, nl, top = 0.01, 3, 2
    LO, HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
    ms, lays = ns.build_ns_levels(4, 4, 0, nl, LO, HI)
    bcs = [ns.cavity_bc(m, l) for m, l in zip(ms, lays)]
    n = lays[top].n
    rng = np.random.default_rng(5)
    states = []
    for k in range(2):
        st = (0.3 + 0.4 * k) * rng.standard_normal(n)
        st[bcs[top][0]] = bcs[top][1]
        states.append(st)
    b = rng.standard_normal(n)
    b[bcs[top][0]] = 0.0
    ctx = femus_amd.Context(0)
    rec = {}

    def cycle(mg):
        bv, x = ctx.vector_from(b), ctx.vector(n)
        mg.vcycle(bv, x)
        out = x.to_numpy().copy()
        assert np.isfinite(out).all()
        bv.destroy(), x.destroy()
        return {"x": words(out)}

    def problem(code, state):
        pb = NavierStokesMG(ctx, 4, 4, 0, nl, nu).init()
        pb.smoother = code
        pb.SOL[top].upload(state)
        return pb

    def option_sets():
        for lds in (0, 1):
            for persistent, fused in ((0, 1), (1, 1), (2, 1), (0, 0)):
                yield persistent, fused, lds

    for persistent, fused, lds in option_sets():
        ctx.set_option("vanka_persistent", persistent)
        ctx.set_option("vanka_fused", fused)
        ctx.set_option("patch_invert_lds", lds)
        tag = "vanka_persistent=%d vanka_fused=%d patch_invert_lds=%d" % (persistent, fused, lds)
        pb = problem(capi.SMOOTH_VANKA, states[0])
        rec["vanka " + tag] = cycle(pb.prepare(top))
        if persistent == 0:       # the same object prepared at another state
            pb.SOL[top].upload(states[1])
            rec["vanka second preparation " + tag] = cycle(pb.prepare(top))
        pb.destroy()
    ctx.set_option("vanka_persistent", 0)
    ctx.set_option("patch_invert_lds", 1)
    for fused in (1, 0):
        ctx.set_option("vanka_fused", fused)
        for solver in ("richardson", "gmres"):
            for n_exact in (0, 5):
                pb = problem(capi.SMOOTH_ASM, states[0])
                mg = pb.prepare(top)
                for l in range(1, nl):
                    if solver == "gmres":
                        mg.set_level_solver(l, "gmres", 30)
                    mg.set_level_patches_exact(l, n_exact)
                mg.setup()
                tag = "asm %s n_exact=%d vanka_fused=%d" % (solver, n_exact, fused)
                rec[tag] = cycle(mg)
                if n_exact == 0:
                    pb.SOL[top].upload(states[1])
                    mg = pb.prepare(top)
                    rec["second preparation " + tag] = cycle(mg)
                pb.destroy()
        # the level operators of the second state installed with set_level on the Multigrid of the first, levels 1 and 2 on padded patterns
        for name, code in (("vanka", capi.SMOOTH_VANKA), ("asm", capi.SMOOTH_ASM)):
            pbs = [problem(code, st) for st in states]
            for pb in pbs:
                pb.prepare(top)
            pb, mg = pbs[0], pbs[0].mg[top]
            rec["%s before set_level vanka_fused=%d" % (name, fused)] = cycle(mg)
            ops = [pbs[1].A[(top, l)].to_scipy() for l in range(nl)]
            dev = [ctx.matrix_scipy(a if l == 0 else padded(a)) for l, a in enumerate(ops)]
            for l in range(nl):
                mg.set_level(l, dev[l], pb.P[l] if l else None, None, code, pb.omega, pb.npre if l else 1, pb.npost if l else 0)
            mg.setup()
            rec["%s after set_level onto padded patterns vanka_fused=%d" % (name, fused)] = cycle(mg)
            for pb in pbs:
                pb.destroy()
            for a in dev:
                a.destroy()
    ctx.set_option("vanka_fused", 1)
    with open(path, "w") as f:
        json.dump({"library": os.environ.get("FEMUS_HIP_LIBRARY", "in-tree"), "device": ctx.device_name(), "records": rec}, f)
    print("patch_bits: %d records written to %s" % (len(rec), path))
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
        cases.append({"case": k, "words": len(ra[k]["x"]), "sha256_of_words": hashlib.sha256(json.dumps(ra[k], sort_keys=True).encode()).hexdigest(),
                      "identical": same})
    distinct = len({c["sha256_of_words"] for c in cases})
    json.dump({"what": "one V(2,2) cycle of the block Schwarz smoothers as uint64 words, parent build against this one (tests/dev/patch_bits.py)",
               "device": A["device"], "cases": len(cases), "distinct_results_among_the_cases": distinct, "words_compared": sum(c["words"] for c in cases),
               "cases_that_differ": differ, "records": cases}, open(out, "w"), indent=1)
    print("patch_bits: %d cases (%d distinct results), %d differ" % (len(cases), distinct, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(*sys.argv[2:5]))
