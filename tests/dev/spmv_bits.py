"""Bit record of the sparse products (fh_spmv.hip), for comparing two builds of the library (FEMUS_HIP_LIBRARY names the one to load).

    python tests/dev/spmv_bits.py dump OUT.json          one build, in a process of its own
    python tests/dev/spmv_bits.py compare A.json B.json OUT.json

dump, as uint64 words:
  - y = Ax, y += Ax, b - Ax and the Jacobi sweep for every (kernel, tile) pair of test_spmv_family_q2_matrix, on the Q2 matrix of that test and on
    the ragged matrix of test_spmv_ragged_rows_and_long_row (tests/test_gpu_algebra.py);
  - the same four for the option cases of test_spmv_instantiation_and_grid_options (spmv_threads 128, spmv_nt 1, spmv_xcd_remap 0 / 1);
  - a walk through (spmv_kernel, spmv_tile) settings on ONE matrix object, every change made both ways, so that every rebuild path of the plan is crossed
    (row blocks of kernel 4 serving kernel 3 and not the other way round, kernels 0 and 2 taking only their own);
  - fh_spmv_expected_bytes and fh_mat_split_info for two values of n_own asked in alternation on one matrix, with a change of tile in between;
  - the ghosted product of tests/test_gpu_halo_overlap.py (interior blocks, exchange, interface blocks) in the four modes, with and without the overlap;
  - one V(2,2) cycle of the benchmark's multigrid (Q2 Poisson, Galerkin coarse operators) on 2^3 -> 8^3 elements, prepared twice on an unchanged
    hierarchy, and how often the cycle was captured during the two preparations.  No export reports a replay; the count is taken from the
    "capture_cycle" lines of FEMUS_HIP_TRACE=1 in a child process (1: the second preparation kept the captured cycle).
compare: exits non-zero unless every word of the two records is the same."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

Q2_PAIRS = [(4, 1024), (4, 2048), (3, 2048), (3, 1024), (3, 4096), (0, 1024), (0, 2048), (0, 4096), (1, 2048), (2, 256), (2, 512), (2, 1024)]
OPTION_CASES = [(3, 1024, "spmv_threads", 128), (3, 2048, "spmv_threads", 128), (2, 256, "spmv_nt", 1), (2, 1024, "spmv_nt", 1),
                (0, 1024, "spmv_xcd_remap", 0), (0, 1024, "spmv_xcd_remap", 1), (3, 1024, "spmv_xcd_remap", 0), (3, 1024, "spmv_xcd_remap", 1),
                (4, 1024, "spmv_xcd_remap", 0), (4, 1024, "spmv_xcd_remap", 1)]
OPTION_DEFAULTS = {"spmv_threads": 256, "spmv_nt": 0, "spmv_xcd_remap": 32}
WALK = [(3, 2048), (3, 1024), (3, 2048), (4, 2048), (3, 2048), (4, 1024), (4, 2048), (2, 1024), (3, 1024), (2, 1024), (2, 512), (0, 1024), (3, 1024),
        (0, 1024), (0, 2048), (4, 2048), (0, 2048), (1, 2048), (3, 2048)]


def words(a):
    import numpy as np
    return [int(w) for w in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)]


def ragged_matrix():
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    m, n = 777, 5000
    rows, cols, vals = [], [], []
    for i in range(m):
        k = 4500 if i == 400 else [0, 1, 3, 64, 130][i % 5]
        c = np.sort(rng.choice(n, size=k, replace=False))
        rows += [i] * k
        cols += c.tolist()
        vals += rng.uniform(-1, 1, k).tolist()
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, n))


def option_matrix():
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.default_rng(2049)
    n, per = 2049, 64
    indices = np.concatenate([np.sort(rng.choice(n, size=per, replace=False)) for _ in range(n)]).astype(np.int32)
    return sp.csr_matrix((rng.uniform(-1, 1, n * per), indices, np.arange(n + 1) * per), shape=(n, n))


def halo_operator(rng, n_own, n_ghost, ghost_rows):
    import numpy as np
    import scipy.sparse as sp
    rows, cols, vals = [], [], []
    for i in range(n_own):
        c = rng.choice(n_own, size=rng.integers(3, 40), replace=False)
        if i in ghost_rows:
            c = np.concatenate([c, n_own + rng.choice(n_ghost, size=5, replace=False)])
        rows += [i] * c.size
        cols += list(c)
        vals += list(rng.uniform(-1, 1, c.size))
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n_own, n_own + n_ghost))
    A.sort_indices()
    return A


class _SelfComm:
    def alltoallv(self, arrays, dtype):
        import numpy as np
        return [np.array(a, dtype=dtype, copy=True) for a in arrays]

    def allreduce_sum(self, a):
        import numpy as np
        return np.array(a, copy=True)


def cycle(path):
    """the child of dump: two preparations of an unchanged hierarchy, a cycle after each"""
    import femus_amd
    from femus_amd.poisson import PoissonMG
    ctx = femus_amd.Context(0)
    pb = PoissonMG(ctx, 2, 2, 2, 3, fe="biquadratic", order="seventh", omega=2. / 3., npre=2, npost=2, coarse="galerkin", source_kind=0, params=(1.0,)).init()
    out = []
    for _ in range(2):
        pb.assemble()
        pb.prepare()
        pb.zero_boundary_residuals()
        pb.vcycle()
        out += words(pb.EPSC.to_numpy())
    with open(path, "w") as f:
        json.dump(out, f)
    pb.destroy()
    ctx.close()


def dump(path):
    import numpy as np
    rec = {}
    # the cycle first, in a child with the set-up trace on, before this process opens the device
    tmp = path + ".cycle"
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "cycle", tmp], env=dict(os.environ, FEMUS_HIP_TRACE="1"), stderr=subprocess.PIPE,
                           text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-3000:]
    rec["V(2,2) cycle after each of two preparations"] = {"x": json.load(open(tmp))}
    os.remove(tmp)
    rec["captures of the cycle during the two preparations"] = {"x": [sum("capture_cycle: warm-up" in l for l in child.stderr.splitlines())]}

    import femus_amd
    from femus_amd import capi
    from oracle import femus_oracle as fo
    ctx = femus_amd.Context(0)

    def four_modes(M, A, seed):
        m, n = A.shape
        rng = np.random.default_rng(seed)
        xs, bs, y0, dinv = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(0.5, 2.0, m)
        x, b, d, y = ctx.vector_from(xs), ctx.vector_from(bs), ctx.vector_from(dinv), ctx.vector_from(y0)
        out = []
        y.add_vector(x, M)
        out += words(y.to_numpy())
        y.matrix_mult(x, M)
        out += words(y.to_numpy())
        y.resid(b, x, M)
        out += words(y.to_numpy())
        y.jacobi_sweep(b, x, M, d, 0.7)
        out += words(y.to_numpy())
        assert np.isfinite(y.to_numpy()).all()
        for v in (x, b, d, y):
            v.destroy()
        return {"x": out}

    ms = fo.build_levels(2, 2, 2, 3)
    Q2, _ = fo.assemble_poisson(ms[-1], "biquadratic", lambda xg: np.ones(xg.shape[:2]))
    Q2 = Q2.tocsr()
    mats = {"Q2": Q2, "ragged": ragged_matrix()}
    for kernel, tile in Q2_PAIRS:
        ctx.set_option("spmv_kernel", kernel)
        ctx.set_option("spmv_tile", tile)
        for name, A in mats.items():
            M = ctx.matrix_scipy(A)
            rec["%s kernel=%d tile=%d" % (name, kernel, tile)] = four_modes(M, A, 11)
            M.destroy()
    A = option_matrix()
    for kernel, tile, option, value in OPTION_CASES:
        ctx.set_option("spmv_kernel", kernel)
        ctx.set_option("spmv_tile", tile)
        ctx.set_option(option, value)
        M = ctx.matrix_scipy(A)
        rec["option matrix kernel=%d tile=%d %s=%d" % (kernel, tile, option, value)] = four_modes(M, A, 12)
        M.destroy()
        ctx.set_option(option, OPTION_DEFAULTS[option])
    for name, A in mats.items():
        ctx.set_option("spmv_kernel", 3)
        ctx.set_option("spmv_tile", 2048)
        M = ctx.matrix_scipy(A)
        for step, (kernel, tile) in enumerate(WALK):
            ctx.set_option("spmv_kernel", kernel)
            ctx.set_option("spmv_tile", tile)
            rec["%s walk step %02d kernel=%d tile=%d" % (name, step, kernel, tile)] = four_modes(M, A, 13)
        M.destroy()
    # the ghosted operator of tests/test_gpu_halo_overlap.py
    ctx.set_option("spmv_kernel", 3)
    ctx.set_option("spmv_tile", 2048)
    rng = np.random.default_rng(7)
    n_own, n_ghost = 6000, 500
    A_h = halo_operator(rng, n_own, n_ghost, set(range(5200, 6000)) | set(range(100, 110)))
    M = ctx.matrix_scipy(A_h)
    asked = []
    for tile in (2048, 1024, 2048):
        ctx.set_option("spmv_tile", tile)
        for n_own_cols in (n_own, 3000, n_own, 3000):
            asked += list(M.split_info(n_own_cols)) + list(M.spmv_expected_bytes(3)) + list(M.spmv_expected_bytes(0))
    rec["split_info and expected_bytes, n_own 6000 / 3000 in alternation, tiles 2048 / 1024 / 2048"] = {"x": [int(v) for v in asked]}
    send_idx = rng.choice(n_own, size=n_ghost, replace=False).astype(np.int32)
    halo = capi.Halo.host(ctx, 0, 1, _SelfComm(), [n_ghost], send_idx, [n_ghost])
    x = ctx.vector(n_own + n_ghost, n_own, 0, np.arange(n_own, n_own + n_ghost, dtype=np.int32))
    xo, y0 = rng.uniform(-1, 1, n_own), rng.uniform(-1, 1, n_own)
    x.upload(xo)
    b, dinv, y = ctx.vector_from(rng.uniform(-1, 1, n_own)), ctx.vector_from(rng.uniform(0.5, 2, n_own)), ctx.vector(n_own)
    for overlap in (1, 0):
        ctx.set_option("halo_overlap", overlap)
        out = []
        for mode in range(4):
            y.upload(y0)
            halo.spmv(M, x, y, mode, b if mode >= 2 else None, dinv if mode == 3 else None, 0.7)
            out += words(y.to_numpy())
        rec["ghosted product, four modes, halo_overlap=%d" % overlap] = {"x": out}
    ctx.set_option("halo_overlap", 1)
    halo.destroy()
    M.destroy()
    with open(path, "w") as f:
        json.dump({"library": os.environ.get("FEMUS_HIP_LIBRARY", "in-tree"), "device": ctx.device_name(), "records": rec}, f)
    print("spmv_bits: %d records written to %s" % (len(rec), path))
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
    captures = ra["captures of the cycle during the two preparations"]["x"][0]
    json.dump({"what": "the sparse products as uint64 words, parent build against this one (tests/dev/spmv_bits.py)",
               "device": A["device"], "cases": len(cases), "distinct_results_among_the_cases": distinct, "words_compared": sum(c["words"] for c in cases),
               "cases_that_differ": differ, "captures_of_the_cycle_during_two_preparations_parent": captures,
               "captures_of_the_cycle_during_two_preparations_this_build": rb["captures of the cycle during the two preparations"]["x"][0],
               "records": cases}, open(out, "w"), indent=1)
    print("spmv_bits: %d cases (%d distinct results), %d differ" % (len(cases), distinct, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif sys.argv[1] == "cycle":
        cycle(sys.argv[2])
    else:
        sys.exit(compare(*sys.argv[2:5]))
