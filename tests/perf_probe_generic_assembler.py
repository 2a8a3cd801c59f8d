"""Dev probe: the resident generic assembler (capi.GenericAssembler) against the one-shot calls on the same inputs -- cube_Tet.neu refined three and four times
as TET15 (53 760 / 430 080 elements) and the mixed cube refined three times (biquadratic).

  python tests/perf_probe_generic_assembler.py                       wall times (warm-up, repeats, spread) -> profiles/generic_assembler_probe.json
  rocprofv3 --kernel-trace --stats -d DIR -o ga -- python tests/perf_probe_generic_assembler.py --trace tet3
                                                                     N calls of each path on one mesh, for the kernel share
  python tests/perf_probe_generic_assembler.py --merge DIR           kernel times per call out of the stats files under DIR into the same JSON

Wall time: the call and the synchronisation after it (the one-shot call synchronises itself); `stream` is the resident path enqueued N times before one
synchronisation.  hbm_fraction = algorithmic_bytes / time / 8 TB/s."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "generic_assembler_probe.json")
MESHES = {"tet3": ("cube_Tet.neu", 3), "tet4": ("cube_Tet.neu", 4), "mixed3": ("cube_all_shapes_Six_boundary_groups.neu", 3)}
N_TRACE = 10
HBM = 8e12


def build(ctx, name, pack=1):
    from femus_amd import capi, mixed_mesh
    fname, nref = MESHES[name]
    lv = mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", fname))
    for _ in range(nref):
        lv = mixed_mesh.refine(*lv[:4])
    kind, ed, xs, own = lv[0], lv[1], lv[2], lv[4]
    ndof = own[2]
    shapes = sorted(set(kind.tolist()))
    eds = [ed[kind == s][:, :mixed_mesh.CLASSES[s][2]] for s in shapes]
    width = max(e.shape[1] for e in eds)
    table = np.concatenate([np.concatenate([e, np.broadcast_to(e[:, :1], (e.shape[0], width - e.shape[1]))], axis=1) for e in eds])
    K = capi.Mat.from_elements(ctx, table, ndof)
    geom, edc = (shapes[0], ed[:, :mixed_mesh.NLOC[shapes[0]]]) if len(shapes) == 1 else (kind, ed)
    SOL, RES = ctx.vector_from(np.random.default_rng(3).uniform(-1, 1, ndof)), ctx.vector(ndof)
    f = capi.Expr("exp(x)*(1+y)-z", "x,y,z,t")
    ctx.set_option("generic_pack", pack)
    t0 = time.perf_counter()
    gen = capi.GenericAssembler(ctx, geom, "biquadratic", edc, xs, K)
    ctx.sync()
    create_ms = (time.perf_counter() - t0) * 1e3
    ctx.set_option("generic_pack", 1)

    def one_shot():
        if isinstance(geom, str):
            capi.assemble_poisson_rows(ctx, geom, "biquadratic", edc, xs, K, RES, sol=SOL, source=f)
        else:
            capi.assemble_poisson_mixed(ctx, "biquadratic", geom, edc, xs, K, RES, sol=SOL, source=f)

    def resident():
        gen.assemble(K, RES, sol=SOL, source=f)

    return {"nel": int(ed.shape[0]), "ndof": int(ndof), "nnz": int(K.to_scipy().nnz) if ed.shape[0] < 100000 else None, "create_ms": create_ms, "gen": gen,
            "one_shot": one_shot, "resident": resident}


def wall(ctx, fn, warm=3, reps=9):
    for _ in range(warm):
        fn()
    ctx.sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}


def load():
    return json.load(open(OUT)) if os.path.exists(OUT) else {}


def save(d):
    with open(OUT, "w") as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace")
    ap.add_argument("--merge")
    ap.add_argument("--meshes", default="tet3,tet4,mixed3")
    a = ap.parse_args()
    if a.merge:
        out = load()
        for name in MESHES:
            files = glob.glob(os.path.join(a.merge, "**", "*%s*kernel_stats.csv" % name), recursive=True)
            if not files:
                continue
            ns = {"one_shot": 0.0, "resident": 0.0}
            per = {}
            for row in csv.DictReader(open(files[0])):
                kn = row["Name"]
                path = "one_shot" if ("k_poisson_pairs_generic" in kn or "k_poisson_rows_generic" in kn) else "resident" if ("k_gen_pairs" in kn or "k_gen_rows" in kn) else None
                if path:
                    ns[path] += float(row["TotalDurationNs"])
                    per[kn.split("(")[0][:60]] = float(row["TotalDurationNs"]) / N_TRACE / 1e6
            m = out.setdefault(name, {})
            m["kernel_ms_per_call"] = {k: v / N_TRACE / 1e6 for k, v in ns.items()}
            m["kernels_ms_per_call"] = per
            if "algorithmic_bytes" in m and ns["resident"] > 0:
                m["hbm_fraction_kernel"] = m["algorithmic_bytes"] / (ns["resident"] / N_TRACE / 1e9) / HBM
        save(out)
        print(json.dumps(out, indent=1, sort_keys=True))
        return
    import femus_amd
    ctx = femus_amd.Context(0)
    if a.trace:
        p = build(ctx, a.trace)
        for fn in (p["one_shot"], p["resident"]):
            for _ in range(N_TRACE):
                fn()
            ctx.sync()
        return
    out = load()
    for name in a.meshes.split(","):
        p = build(ctx, name)
        info = p["gen"].info()
        m = out.setdefault(name, {})
        m.update({"nel": p["nel"], "ndof": p["ndof"], "create_ms": p["create_ms"], "elems_per_workgroup": info["elems_per_workgroup"],
                  "algorithmic_bytes": info["algorithmic_bytes"], "device_bytes": info["device_bytes"]})
        m["wall_one_shot"] = wall(ctx, p["one_shot"])
        m["wall_resident"] = wall(ctx, p["resident"])

        def stream():
            for _ in range(N_TRACE):
                p["resident"]()
        s = wall(ctx, stream, warm=1, reps=5)
        m["wall_resident_stream_per_call"] = {k: v / N_TRACE for k, v in s.items()}
        m["hbm_fraction_wall"] = info["algorithmic_bytes"] / (m["wall_resident_stream_per_call"]["median_ms"] / 1e3) / HBM
        p["gen"].destroy()
        print(name, json.dumps(m, sort_keys=True), flush=True)
        save(out)


if __name__ == "__main__":
    main()
