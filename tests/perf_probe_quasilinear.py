"""Dev probe, not a test: what the quasilinear element body (capi.GenericAssembler.assemble_form) costs next to the Poisson body of the same object, on
cube_Tet.neu refined four times as TET15 (430 080 elements, the mesh of tests/perf_probe_generic_assembler.py), in one process:

  assemble          the Poisson path (k_gen_pairs + k_gen_rows): the yardstick of this run
  form_f            assemble_form with f alone: the same equation through the nc x nc body -- the cost of the layout
  form_B            assemble_form with form B (a = 1 + u^2, a_u = 2 u, c = sqrt(1 + u^2), c_u = u / sqrt(1 + u^2)) -- layout and programs

  python tests/perf_probe_quasilinear.py [--out FILE]        medians of 11 calls, each ended by a synchronisation -> profiles/quasilinear_probe.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "quasilinear_probe.json")


def wall(ctx, fn, warm=3, reps=11):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--refinements", type=int, default=4)
    a = ap.parse_args()
    import femus_amd
    from femus_amd import capi, mixed_mesh
    ctx = femus_amd.Context(0)
    lv = mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", "cube_Tet.neu"))
    for _ in range(a.refinements):
        lv = mixed_mesh.refine(*lv[:4])
    ed, xs, ndof = lv[1][:, :mixed_mesh.CLASSES["tet"][2]], lv[2], lv[4][2]
    print("%d elements, %d dofs" % (ed.shape[0], ndof), flush=True)
    K = capi.Mat.from_elements(ctx, ed, ndof)
    SOL, RES = ctx.vector_from(np.random.default_rng(3).uniform(-1, 1, ndof)), ctx.vector(ndof)
    gen = capi.GenericAssembler(ctx, "tet", "biquadratic", lv[1][:, :mixed_mesh.NLOC["tet"]], xs, K)
    f = capi.Expr("exp(x)*(1+y)-z", "x,y,z,t")
    form_f = capi.QuasilinearForm(f="exp(x)*(1+y)-z")
    form_b = capi.QuasilinearForm(f="exp(x)*(1+y)-z", a="1+u*u", a_u="2*u", c="sqrt(1+u*u)", c_u="u/sqrt(1+u*u)")
    out = {"nel": int(ed.shape[0]), "ndof": int(ndof), "calls": 11}
    out["assemble"] = wall(ctx, lambda: gen.assemble(K, RES, sol=SOL, source=f))
    out["form_f"] = wall(ctx, lambda: gen.assemble_form(K, RES, SOL, form_f))
    out["form_B"] = wall(ctx, lambda: gen.assemble_form(K, RES, SOL, form_b))
    out["factor_form_f"] = out["form_f"]["median_ms"] / out["assemble"]["median_ms"]
    out["factor_form_B"] = out["form_B"]["median_ms"] / out["assemble"]["median_ms"]
    out["info"] = gen.info()
    out["gauss_chunk"] = gen.form_chunks()
    for q in (gen, f, form_f, form_b, K):
        q.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
