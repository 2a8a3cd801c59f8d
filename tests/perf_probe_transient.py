"""Dev probe, not a test: what the transient element body (capi.GenericAssembler.assemble_transient) costs next to the quasilinear body of the same object, on
cube_Tet.neu refined four times as TET15 (430 080 elements, the mesh of tests/perf_probe_quasilinear.py), the 31-point rule, form B's programs
(a = 1 + u^2, a_u = 2 u, c = sqrt(1 + u^2), c_u = u / sqrt(1 + u^2), f = exp(x) (1 + y) - z), in one process and one run:

  form_B               assemble_form: the yardstick of this run
  transient_theta_1    assemble_transient with theta = 1: the mass term, u - uo, nothing evaluated at the old state
  transient_theta_05   assemble_transient with theta = 0.5: f, a, c and the gradient at the old state as well
and after it, under "other_families", the same three on the same mesh as TET10 (32 lanes per element) and TET4 (16 lanes).

  python tests/perf_probe_transient.py [--out FILE]        medians of 11 calls, each ended by a synchronisation -> profiles/transient_probe.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "transient_probe.json")


def main():
    from perf_probe_quasilinear import wall
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
    xs = lv[2]
    form = capi.QuasilinearForm(f="exp(x)*(1+y)-z", a="1+u*u", a_u="2*u", c="sqrt(1+u*u)", c_u="u/sqrt(1+u*u)")

    def family(fe):
        k = {"linear": 0, "serendipity": 1, "biquadratic": 2}[fe]
        ed, ndof = lv[1][:, :mixed_mesh.CLASSES["tet"][k]], lv[4][k]
        print("%s: %d elements, %d dofs" % (fe, ed.shape[0], ndof), flush=True)
        K = capi.Mat.from_elements(ctx, ed, ndof)
        rng = np.random.default_rng(3)
        SOL, OLD, RES = ctx.vector_from(rng.uniform(-1, 1, ndof)), ctx.vector_from(rng.uniform(-1, 1, ndof)), ctx.vector(ndof)
        gen = capi.GenericAssembler(ctx, "tet", fe, lv[1][:, :mixed_mesh.NLOC["tet"]], xs, K)
        out = {"nel": int(ed.shape[0]), "ndof": int(ndof), "calls": 11}
        out["form_B"] = wall(ctx, lambda: gen.assemble_form(K, RES, SOL, form))
        out["transient_theta_1"] = wall(ctx, lambda: gen.assemble_transient(K, RES, SOL, OLD, form, 0.7, 0.05, 1.0))
        out["transient_theta_05"] = wall(ctx, lambda: gen.assemble_transient(K, RES, SOL, OLD, form, 0.7, 0.05, 0.5))
        out["ratio_theta_1"] = out["transient_theta_1"]["median_ms"] / out["form_B"]["median_ms"]
        out["ratio_theta_05"] = out["transient_theta_05"]["median_ms"] / out["form_B"]["median_ms"]
        out["info"] = gen.info()
        out["gauss_chunk_form"], out["gauss_chunk_transient"] = gen.form_chunks(), gen.transient_chunks()
        for q in (gen, K, SOL, OLD, RES):
            q.destroy()
        return out

    out = family("biquadratic")                                    # TET15: the figures that are quoted
    out["other_families"] = {fe: family(fe) for fe in ("serendipity", "linear")}        # TET10 at L = 32, TET4 at L = 16: same mesh, same run
    form.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
