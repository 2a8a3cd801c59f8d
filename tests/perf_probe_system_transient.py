"""Dev probe, not a test: what the theta-step of a system (capi.GenericAssembler.assemble_system_transient) costs next to the stationary system body with the
same programs on the same object, on cube_Tet.neu refined four times as TET15 (430 080 elements, the mesh and settings of tests/perf_probe_system.py), the
31-point rule, in one process:

  system_m{1,2,3}              assemble_system with the forms of tests/perf_probe_system.py: the yardstick of this run
  step_m{1,2,3}_theta1         assemble_system_transient with the same programs, M = 1, theta = 1 (nothing evaluated at the old state)
  step_m{1,2,3}_theta05        the same at theta = 0.5 (f, c and A once more at the old state)
  transient_m1_theta{1,05}     assemble_transient with form B as a scalar form: the scalar theta-step, for m = 1

  python tests/perf_probe_system_transient.py [--out FILE] [--m 1 2 3]     medians of 11 calls, each ended by a synchronisation
                                                                            -> profiles/system_transient_probe.json
--m restricts the systems that run (a kernel trace of one m at a time: the kernels of all m have one name)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "system_transient_probe.json")
TIME, DT = 0.7, 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--refinements", type=int, default=4)
    ap.add_argument("--m", type=int, nargs="*", default=[1, 2, 3])
    a = ap.parse_args()
    import femus_amd
    import system_reference as sr
    from femus_amd import capi, mixed_mesh
    from perf_probe_quasilinear import wall
    ctx = femus_amd.Context(0)
    lv = mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", "cube_Tet.neu"))
    for _ in range(a.refinements):
        lv = mixed_mesh.refine(*lv[:4])
    ed, xs, ndof = lv[1][:, :mixed_mesh.CLASSES["tet"][2]], lv[2], lv[4][2]
    print("%d elements, %d dofs" % (ed.shape[0], ndof), flush=True)
    S = capi.Mat.from_elements(ctx, ed, ndof)
    gen = capi.GenericAssembler(ctx, "tet", "biquadratic", lv[1][:, :mixed_mesh.NLOC["tet"]], xs, S)
    text_b = dict(f="exp(x)*(1+y)-z", a="1+u*u", a_u="2*u", c="sqrt(1+u*u)", c_u="u/sqrt(1+u*u)")
    form_b = capi.QuasilinearForm(**text_b)
    forms = {1: capi.SystemForm(**sr.scalar_texts([text_b])),
             2: capi.SystemForm(2, f=[None, "-4*pi*pi*pi*pi*cos(pi*x)*cos(pi*y)"], c=["u1", None], c_u=[[None, "1"], [None, None]]),
             3: capi.SystemForm(**sr.form_s(3)[0])}
    rng = np.random.default_rng(3)
    u, uo = rng.uniform(-1, 1, 3 * ndof), rng.uniform(-1, 1, 3 * ndof)
    out = {"nel": int(ed.shape[0]), "ndof": int(ndof), "calls": 11, "nnz_scalar": int(S.nnz), "time": TIME, "dt": DT}
    for m in a.m:
        K = S.block_system(m) if m > 1 else S
        SOL, OLD, RES = ctx.vector_from(u[:m * ndof]), ctx.vector_from(uo[:m * ndof]), ctx.vector(m * ndof)
        base = "system_m%d" % m
        out[base] = wall(ctx, lambda: gen.assemble_system(K, RES, SOL, forms[m]))
        out[base]["gauss_chunk_and_lanes"] = gen.system_chunks(m)
        out[base]["programs"] = len(forms[m].exprs)
        print(base, out[base], flush=True)
        for theta, tag in ((1.0, "theta1"), (0.5, "theta05")):
            key = "step_m%d_%s" % (m, tag)
            out[key] = wall(ctx, lambda: gen.assemble_system_transient(K, RES, SOL, OLD, forms[m], TIME, DT, theta))
            out[key]["over_system"] = out[key]["median_ms"] / out[base]["median_ms"]
            out[key]["gauss_chunk_and_lanes"] = gen.system_transient_chunks(m)
            print(key, out[key], flush=True)
            if m == 1:
                tkey = "transient_m1_%s" % tag
                out[tkey] = wall(ctx, lambda: gen.assemble_transient(S, RES, SOL, OLD, form_b, TIME, DT, theta))
                out[key]["over_transient"] = out[key]["median_ms"] / out[tkey]["median_ms"]
                print(tkey, out[tkey], "step over transient %.3f" % out[key]["over_transient"], flush=True)
        for q in (SOL, OLD, RES) + ((K,) if m > 1 else ()):
            q.destroy()
    out["info"] = gen.info()
    for q in [gen, form_b, S] + list(forms.values()):
        q.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
