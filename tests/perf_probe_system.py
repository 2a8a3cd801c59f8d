"""Dev probe, not a test: what the system element body (capi.GenericAssembler.assemble_system) costs next to the scalar form body of the same object, on
cube_Tet.neu refined four times as TET15 (430 080 elements, the mesh of tests/perf_probe_quasilinear.py), the 31-point rule, in one process:

  form_B            assemble_form with form B (a = 1 + u^2, a_u = 2 u, c = sqrt(1 + u^2), c_u = u / sqrt(1 + u^2)): the yardstick of this run
  system_m1         assemble_system with the same form as a system of one variable
  system_m2         ex04 with the rows exchanged (row 0: -lap u + v = 0, row 1: -lap v = -f)
  system_m3         form S of tests/system_reference.py (a viscous Burgers system with cross-diffusion)

  python tests/perf_probe_system.py [--out FILE] [--m 1 2 3]     medians of 11 calls, each ended by a synchronisation -> profiles/system_probe.json
--m restricts the systems that run (a kernel trace of one m at a time: the kernels of all m have one name)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "system_probe.json")


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
    u = np.random.default_rng(3).uniform(-1, 1, 3 * ndof)
    SOL1, RES1 = ctx.vector_from(u[:ndof]), ctx.vector(ndof)
    out = {"nel": int(ed.shape[0]), "ndof": int(ndof), "calls": 11, "nnz_scalar": int(S.nnz)}
    out["form_B"] = wall(ctx, lambda: gen.assemble_form(S, RES1, SOL1, form_b))
    print("form_B", out["form_B"], flush=True)
    for m in a.m:
        K = S.block_system(m) if m > 1 else S
        SOL, RES = ctx.vector_from(u[:m * ndof]), ctx.vector(m * ndof)
        key = "system_m%d" % m
        out[key] = wall(ctx, lambda: gen.assemble_system(K, RES, SOL, forms[m]))
        out[key]["factor"] = out[key]["median_ms"] / out["form_B"]["median_ms"]
        out[key]["gauss_chunk_and_lanes"] = gen.system_chunks(m)
        out[key]["programs"] = len(forms[m].exprs)
        print(key, out[key], flush=True)
        for q in (SOL, RES) + ((K,) if m > 1 else ()):
            q.destroy()
    out["info"] = gen.info()
    out["gauss_chunk_form"] = gen.form_chunks()
    for q in [gen, form_b, S] + list(forms.values()):
        q.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
