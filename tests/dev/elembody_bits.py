"""Bit record of the four element bodies of the generic assembler (fh_generic.hip, fh_quasilinear.hip, fh_transient.hip, fh_system.hip), for comparing two
builds of the library (FEMUS_HIP_LIBRARY names the one to load).

    python tests/dev/elembody_bits.py dump OUT.json          one build, in a process of its own
    python tests/dev/elembody_bits.py compare A.json B.json OUT.json

dump: on the meshes of tests/test_gpu_generic_assembler.py (refined once and curved, a few dozen elements) every body on every family at the seventh rule, on
RULE_CASES at the four other rules, through the second builder (from a resident mesh), on 105 tetrahedra (a last workgroup that is not full at 16, 32 and 64
lanes per element) and with debug_poison set before create.  Per assembly: the SHA-256 of KK's values and of RES as 64-bit words, and what info() and the three
*_chunks exports report at that moment.  compare: exits non-zero unless every record of the two is the same."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tobytes()).hexdigest()


def all_bodies(ctx, rec, tag, s, gen, K, with_one_shot=True):
    """every body through `gen` into K (a matrix of s's pattern): the Poisson body and the one-shot call with and without source and state, forms A, B and f
    alone, a theta-step at theta 0, 0.5 and 1, systems of m = 1 .. 4 variables (f alone; form S where m is the dimension; form R at m = 4 in 3-D)"""
    import numpy as np
    import quasilinear_reference as qr
    import system_reference as sr
    from femus_amd import capi
    from test_gpu_generic_assembler import one_shot
    dim, n = s.xs.shape[1], s.ndof

    def put(name, KK, RES):
        k, r = KK.to_scipy().data, RES.to_numpy()
        rec[tag + ": " + name] = {"K": sha(k), "RES": sha(r), "words": int(k.size + r.size), "info": gen.info(), "form_chunks": gen.form_chunks(),
                                  "transient_chunks": gen.transient_chunks(), "system_chunks": {str(m): gen.system_chunks(m) for m in (1, 2, 3, 4)}}

    for name, kw in (("state and source", dict(sol=s.SOL, source=s.f)), ("state", dict(sol=s.SOL)), ("source, sol NULL", dict(source=s.f))):
        gen.assemble(K, s.RES, **kw)
        put("poisson, " + name, K, s.RES)
        if with_one_shot:
            one_shot(ctx, s.geom, s.fe, s.ed, s.xs, s.K2, s.RES2, order=s.order, **kw)
            put("one-shot, " + name, s.K2, s.RES2)
    texts = {"A": qr.with_source(qr.form_a(dim), dim)[0], "B": qr.with_source(qr.form_b(dim), dim)[0], "f": qr.with_source(({}, {}), dim)[0]}
    for name, text in texts.items():
        form = capi.QuasilinearForm(**text)
        gen.assemble_form(K, s.RES, s.SOL, form)
        put("form " + name, K, s.RES)
        form.destroy()
    tform, OLD = capi.TransientForm(**texts["B"]), ctx.vector_from(0.5 * s.u)
    for theta in (0.0, 0.5, 1.0):
        gen.assemble_transient(K, s.RES, s.SOL, OLD, tform, 0.25, 0.125, theta)
        put("transient theta %g" % theta, K, s.RES)
    tform.destroy()
    for m in (1, 2, 3, 4):
        KB = K.block_system(m)
        SOL, RES = ctx.vector_from(np.random.default_rng(11).uniform(-1, 1, m * n)), ctx.vector(m * n)
        forms = {"f": capi.SystemForm(m, f=[texts["f"]["f"]] * m)}
        if m == dim:
            forms["S"] = capi.SystemForm(**sr.form_s(dim)[0])
        if m == 4 and dim == 3:
            forms["R"] = capi.SystemForm(**sr.form_r(dim)[0])
        for name, form in forms.items():
            gen.assemble_system(KB, RES, SOL, form)
            put("system m = %d, form %s" % (m, name), KB, RES)
            form.destroy()
        KB.destroy()


def dump(path):
    import femus_amd
    from femus_amd import capi, mixed_mesh
    from test_gpu_generic_assembler import CASES, FES, GOLDEN, RULES, Setup, curved
    from test_gpu_quasilinear import RULE_CASES, level

    ctx = femus_amd.Context(0)
    rec = {}
    for case in CASES:
        for fe in FES:
            s = Setup(ctx, case, fe, lv=level(case))
            all_bodies(ctx, rec, "%s %s seventh" % (case, fe), s, s.gen, s.K)
            s.close()
    for case, fe in RULE_CASES:
        for order in RULES:
            if order != "seventh":
                s = Setup(ctx, case, fe, order=order, lv=level(case))
                all_bodies(ctx, rec, "%s %s %s" % (case, fe, order), s, s.gen, s.K)
                s.close()
    for case in CASES:                                     # the second builder, as tests/test_gpu_system.py::test_both_builders_give_the_same_bits makes it
        if case == "tri":
            lv = mixed_mesh.tri_box(3, 2, (0., 0.), (1.5, 1.))
        else:
            lv = mixed_mesh.read_gambit(os.path.join(GOLDEN, {"tet": "cube_Tet.neu", "wedge": "cube_Wedge.neu", "mixed3d": "cube_all_shapes_Six_boundary_groups.neu",
                                                              "mixed2d": "square_mixed.neu"}[case]))
        lv = mixed_mesh.refine(*lv[:4])
        s = Setup(ctx, case, "biquadratic", lv=(lv[0], lv[1], lv[2], lv[4]))
        mesh = capi.ElementMesh.from_arrays(ctx, lv[0], lv[1], curved(lv[2]), lv[3], lv[4])
        gd = capi.GenericAssembler.from_mesh(mesh, "biquadratic", s.K2)
        mesh.destroy()
        all_bodies(ctx, rec, "%s biquadratic seventh, from the resident mesh" % case, s, gd, s.K2, with_one_shot=False)
        gd.destroy()
        s.close()
    before = int(os.environ.get("FEMUS_HIP_POISON", "0") or 0)
    for poison in (0, 1):                                  # 105 tetrahedra: no multiple of 16, 8 or 4 elements per workgroup
        for fe in FES:
            ctx.set_option("debug_poison", 1 if poison else before)
            s = Setup(ctx, "tet", fe, refinements=0)
            ctx.set_option("debug_poison", before)
            assert s.ed.shape[0] == 105
            all_bodies(ctx, rec, "105 tetrahedra %s seventh, debug_poison %d" % (fe, poison), s, s.gen, s.K)
            s.close()
    with open(path, "w") as f:
        json.dump({"library": os.environ.get("FEMUS_HIP_LIBRARY", "in-tree"), "device": ctx.device_name(), "records": rec}, f)
    print("elembody_bits: %d records written to %s" % (len(rec), path))
    ctx.close()


def compare(pa, pb, out):
    A, B = json.load(open(pa)), json.load(open(pb))
    ra, rb = A["records"], B["records"]
    assert sorted(ra) == sorted(rb), "the two records hold different cases"
    words, plans, differ = 0, {}, []
    for k in sorted(ra):
        if ra[k] != rb[k]:
            differ.append(k)
        words += ra[k]["words"]
        if k.endswith("system m = 4, form f"):             # the mesh's last record: what its object reports once every body has run on it
            plans[k.split(": ")[0]] = {"elems_per_workgroup": ra[k]["info"]["elems_per_workgroup"], "form_chunks": ra[k]["form_chunks"],
                                       "transient_chunks": ra[k]["transient_chunks"], "system_chunks_and_lanes": ra[k]["system_chunks"]}
    json.dump({"what": "SHA-256 of KK's values and of RES as uint64 words, info() and the chunks and lanes the exports report, for every element body of the "
                       "generic assembler: parent build against this one (tests/dev/elembody_bits.py); a record is identical when all of that is equal",
               "device": A["device"], "cases": len(ra), "words_compared": words, "cases_that_differ": len(differ), "differ": differ,
               "plans": plans}, open(out, "w"), indent=1)
    print("elembody_bits: %d cases, %d differ" % (len(ra), len(differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(*sys.argv[2:5]))
