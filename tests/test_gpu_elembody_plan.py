"""The launch geometry the four element bodies of the generic assembler choose (gp_plan_body, femus_amd/csrc/fh_generic.hip): lanes per element and Gauss
points per LDS chunk, held against a restatement of the rules from the headers of the four files.  The values of an assembly do not depend on the chunk -- every
body gives the same bits whatever it is -- so a chunk or a lane count that silently shrinks would cost speed and fail no other test.

Restated here, per element at nc nodes and a chunk of gc points, in doubles of LDS:
    Poisson    nc 4 + gc 14 + gc nc 3
    form       nc 4 + gc 21 + gc nc 5
    transient  nc 5 + gc 28 + gc nc 5
    system     nc (3 + m) + gc (13 + 6 m + 8 m^2) + gc nc 3
A workgroup of 256 threads holds 256 / L elements and at most 64 KB.  The chunk starts at min(ng, 32).  Halving rule (Poisson, form, system): gc -> (gc + 1) / 2
until the workgroup fits.  Evened rule (transient): gc -> gc - 1 until it fits, then the ng points are spread evenly over the chunks that makes.  Lanes: 16 / 32 /
64 by the nc (nc + 1) / 2 pairs of the Poisson body (<= 32, <= 64, more); the form and transient bodies run on the same lanes, the system body on 1 / 2 / 4 / 4
times as many for m = 1 / 2 / 3 / 4, at most 64.

What is held against the object: the chunks of the form, the transient and the system body, the system body's lanes, and the Poisson body's lanes through
elems_per_workgroup of info().  The Poisson body's own chunk is restated for the arithmetic test only: no export reports it, so the object's is NOT checked.
The lanes are those of the context's default, generic_pack = 1."""
import pytest

import quasilinear_reference as qr
from femus_amd import mixed_mesh
from test_gpu_generic_assembler import FAM, RULES, Setup
from test_gpu_quasilinear import RULE_CASES, level

BUDGET = 64 * 1024
DOUBLES = {"poisson": lambda nc, gc: nc * 4 + gc * 14 + gc * nc * 3,
           "form": lambda nc, gc: nc * 4 + gc * 21 + gc * nc * 5,
           "transient": lambda nc, gc: nc * 5 + gc * 28 + gc * nc * 5}


def system_doubles(m):
    return lambda nc, gc: nc * (3 + m) + gc * (13 + 6 * m + 8 * m * m) + gc * nc * 3


def poisson_lanes(nc):
    npair = nc * (nc + 1) // 2
    return 16 if npair <= 32 else 32 if npair <= 64 else 64


def system_lanes(nc, m):
    return min(64, poisson_lanes(nc) * {1: 1, 2: 2, 3: 4, 4: 4}[m])


def chunk(doubles, nc, ng, lanes, evened=False):
    """the restated rule; the shape fits at the chunk it returns"""
    fits = lambda gc: (256 // lanes) * doubles(nc, gc) * 8 <= BUDGET
    gc = min(ng, 32)
    while gc > 1 and not fits(gc):
        gc = gc - 1 if evened else (gc + 1) // 2
    assert fits(gc)
    if evened:
        nchunk = -(-ng // gc)
        gc = -(-ng // nchunk)
    return gc


def expected(shapes, fe, order):
    """{shape: (nc, ng)} of a mesh's shapes, then every figure the exports report"""
    from femus_amd import capi
    sizes = {s: (mixed_mesh.CLASSES[s][FAM[fe]], len(capi.fe_gauss(s, order)[0])) for s in shapes}
    want = {"elems_per_workgroup": {s: 256 // poisson_lanes(nc) for s, (nc, ng) in sizes.items()},
            "form": {s: chunk(DOUBLES["form"], nc, ng, poisson_lanes(nc)) for s, (nc, ng) in sizes.items()},
            "transient": {s: chunk(DOUBLES["transient"], nc, ng, poisson_lanes(nc), evened=True) for s, (nc, ng) in sizes.items()}}
    for m in (1, 2, 3, 4):
        want["system", m] = {s: (chunk(system_doubles(m), nc, ng, system_lanes(nc, m)), system_lanes(nc, m)) for s, (nc, ng) in sizes.items()}
    return want


def test_the_restatement_gives_a_chunk_for_every_case_listed():
    """plain arithmetic on the sizes of every shape, family and rule below (largest: WEDGE21 and TET15 at the ninth rule): at least one point fits everywhere"""
    from femus_amd import capi
    for shape, classes in mixed_mesh.CLASSES.items():
        for nc in classes:
            for order in RULES:
                ng = len(capi.fe_gauss(shape, order)[0])
                assert chunk(DOUBLES["poisson"], nc, ng, poisson_lanes(nc)) >= 1
                assert chunk(DOUBLES["form"], nc, ng, poisson_lanes(nc)) >= 1
                assert chunk(DOUBLES["transient"], nc, ng, poisson_lanes(nc), evened=True) >= 1
                for m in (1, 2, 3, 4):
                    assert chunk(system_doubles(m), nc, ng, system_lanes(nc, m)) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("order", RULES)
@pytest.mark.parametrize("case,fe", RULE_CASES)
def test_chunks_and_lanes_of_every_body_are_the_restated_ones(ctx, case, fe, order):
    from femus_amd import capi
    s = Setup(ctx, case, fe, order=order, lv=level(case))
    dim = s.xs.shape[1]
    f = qr.with_source(({}, {}), dim)[0]["f"]
    form, OLD = capi.QuasilinearForm(f=f, a="1"), ctx.vector_from(0.5 * s.u)
    made = [form]
    try:
        want = expected(s.gen.shapes, fe, order)
        assert s.gen.info()["elems_per_workgroup"] == want["elems_per_workgroup"]
        assert all(gc == 0 for gc in s.gen.form_chunks().values()) and all(gc == 0 for gc in s.gen.transient_chunks().values())      # no such call yet
        s.gen.assemble_form(s.K, s.RES, s.SOL, form)
        s.gen.assemble_transient(s.K, s.RES, s.SOL, OLD, form, 0.25, 0.125, 0.5)
        print(case, fe, order, "form", s.gen.form_chunks(), "transient", s.gen.transient_chunks(), end=" ")
        assert s.gen.form_chunks() == want["form"]
        assert s.gen.transient_chunks() == want["transient"]
        for m in (1, 2, 3, 4):
            K, one = s.K.block_system(m), capi.SystemForm(m, f=[f] * m)
            made += [K, one]
            s.gen.assemble_system(K, ctx.vector(m * s.ndof), ctx.vector(m * s.ndof), one)
            print("m = %d" % m, s.gen.system_chunks(m), end=" ")
            assert s.gen.system_chunks(m) == want["system", m]
        assert s.gen.info()["elems_per_workgroup"] == want["elems_per_workgroup"]
    finally:
        for x in made:
            x.destroy()
        s.close()
