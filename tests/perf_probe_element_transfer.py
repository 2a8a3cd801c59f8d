"""Dev probe: the transfers and Dirichlet lists of element meshes built on the device (capi.ElementMesh.prolongator / boundary_dofs) against the host builders
of app_poisson.run_elements in the same process -- the TET15 chain of cube_Tet.neu (105 elements) up to 53 760 -> 430 080 elements and the mixed cube (20
hexahedra, tetrahedra and prisms) one level less, biquadratic.

  python tests/perf_probe_element_transfer.py                  one JSON line; also written to profiles/element_transfer_probe.json
  rocprofv3 --kernel-trace --stats -d DIR -o et -- python tests/perf_probe_element_transfer.py --device-only
                                                               the device builds alone, for the kernel share

Per transfer (the number of fine elements is the key): host_ms = _prolongator_from_children with its Mat.from_csr upload; device_ms = ElementMesh.prolongator and
the synchronisation after it (the second of two builds; the first, which loads the code objects, is kept as first_ms).  Per level: bdc_host_ms = the face loop
of run_elements (every flag below -1 taken as Dirichlet, values left out), bdc_device_ms = boundary_dofs with its download.  equal: the two transfers hold the
same integers and bits, the two lists the same dofs.  The levels are refined on the device and come down once, as in run_elements."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "element_transfer_probe.json")
MESHES = {"tet": ("cube_Tet.neu", 4), "mixed": ("cube_all_shapes_Six_boundary_groups.neu", 3)}
FE, FAM = "biquadratic", 2


class Builder:
    """what _prolongator_from_children reads of a Poisson001"""

    def __init__(self, ctx):
        self.ctx, self.fe = ctx, FE


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def host_bdc(level, flags):
    kind, ed, _, ff, _ = level
    fn_by = {s: [capi.fe_face_nodes(s, FE, f) for f in range(mixed_mesh.NFACES[s])] for s in sorted(set(kind.tolist()))}
    val = {}
    for iel, f in zip(*np.nonzero(ff < -1)):
        if int(ff[iel, f]) in flags:
            for node in ed[iel, fn_by[kind[iel]][f]]:
                val[int(node)] = 0.0
    return np.array(sorted(val), dtype=np.int32)


def csr(P):
    rp, col = P.pattern()
    return rp, col, P.values().view(np.uint64)


def main():
    global capi, mixed_mesh
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    import femus_amd
    from femus_amd import app_poisson, capi, mixed_mesh
    ctx = femus_amd.Context(0)
    out = {}
    for name, (fname, nref) in MESHES.items():
        mesh = mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", fname))
        flags = sorted({int(f) for f in np.unique(mesh[3]) if f < -1})
        dev = [capi.ElementMesh.from_arrays(ctx, *mesh)]
        for _ in range(nref):
            dev.append(dev[-1].refine())
        m = {"nel": [d.nel for d in dev[1:]], "ndof_fine": [d.own[FAM] for d in dev[1:]], "first_ms": [], "device_ms": [], "nnz": [], "bdc_device_ms": [], "bdc_dofs": []}
        if not a.device_only:
            m.update({"host_ms": [], "bdc_host_ms": [], "equal": [], "bdc_equal": []})
            levels = [d.arrays() for d in dev]
        for l in range(1, nref + 1):
            P = None
            for key in ("first_ms", "device_ms"):
                if P is not None:
                    P.destroy()
                ctx.sync()
                t0 = time.perf_counter()
                P = dev[l - 1].prolongator(dev[l], FE)
                ctx.sync()
                m[key].append(ms(t0))
            m["nnz"].append(P.nnz)
            dev[l].boundary_dofs(FE, flags)
            t0 = time.perf_counter()
            bd = dev[l].boundary_dofs(FE, flags)
            m["bdc_device_ms"].append(ms(t0))
            m["bdc_dofs"].append(int(bd.size))
            if not a.device_only:
                kind = levels[l - 1][0]
                groups = [(s, np.nonzero(kind == s)[0], mixed_mesh.CLASSES[s][FAM]) for s in sorted(set(kind.tolist()))]
                t0 = time.perf_counter()
                H = app_poisson.Poisson001._prolongator_from_children(Builder(ctx), groups, levels[l - 1][1], levels[l][1], levels[l - 1][4][FAM], levels[l][4][FAM])
                ctx.sync()
                m["host_ms"].append(ms(t0))
                m["equal"].append(bool(all(np.array_equal(x, y) for x, y in zip(csr(P), csr(H)))))
                H.destroy()
                t0 = time.perf_counter()
                hb = host_bdc(levels[l], set(flags))
                m["bdc_host_ms"].append(ms(t0))
                m["bdc_equal"].append(bool(np.array_equal(hb, bd)))
            P.destroy()
        if not a.device_only:
            m["host_over_device"] = [x / y for x, y in zip(m["host_ms"], m["device_ms"])]
            m["bdc_host_over_device"] = [x / y for x, y in zip(m["bdc_host_ms"], m["bdc_device_ms"])]
        for d in dev:
            d.destroy()
        out[name] = m
    ctx.close()
    if not a.device_only:
        with open(OUT, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
