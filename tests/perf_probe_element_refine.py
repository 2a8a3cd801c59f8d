"""Dev probe: uniform refinement of element meshes on the device (capi.ElementMesh.refine) against the numpy refiner (mixed_mesh.refine) in the same process --
cube_Tet.neu (105 TET15 elements) and the mixed cube (20 hexahedra, tetrahedra and prisms), four refinements each: the five-level case of
profiles/r06_simplex_five_levels.txt.

  python tests/perf_probe_element_refine.py                  one JSON line; also written to profiles/element_refine_probe.json
  rocprofv3 --kernel-trace --stats -d DIR -o er -- python tests/perf_probe_element_refine.py --device-only
                                                             the device chains alone, for the kernel share

Per level (the number of fine elements is the key): host_ms = mixed_mesh.refine; device_ms = ElementMesh.refine and the synchronisation after it;
device_get_ms = the same and the download of the fine level's arrays into mixed_mesh's layout (what app_poisson.run_elements pays per level).  The device
chain runs twice; the second run is reported (the first loads the code objects), the first is kept as `first_run`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "element_refine_probe.json")
MESHES = {"tet": "cube_Tet.neu", "mixed": "cube_all_shapes_Six_boundary_groups.neu"}
NREF = 4


def host_chain(mesh):
    t, levels = [], [mesh]
    for _ in range(NREF):
        t0 = time.perf_counter()
        levels.append(mixed_mesh.refine(*levels[-1][:4]))
        t.append((time.perf_counter() - t0) * 1e3)
    return t, levels


def device_chain(ctx, mesh):
    t_ref, t_get, nel = [], [], []
    t0 = time.perf_counter()
    dev = [capi.ElementMesh.from_arrays(ctx, *mesh)]
    upload = (time.perf_counter() - t0) * 1e3
    last = None
    for _ in range(NREF):
        t0 = time.perf_counter()
        dev.append(dev[-1].refine())
        ctx.sync()
        t1 = time.perf_counter()
        last = dev[-1].arrays()
        t2 = time.perf_counter()
        t_ref.append((t1 - t0) * 1e3)
        t_get.append((t2 - t0) * 1e3)
        nel.append(dev[-1].nel)
    for m in dev:
        m.destroy()
    return {"upload_ms": upload, "device_ms": t_ref, "device_get_ms": t_get, "nel": nel}, last


def main():
    global capi, mixed_mesh
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    import femus_amd
    from femus_amd import capi, mixed_mesh
    ctx = femus_amd.Context(0)
    out = {}
    for name, fname in MESHES.items():
        mesh = mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", fname))
        first, _ = device_chain(ctx, mesh)
        d, last = device_chain(ctx, mesh)
        m = {"nel": d["nel"], "nnode_finest": int(last[2].shape[0]), "upload_ms": d["upload_ms"], "device_ms": d["device_ms"], "device_get_ms": d["device_get_ms"],
             "first_run": {k: first[k] for k in ("device_ms", "device_get_ms")}}
        if not a.device_only:
            m["host_ms"], levels = host_chain(mesh)
            h = levels[-1]
            m["equal"] = bool(np.array_equal(h[1], last[1]) and np.array_equal(h[3], last[3]) and np.array_equal(h[2].view(np.int64), last[2].view(np.int64)))
            m["host_over_device"] = [x / y for x, y in zip(m["host_ms"], m["device_ms"])]
            m["host_over_device_get"] = [x / y for x, y in zip(m["host_ms"], m["device_get_ms"])]
        out[name] = m
    ctx.close()
    if not a.device_only:
        with open(OUT, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
