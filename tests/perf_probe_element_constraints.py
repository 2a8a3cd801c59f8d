"""Dev probe: the hanging-node constraints of a flagged level of an element mesh, searched on the device (capi.ElementMesh.amr_constraints) and, in the same run,
by the host search of the library on the downloaded arrays (fh_set_option "elem_constraints_host" = 1, at most 16 threads).

  python tests/perf_probe_element_constraints.py        one JSON line; also written to profiles/element_constraints_probe.json

The mesh is that of tests/perf_probe_element_refine_flagged.py: cube_Tet.neu refined three times on the device (53 760 TET15), the half-space x > 0.5 flagged and
refined (254 464 elements, levels 3 and 4).  Biquadratic family, both modes.  Every figure is REPEATS calls after WARMUP unmeasured ones, in ms: median, minimum, maximum.
  call_ms     the whole call between the context's timer_start / timer_stop (events on its stream around a call that ends synchronised)
  split_ms    the library's own wall clocks inside that call (fh_elem_mesh_amr_timings): "search" -- the kernels from the face count to the entries, with their scans
              and size read-backs (device), or the threaded search (host); "download" -- of the entries (device), of the whole mesh (host); "resolution" -- the
              serial walk that turns the entries into rows, the same code on both sides
`device_over_host` = median call of the device search / median call of the host search (below 1: the device search is the faster one)."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "element_constraints_probe.json")
MESH, NUNIFORM, EXPR, FE = "cube_Tet.neu", 3, "x > 0.5", "biquadratic"
WARMUP, REPEATS = 2, 7


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def timed(ctx, mesh, mode):
    call, split, c = [], {"search": [], "download": [], "resolution": []}, None
    for k in range(WARMUP + REPEATS):
        ctx.sync()
        ctx.timer_start()
        c = mesh.amr_constraints(FE, mode)
        ms = ctx.timer_stop()
        if k >= WARMUP:
            call.append(ms)
            for name, v in mesh.amr_timings().items():
                split[name].append(v)
    return {"call_ms": stats(call), "split_ms": {k: stats(v) for k, v in split.items()}}, c


def main():
    import femus_amd
    from femus_amd import capi, mixed_mesh
    ctx = femus_amd.Context(0)
    dev = [capi.ElementMesh.from_arrays(ctx, *mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", MESH)))]
    for _ in range(NUNIFORM):
        dev.append(dev[-1].refine())
    dev[-1].flag(EXPR)
    dev.append(dev[-1].refine("resident"))
    f = dev[-1]
    out = {"mesh": MESH, "nel_coarse": dev[-2].nel, "nel": f.nel, "nnode": f.nnode, "level": f.level, "flag": EXPR, "fe": FE, "warmup": WARMUP, "repeats": REPEATS,
           "host_threads": min(16, os.cpu_count() or 1)}
    for mode in ("reference", "coarsest"):
        d, cd = timed(ctx, f, mode)
        ctx.set_option("elem_constraints_host", 1)
        try:
            h, ch = timed(ctx, f, mode)
        finally:
            ctx.set_option("elem_constraints_host", 0)
        same = all(np.array_equal(cd[k], ch[k]) for k in range(3))
        out[mode] = {"device": d, "host": h, "hanging": int(cd[0].size), "entries": int(cd[2].size), "integers_equal": bool(same),
                     "max_weight_difference": float(np.abs(cd[3] - ch[3]).max()) if same and cd[3].size else None,
                     "device_over_host": d["call_ms"]["median"] / h["call_ms"]["median"]}
    for m in dev:
        m.destroy()
    ctx.close()
    line = json.dumps(out, sort_keys=True)
    print(line)
    with open(OUT, "w") as fo:
        json.dump(out, fo, indent=1, sort_keys=True)
        fo.write("\n")


if __name__ == "__main__":
    main()
