"""Dev probe: selective refinement of an element mesh on the device (capi.ElementMesh.flag + refine("resident") + prolongator) against the numpy statement of
the same rule (mixed_mesh.flag_elements / refine_flagged, app_poisson._prolongator_from_links) in the same process, and the uniform refine() of the same mesh
beside the figure of profiles/element_refine_probe.json (tet, 53 760 -> 430 080 elements), which the commit before this one wrote.

  python tests/perf_probe_element_refine_flagged.py                one JSON line; also written to profiles/element_refine_flagged_probe.json
  python tests/perf_probe_element_refine_flagged.py --device-only  without the numpy side (and without writing the file)

The mesh is that probe's: cube_Tet.neu refined three times on the device (53 760 TET15 elements, level 3).  The flag is the half-space x > 0.5.  Every
device figure is a host clock around calls that end in a synchronisation: REPEATS runs after WARMUP unmeasured ones; median, minimum and maximum in ms.
  device_ms       flag + flagged refinement + biquadratic prolongator, everything left resident
  device_get_ms   the same and the download of the fine level (arrays, levels and links) and of the transfer's CSR arrays
  uniform_ms      ElementMesh.refine() of the same mesh (the parent commit's figure: `parent_uniform_ms`, its two runs; `uniform_over_parent` = median / its
                  reported run)
  host_ms         the numpy rule, once (flag_elements is a Python loop over the elements and is reported on its own)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "element_refine_flagged_probe.json")
PARENT = os.path.join(ROOT, "profiles", "element_refine_probe.json")
MESH, NUNIFORM, EXPR, FE = "cube_Tet.neu", 3, "x > 0.5", "biquadratic"
WARMUP, REPEATS = 3, 11


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def timed(ctx, fn, cleanup):
    out = []
    for k in range(WARMUP + REPEATS):
        ctx.sync()
        t0 = time.perf_counter()
        made = fn()
        ctx.sync()
        t1 = time.perf_counter()
        cleanup(made)
        if k >= WARMUP:
            out.append((t1 - t0) * 1e3)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    import femus_amd
    from femus_amd import app_poisson, capi, mixed_mesh
    ctx = femus_amd.Context(0)
    dev = [capi.ElementMesh.from_arrays(ctx, *mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", MESH)))]
    for _ in range(NUNIFORM):
        dev.append(dev[-1].refine())
    c = dev[-1]
    expr = capi.Expr(EXPR, "x,y,z,level")

    def flagged():
        c.flag(expr)
        f = c.refine("resident")
        return f, c.prolongator(f, FE)

    def flagged_get():
        f, P = flagged()
        return f, P, f.arrays(), f.elem_levels(), P.pattern(), P.values()

    def drop(made):
        made[0].destroy()
        made[1].destroy()

    out = {"mesh": MESH, "nel": c.nel, "nnode": c.nnode, "level": c.level, "flag": EXPR, "fe": FE, "warmup": WARMUP, "repeats": REPEATS}
    out["uniform_ms"] = timed(ctx, c.refine, lambda f: f.destroy())
    out["device_ms"] = timed(ctx, flagged, drop)
    out["device_get_ms"] = timed(ctx, flagged_get, drop)
    out["uniform_again_ms"] = timed(ctx, c.refine, lambda f: f.destroy())                 # the drift of the machine over the run
    f, P, fine, links, (rp, col), val = flagged_get()
    flags = c.flag(expr)
    out.update(nel_fine=f.nel, nnode_fine=f.nnode, flagged=int(flags.sum()), nnz=int(col.size))
    drop((f, P))
    if os.path.exists(PARENT):
        tet = json.load(open(PARENT))["tet"]
        k = tet["nel"].index(8 * c.nel)
        out["parent_uniform_ms"] = [tet["device_ms"][k], tet["first_run"]["device_ms"][k]]
        out["uniform_over_parent"] = out["uniform_ms"]["median"] / tet["device_ms"][k]
    if not a.device_only:
        kind, ed, xs, ff, own = c.arrays()
        lev = np.full(c.nel, c.level)
        e = lambda x, l: x[0] > 0.5
        t0 = time.perf_counter()
        hflags = mixed_mesh.flag_elements(kind, ed, xs, lev, c.level, e)
        t1 = time.perf_counter()
        h = mixed_mesh.refine_flagged(kind, ed, xs, ff, hflags, lev, c.level)
        t2 = time.perf_counter()

        class Builder:
            fe, ctx = FE, None
        got = []
        keep = capi.Mat.__dict__["from_csr"]
        capi.Mat.from_csr = classmethod(lambda cls, cx, m, n, rowptr, cols, vals=None: got.append((np.array(rowptr), np.array(cols), np.array(vals))))
        try:
            groups = [(s, np.nonzero(kind == s)[0], mixed_mesh.CLASSES[s][2]) for s in sorted(set(kind.tolist()))]
            app_poisson.Poisson001._prolongator_from_links(Builder(), groups, ed, h[1], own[2], h[4][2], h[6], h[7])
        finally:
            capi.Mat.from_csr = keep
        t3 = time.perf_counter()
        out["host_ms"] = {"flag_elements": (t1 - t0) * 1e3, "refine_flagged": (t2 - t1) * 1e3, "prolongator": (t3 - t2) * 1e3}
        bits = lambda x: np.ascontiguousarray(x).view(np.int64)
        out["equal"] = bool(np.array_equal(hflags, flags) and np.array_equal(h[1], fine[1]) and np.array_equal(h[3], fine[3]) and list(h[4]) == list(fine[4])
                            and np.array_equal(bits(h[2]), bits(fine[2])) and all(np.array_equal(x, y) for x, y in zip(h[5:8], links))
                            and np.array_equal(got[0][0], rp) and np.array_equal(got[0][1], col) and np.array_equal(bits(got[0][2]), bits(val)))
        numpy_ms = out["host_ms"]["refine_flagged"] + out["host_ms"]["prolongator"]
        out["host_over_device"] = numpy_ms / out["device_ms"]["median"]                 # without the Python loop of flag_elements
        out["host_over_device_get"] = numpy_ms / out["device_get_ms"]["median"]
    expr.destroy()
    for m in dev:
        m.destroy()
    ctx.close()
    if not a.device_only:
        with open(OUT, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
