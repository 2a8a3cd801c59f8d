"""Dev probe: the error-norm flags of an element mesh on the device (capi.ElementMesh.flag_by_error, fh_elem_mesh_error_flag) against the host statement of the
same rule in the library (capi.error_flag_host, fh_elem_error_flag_host: the same element body, one thread) in the same process.

  python tests/perf_probe_element_error_flag.py                one JSON line; also written to profiles/element_error_flag_probe.json
  python tests/perf_probe_element_error_flag.py --device-only  without the host side (and without writing the file)

The mesh is that of tests/perf_probe_element_refine_flagged.py: cube_Tet.neu refined three times on the device (53 760 TET15 elements, level 3), then flagged
by the half-space x > 0.5 and refined once more, so that elements of two levels are present.  sol is a smooth function, eps a bump around the corner (1, 1, 1).
Every device figure is a host clock around calls that end in a synchronisation: REPEATS runs after WARMUP unmeasured ones; median, minimum and maximum in ms.
  device_ms       flag_by_error, flags downloaded (the call's own copy)
  indicators_ms   error_indicators (the element pass and two downloads of nel doubles)
  flag_refine_ms  flag_by_error + refine("resident")
  host_ms         error_flag_host on the downloaded arrays, once"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "element_error_flag_probe.json")
MESH, NUNIFORM, EXPR = "cube_Tet.neu", 3, "x > 0.5"
WARMUP, REPEATS = 3, 11
CASES = [("biquadratic", "H1"), ("linear", "L2")]


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def timed(ctx, fn, cleanup=lambda made: None):
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
    from femus_amd import capi, mixed_mesh
    ctx = femus_amd.Context(0)
    dev = [capi.ElementMesh.from_arrays(ctx, *mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", MESH)))]
    for _ in range(NUNIFORM):
        dev.append(dev[-1].refine())
    dev[-1].flag(EXPR)
    dev.append(dev[-1].refine("resident"))
    c = dev[-1]
    xs = c.coords()
    lev = c.elem_levels()[0]
    out = {"mesh": MESH, "nel": c.nel, "nnode": c.nnode, "level": c.level, "refinable": int((lev == c.level).sum()), "warmup": WARMUP, "repeats": REPEATS, "cases": {}}
    for fe, norm in CASES:
        n = c.own[capi.FE[fe]]
        x = xs[:n]
        sol = 1.0 + np.sin(3.0 * x[:, 0]) * np.cos(2.0 * x[:, 1]) + x[:, 2] ** 2
        q = ((x - 1.0) ** 2).sum(axis=1) / 0.36
        eps = 1e-2 * np.where(q < 1.0, (1.0 - q) ** 2, 0.0)
        S, E = ctx.vector_from(sol), ctx.vector_from(eps)
        r = c.flag_by_error(fe, S, E, 0.0, norm)
        err2, vol = c.error_indicators(fe, E, norm)                   # the threshold at which half of the elements the bump reaches are strong
        sel = err2 > 0
        thr = float("%.3g" % np.sqrt(np.median(err2[sel] / vol[sel]) * r["sums"][1] / r["sums"][0]))
        one = {"threshold": thr}
        one["device_ms"] = timed(ctx, lambda: c.flag_by_error(fe, S, E, thr, norm))
        one["indicators_ms"] = timed(ctx, lambda: c.error_indicators(fe, E, norm))
        one["flag_refine_ms"] = timed(ctx, lambda: (c.flag_by_error(fe, S, E, thr, norm), c.refine("resident"))[1], lambda f: f.destroy())
        d = c.flag_by_error(fe, S, E, thr, norm)
        one.update(nflagged=d["nflagged"], threshold_out=d["threshold"], sums=[float(v) for v in d["sums"]])
        if not a.device_only:
            kind, ed, xh, ff, own = c.arrays()
            t0 = time.perf_counter()
            h = capi.error_flag_host(kind, ed, xh, lev, c.level, fe, sol, eps, thr, norm)
            one["host_ms"] = (time.perf_counter() - t0) * 1e3
            bits = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.int64)
            one["equal"] = bool(np.array_equal(h["flags"], d["flags"]) and np.array_equal(bits(h["sums"]), bits(d["sums"])) and h["threshold"] == d["threshold"])
            one["host_over_device"] = one["host_ms"] / one["device_ms"]["median"]
        out["cases"]["%s-%s" % (fe, norm)] = one
        S.destroy()
        E.destroy()
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
