"""Dev probe: what stands between "the levels are resident" and "the first assembly" in app_poisson.Poisson001.run_elements, made from the downloaded arrays
(mesh_data "host") and from the device copy (mesh_data "device") in the same process -- the TET15 chain of cube_Tet.neu (105 elements) up to 430 080 elements
and the mixed cube (20 hexahedra, tetrahedra and prisms) up to 81 920, biquadratic.

  python tests/perf_probe_element_setup.py                     one JSON line; also written to profiles/element_setup_probe.json

Per mesh, milliseconds of wall clock with the stream synchronised before and after (device calls: the second of two, the first loads the code objects):
  download_ms             ElementMesh.arrays() of the top level (the host path downloads every level; all_levels_download_ms is their sum)
  pattern_{host,device}   _pattern_from_elements on the downloaded table / ElementMesh.matrix
  plan_{host,device}      capi.GenericAssembler on the arrays / GenericAssembler.from_mesh
  boundary_{host,device}  the face loop of run_elements over the top level (values left out) / boundary_owners + boundary_faces of every flag
  coords_ms               ElementMesh.coords(), the one download of the device path
  setup_{host,device}     the sum of what each path runs: host = every level's download + pattern + face loop + plan; device = pattern + plan + lists + coords
  info_{host,device}      GenericAssembler.info() of the two plans;  equal: patterns, plans (adj_ptr, adj, pos) and Dirichlet dofs hold the same integers"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "element_setup_probe.json")
MESHES = {"tet": ("cube_Tet.neu", 4), "mixed": ("cube_all_shapes_Six_boundary_groups.neu", 4)}
FE, FAM = "biquadratic", 2


class Builder:
    """what _pattern_from_elements reads of a Poisson001"""

    def __init__(self, ctx):
        self.ctx = ctx


def main():
    import femus_amd
    from femus_amd import app_poisson, capi, mixed_mesh
    ctx = femus_amd.Context(0)

    def timed(fn, repeat=1):
        for k in range(repeat):
            ctx.sync()
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            t = (time.perf_counter() - t0) * 1e3
            if k + 1 < repeat and hasattr(r, "destroy"):
                r.destroy()
        return r, t

    def face_loop(level, flags):
        kind, ed, xs, ff, _ = level
        fn_by = {s: [capi.fe_face_nodes(s, FE, f) for f in range(mixed_mesh.NFACES[s])] for s in sorted(set(kind.tolist()))}
        val, faces = {}, []
        for iel, f in zip(*np.nonzero(ff < -1)):
            nodes = ed[iel, fn_by[kind[iel]][f]]
            if int(ff[iel, f]) in flags:
                for node in nodes:
                    x4 = np.zeros(4)
                    x4[:xs.shape[1]] = xs[node]
                    val[int(node)] = 0.0
            else:
                faces.append(nodes)
        return np.array(sorted(val), dtype=np.int32), faces

    out = {}
    for name, (fname, nref) in MESHES.items():
        mesh = mixed_mesh.read_gambit(os.path.join(ROOT, "tests", "golden", fname))
        flags = sorted({int(f) for f in np.unique(mesh[3]) if f < -1})
        dirichlet, other = [f for f in flags if f != -4], [f for f in flags if f == -4]        # SetBoundaryCondition of the application: flux on face name 3
        dev = [capi.ElementMesh.from_arrays(ctx, *mesh)]
        for _ in range(nref):
            dev.append(dev[-1].refine())
        top = dev[-1]
        m = {"nel": top.nel, "ndof": top.own[FAM]}
        downloads = [timed(d.arrays) for d in dev]
        level = downloads[-1][0]
        m["download_ms"], m["all_levels_download_ms"] = downloads[-1][1], sum(t for _, t in downloads)
        kind, ed, xs = level[0], level[1], level[2]

        def host_pattern():
            eds = [ed[kind == s][:, :mixed_mesh.CLASSES[s][FAM]] for s in sorted(set(kind.tolist()))]
            return app_poisson.Poisson001._pattern_from_elements(Builder(ctx), eds, level[4][FAM])

        Kh, m["pattern_host_ms"] = timed(host_pattern)
        Kd, m["pattern_device_ms"] = timed(lambda: top.matrix(FAM), 2)
        shapes = sorted(set(kind.tolist()))
        geom, edh = (shapes[0], ed[:, :mixed_mesh.NLOC[shapes[0]]]) if len(shapes) == 1 else (kind, ed)
        gh, m["plan_host_ms"] = timed(lambda: capi.GenericAssembler(ctx, geom, FE, edh, xs, Kh))
        gd, m["plan_device_ms"] = timed(lambda: capi.GenericAssembler.from_mesh(top, FAM, Kd), 2)
        (hb, hfaces), m["boundary_host_ms"] = timed(lambda: face_loop(level, set(dirichlet)))
        lists = lambda: (top.boundary_owners(FAM, dirichlet), [top.boundary_faces(FAM, [f]) for f in other])
        (owners, dfaces), m["boundary_device_ms"] = timed(lists, 2)
        _, m["coords_ms"] = timed(top.coords, 2)
        m["setup_host_ms"] = m["all_levels_download_ms"] + m["pattern_host_ms"] + m["boundary_host_ms"] + m["plan_host_ms"]
        m["setup_device_ms"] = m["pattern_device_ms"] + m["plan_device_ms"] + m["boundary_device_ms"] + m["coords_ms"]
        m["setup_host_over_device"] = m["setup_host_ms"] / m["setup_device_ms"]
        m["info_host"], m["info_device"] = gh.info(), gd.info()
        m["boundary_dofs"], m["flux_faces"] = int(hb.size), len(hfaces)
        same = lambda a, b: bool(all(np.array_equal(x, y) for x, y in zip(a, b)))
        m["equal"] = {"pattern": same(Kh.pattern(), Kd.pattern()), "plan": same(gh.plan(), gd.plan()), "dirichlet_dofs": bool(np.array_equal(hb, owners[0])),
                      "flux_faces": sum(f[0].size for f in dfaces) == len(hfaces)}
        for x in (gh, gd, Kh, Kd) + tuple(dev):
            x.destroy()
        out[name] = m
    ctx.close()
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
