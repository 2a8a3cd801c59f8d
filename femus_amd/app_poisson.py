"""applications/001_Poisson/main.cpp over the C-ABI: reads the application's own JSON input, builds the
box mesh, the boundary conditions and the source from their strings, and runs LinearImplicitSystem::MGsolve on the GPU.

    load_config()    <- InputParser::build / JsonInputParser (src/00_file_handling/runtime_input_parsing/file/JsonInputParser.cpp;
                        the vendored jsoncpp reader accepts // comments, so they are stripped here)
    Poisson001       <- main.cpp:46-282: mesh (:118-141), FE order (:149), parsed boundary conditions (:158-180, names of the box
                        faces from MeshGeneration.cpp:544-559 / 1040-1070), source string (:200-211), multigrid options (:216-257)
    run()            <- LinearImplicitSystem::MGsolve (LinearImplicitSystem.cpp:288-411): up to max_number_linear_iteration
                        cycles {MGSolve with the outer GMRES limited to 4 iterations (SetTolerances(1e-12,1e-20,1e50,4)),
                        HasLinearConverged: ||RES||_2 < abs_conv_tol}, then UpdateSol

Sign convention of the application (main.cpp:472-474): F = (src phi - grad phi . grad T) w, i.e. -Laplace T = src, which is the
library kernel with f = -src.  Mesh files ("filename" inputs, Gambit .neu) are read by fh_mesh_read_gambit
and take the boundary conditions of the application's SetBoundaryCondition function (main.cpp:26-36).
All numerics run in libfemus_hip.so; expressions are compiled by fh_expr_compile and evaluated on the device (source) or on the
host at boundary nodes (Dirichlet values).
"""
import json
import os
import re

import numpy as np

from . import capi
from .poisson import PoissonMG

FACE_NAMES = {1: ["left", "right"], 2: ["bottom", "right", "top", "left"], 3: ["bottom", "front", "right", "behind", "left", "top"]}   # MeshGeneration.cpp:248-253 (EDGE3 box)
FE_ORDER = {"first": "linear", "serendipity": "serendipity", "second": "biquadratic"}       # FEOrder of the input (main.cpp:149) -> Lagrange family
PREFIX = "multilevel_problem.multilevel_mesh.first.system.poisson.linear_solver."


def load_config(path_or_text):
    text = open(path_or_text).read() if "\n" not in path_or_text and "{" not in path_or_text else path_or_text
    out, i, in_str = [], 0, False
    while i < len(text):                        # outside strings: drop // comments, make "1." / "1.e-9" / ".5" strict JSON numbers
        c = text[i]
        if c == '"' and (i == 0 or text[i - 1] != "\\"):
            in_str = not in_str
        if not in_str and text.startswith("//", i):
            while i < len(text) and text[i] != "\n":
                i += 1
            continue
        if not in_str and c == "." and (i + 1 >= len(text) or not text[i + 1].isdigit()):
            out.append(".0")                    # jsoncpp reads "1." and "1.e-09"
            i += 1
            continue
        if not in_str and c == "." and (not out or not out[-1][-1].isdigit()):
            out.append("0.")                    # ".5"
            i += 1
            continue
        out.append(c)
        i += 1
    clean = re.sub(r",(\s*[}\]])", r"\1", "".join(out))
    return json.loads(clean)


def get(cfg, dotted, default):
    """InputParser::getValue: value at a dotted path, or the default"""
    node = cfg
    for key in dotted.split("."):
        if not isinstance(node, dict) or key not in node:
            return default
        node = node[key]
    return node


class Poisson001:
    def __init__(self, ctx, config, base_dir=None):
        """config: path of the JSON file, its text, or the parsed dict; base_dir: directory mesh file names are relative to
        (the application is run from its own directory)"""
        self.ctx = ctx
        cfg = config if isinstance(config, dict) else load_config(config)
        self.cfg = cfg
        mesh_type = get(cfg, "multilevel_mesh.first.type", {})
        self.mesh_file, self.geom = None, None            # geom: the element path of a mesh femus_amd/mixed_mesh.py builds; None: the library's mesh code
        if "filename" in mesh_type:
            self.mesh_file = os.path.join(base_dir, mesh_type["filename"]) if base_dir else mesh_type["filename"]
            self.geom = self._gambit_kind(self.mesh_file)
            if self.geom is not None:
                with open(self.mesh_file) as f:
                    tok = f.read().split()
                self.dim = int(tok[tok.index("NDFVL") + 5])
            else:
                probe = capi.Mesh.read_gambit(self.mesh_file)
                self.dim = probe.dim
                probe.destroy()
            self.box = None
        elif "box" in mesh_type:
            b = mesh_type["box"]
            self.box = (int(b.get("nx", 2)), int(b.get("ny", 2)), int(b.get("nz", 0)))
            self.lo = (float(b.get("xa", 0.)), float(b.get("ya", 0.)), float(b.get("za", 0.)))
            self.hi = (float(b.get("xb", 1.)), float(b.get("yb", 1.)), float(b.get("zb", 0.)))
            self.dim = 1 if (self.box[1] == 0 and self.box[2] == 0) else 2 if self.box[2] == 0 else 3
            if self.dim == 2:
                self.hi = (self.hi[0], self.hi[1], 1.0)         # the box generator ignores z in 2-D
            if self.dim == 2 and b.get("elem_type", "Quad9") == "Tri6":                   # MeshGeneration.cpp:568-: the box cut into triangles
                self.geom = "tri"
            if self.dim == 1:
                assert b.get("elem_type", "Edge3") == "Edge3", "the one-dimensional box is made of EDGE3 elements (MeshGeneration.cpp:90)"
        else:
            raise ValueError("Error: no input mesh specified. Please check to have added the keyword mesh in the input json file! ")
        var = "multilevel_solution.multilevel_mesh.first.variable.first."
        self.fe = FE_ORDER[get(cfg, var + "fe_order", "first")]
        self.nlevels = int(get(cfg, PREFIX + "type.multigrid.nlevels", 1))
        self.npre = int(get(cfg, PREFIX + "type.multigrid.npresmoothing", 1))
        self.npost = int(get(cfg, PREFIX + "type.multigrid.npostmoothing", 1))        # the key the application reads (sic)
        self.max_linear = int(get(cfg, PREFIX + "max_number_linear_iteration", 6))
        self.abs_tol = float(get(cfg, PREFIX + "abs_conv_tol", 1.e-08))
        assert get(cfg, PREFIX + "type.multigrid.mgtype", "V_cycle") == "V_cycle", "only the V-cycle of the shipped inputs is served"
        # boundary conditions per face flag (flag = -(face name) - 1)
        self.bc_type, self.bc_func = {}, {}
        if self.box is not None:
            # default Dirichlet homogeneous on every face (InitializeBdc_with_ParsedFunction), then the listed faces
            names = FACE_NAMES[self.dim]
            for n in names:
                self.bc_type[self.flag_of(n)], self.bc_func[self.flag_of(n)] = "dirichlet", None
            for item in get(cfg, var + "boundary_conditions", []):
                name = item.get("facename", "top")
                if name not in names:
                    raise ValueError(" Error: the facename %s does not exist!" % name)
                self.bc_type[self.flag_of(name)] = item.get("bdc_type", "dirichlet")
                self.bc_func[self.flag_of(name)] = capi.Expr(item.get("bdc_func", "0."), "x,y,z,t")
        else:
            # SetBoundaryCondition of the application (main.cpp:26-36): Dirichlet 0 everywhere, flux 0.2 on face name 3
            self.file_flux = {-4: 0.2}
        self.source = capi.Expr(get(cfg, var + "func_source", "0."), "x,y,z,t")

    def flag_of(self, name):
        return -(FACE_NAMES[self.dim].index(name) + 2)

    def face_bc(self, flag):
        """(type, function or None) of a boundary face"""
        if self.box is None:
            return ("neumann", None) if flag in self.file_flux else ("dirichlet", None)
        return self.bc_type[flag], self.bc_func[flag]

    def dirichlet_data(self, mesh):
        """GenerateBdc with parsed functions (MultiLevelSolution.cpp:762-800): elements and faces in order; nodes of Dirichlet
        faces get Bdc = 0 and Sol = value(x, y, z, t = 0); a later face overwrites an earlier one"""
        ed, xy, ff = mesh.arrays()
        nc = {"linear": 2 ** self.dim, "serendipity": {1: 3, 2: 8, 3: 20}[self.dim], "biquadratic": 3 ** self.dim}[self.fe]
        val = {}
        for iel, f in zip(*np.nonzero(ff < -1)):
            kind, fn = self.face_bc(int(ff[iel, f]))
            if kind != "dirichlet":
                continue
            for i in capi.fe_face_nodes(mesh.geom, "biquadratic", f):
                if i >= nc:
                    continue
                node = int(ed[iel, i])
                x4 = np.zeros(4)
                x4[:self.dim] = xy[node]
                val[node] = fn(x4) if fn is not None else 0.0
        idx = np.array(sorted(val), dtype=np.int32)
        return idx, np.array([val[i] for i in idx])

    def run(self, smoother=capi.SMOOTH_GS_COLOR, omega=0.5, log=None, output_dir=None, simplex_smoother=capi.SMOOTH_GS_COLOR, simplex_omega=1.0):
        """smoother / omega: the application sets RICHARDSON + SOR_PRECOND on the fine grids (main.cpp:240-242) and leaves the
        Richardson scale at the solver default 0.5 (LinearEquationSolverPetsc.hpp:145).  output_dir: write what the application writes at
        its end (main.cpp:259-270): the VTK and the GMV file of "Sol", named as the reference names them"""
        ctx = self.ctx
        if self.dim == 1:
            return self.run_line(log)
        # triangles, tetrahedra, prisms, mixed shapes: multicolour Gauss-Seidel by default -- the iteration counts of the natural-order symmetric sweep the
        # application sets (SOR_PRECOND; simplex_smoother=capi.SMOOTH_SOR runs that one) at half the time on 240 k unknowns (tests/dev/probe_simplex_smoother.py)
        if self.geom is not None:
            return self.run_elements(log, simplex_smoother, simplex_omega)
        meshes = [capi.Mesh.box(*self.box, self.lo, self.hi) if self.box is not None else capi.Mesh.read_gambit(self.mesh_file)]
        for _ in range(1, self.nlevels):
            meshes.append(meshes[-1].refine())
        data = [self.dirichlet_data(m) for m in meshes]
        pb = PoissonMG(ctx, 0, 0, 0, self.nlevels, fe=self.fe, omega=omega, npre=self.npre, npost=self.npost, meshes=meshes,
                       smoother=smoother, dirichlet=[d[0] for d in data], source_expr=self.source, source_scale=-1.0)
        pb.init()
        top = self.nlevels - 1
        sol0 = np.zeros(pb.ndof[top])
        sol0[data[top][0]] = data[top][1]
        pb.SOL.upload(sol0)
        pb.assemble()
        # non-homogeneous Neumann faces: the parsed function of the face evaluated at every face Gauss point (box input, main.cpp:495-553);
        # the constant flux of SetBoundaryCondition (mesh-file input, main.cpp:556-594)
        flux = dict(self.file_flux) if self.box is None else {}
        for flag, kind in self.bc_type.items():
            if kind == "neumann" and self.bc_func[flag] is not None:
                flux[flag] = self.bc_func[flag]
        if flux:
            capi.assemble_neumann(ctx, meshes[top], self.fe, pb.RES, flux)
        pb.prepare()
        history = []
        for it in range(self.max_linear):
            its, _ = pb.mgsolve(outer="gmres", rtol=1e-12, atol=1e-20, maxit=4)
            rn = pb.RES.l2_norm()
            history.append((its, rn))
            if log:
                log("linear iteration %d: %d Krylov steps, Linear Res L2norm = %.6e" % (it + 1, its, rn))
            if rn < self.abs_tol:
                break
        pb.update_sol()
        _, xy, _ = meshes[top].arrays()
        result = {"solution": pb.SOL.to_numpy(), "coords": xy[:pb.ndof[top]], "history": history, "converged": history[-1][1] < self.abs_tol,
                  "dofs": pb.ndof[top]}
        if output_dir is not None:
            import os
            from . import writers
            # VTKWriter / GMVWriter file names: <prefix>.level<gridn>.<time step>.<order>.<ext> with gridn = number of levels
            stem = os.path.join(str(output_dir), "sol.level%d.%d.%s" % (self.nlevels, 0, "biquadratic"))
            field = result["solution"]
            if field.size != meshes[top].nnode:          # linear / serendipity solution: the writers carry the vertex values to the nodes of the output family
                field = field[:meshes[top].own_size[0]]
            writers.write_vtu(stem + ".vtu", meshes[top], {"Sol": field})
            writers.write_gmv(stem + ".gmv", meshes[top], {"Sol": field}, "biquadratic")
            result["files"] = [stem + ".vtu", stem + ".gmv"]
        pb.destroy()
        return result

    # the element path as flags: the TRI6 box, a file of TET10 alone, of WEDGE18 alone, any other file mixed_mesh.py reads
    tri, tet, wedge, mixed = (property(lambda self, g=g: self.geom == g) for g in ("tri", "tet", "wedge", "mixed"))

    @staticmethod
    def _gambit_kind(path):
        """the element path of a Gambit file: None for HEX27 alone or QUAD9 alone (the library's reader); otherwise femus_amd/mixed_mesh.py reads it, and
        "tet" / "wedge" (TET10 / WEDGE18 alone: that shape's kernel) or "mixed" (every other file: several shapes, the two-dimensional files with triangles; an
        element the reader does not serve is named there and refused)"""
        from . import mixed_mesh
        with open(path) as f:
            tok = f.read().split()
        if "ELEMENTS/CELLS" not in tok or "NDFVL" not in tok:
            return None
        nel = int(tok[tok.index("NDFVL") + 2])
        p = tok.index("ELEMENTS/CELLS") + 2
        seen = set()
        for _ in range(nel):
            seen.add(mixed_mesh.GAMBIT.get((int(tok[p + 1]), int(tok[p + 2]))))
            p += 3 + int(tok[p + 2])
        if seen in ({"hex"}, {"quad"}):
            return None
        return seen.pop() if seen in ({"tet"}, {"wedge"}) else "mixed"

    def run_elements(self, log=None, smoother=capi.SMOOTH_GS_COLOR, omega=1.0, transfers="device", selective_levels=0, flag=None, amr_mode="reference",
                     mesh_data="host"):
        """LinearImplicitSystem::MGsolve on the meshes femus_amd/mixed_mesh.py builds, in all three Lagrange families: the TRI6 box (TRI7 inside; the box's
        boundary conditions and source), Gambit files of TET10 (input3D_Tet_*.json with input/cube_Tet.neu; TET15 inside), of WEDGE18 (input3D_Wedge_*.json with
        input/cube_Wedge.neu; WEDGE21 inside), of mixed shapes (input3D.json / input3D_All_first.json with input/cube_all_shapes_Six_boundary_groups.neu:
        tetrahedra, prisms and hexahedra) and the two-dimensional files of QUAD9 and / or TRI6 (the boundary conditions of the application's SetBoundaryCondition:
        Dirichlet 0, flux 0.2 on face name 3).  The Poisson callback through the generic kernel on the finest level (fh_assemble_poisson_rows for the box and
        the tetrahedral / prism files, fh_assemble_poisson_mixed on the mixed path, elem_dof rows padded with -1), transfers from the element prolongators,
        Galerkin operators below.  transfers: "device" builds every level's PP and Dirichlet list from the resident meshes (capi.ElementMesh.prolongator /
        boundary_dofs), "host" with _prolongator_from_children and the face loop below -- the same bits.
        selective_levels > 0: the last so many of the nlevels come from a flagged refinement on the device (MultiLevelMesh::RefineMesh with a flag function:
        resident.flag(flag), an expression over x, y, z, level, then refine("resident")); the levels before them are uniform as ever.  A non-homogeneous level l gets
        its hanging dofs and P_amr[l] from the resident mesh (capi.ElementMesh.amr_constraints / amr_prolongator, amr_mode "reference" or "coarsest") and is wired
        as LinearImplicitSystem does it (poisson.py for the box meshes): bdc[l] = Dirichlet + hanging, PP[l + 1] <- PP[l + 1] P_amr[l], and on the top level
        RES <- P_amr^T RES, the operator P_amr^T KK P_amr, EPS <- P_amr EPS (_mgsolve).  The start vector is made conforming, SOL <- P_amr SOL, so that a hanging
        dof with a master on the Dirichlet boundary starts from its masters' values.  Only with transfers "device".
        result["levels"]: (ed, xs, ff) of every level; ed and ff as wide as the shape, or padded to 27 and 6 on the mixed path; result["hanging"]: the top
        level's hanging dofs; result["elem_levels"]: the level of every element of the top level.
        mesh_data: "host" downloads every level (capi.ElementMesh.arrays) and makes the pattern, the plan of the element loop and the boundary data from the
        arrays.  "device" (only with transfers "device") makes them where the levels live -- capi.ElementMesh.matrix, capi.GenericAssembler.from_mesh,
        boundary_owners and boundary_faces of the top level -- and brings down the top level's coordinates alone, for result["coords"] and the Neumann calls;
        no level is downloaded, so result["levels"] is ABSENT in this mode.  Everything else in the result is the same, bit for bit."""
        from . import mixed_mesh
        ctx = self.ctx
        levels = [mixed_mesh.tri_box(self.box[0], self.box[1], self.lo[:2], self.hi[:2]) if self.box is not None else mixed_mesh.read_gambit(self.mesh_file)]
        if transfers not in ("device", "host"):
            raise ValueError("transfers must be \"device\" or \"host\", not %r" % (transfers,))
        if mesh_data not in ("device", "host"):
            raise ValueError("mesh_data must be \"device\" or \"host\", not %r" % (mesh_data,))
        if mesh_data == "device" and transfers != "device":
            raise ValueError("mesh_data \"device\" keeps the levels on the device: transfers must be \"device\", not %r" % (transfers,))
        resident_data = mesh_data == "device"
        fam = {"linear": 0, "serendipity": 1, "biquadratic": 2}[self.fe]
        selective_levels = int(selective_levels)
        if selective_levels:
            if transfers != "device":
                raise ValueError("flagged levels (selective_levels = %d) are built on the device: transfers must be \"device\", not %r" % (selective_levels, transfers))
            if not 0 < selective_levels < self.nlevels or flag is None:
                raise ValueError("selective_levels must be 0 .. nlevels - 1 = %d and come with a flag expression over x, y, z, level" % (self.nlevels - 1))
            if amr_mode not in ("reference", "coarsest"):
                raise ValueError("amr_mode must be \"reference\" or \"coarsest\", not %r" % (amr_mode,))
        n_uniform = self.nlevels - selective_levels
        P_amr = [None] * self.nlevels
        hanging = [np.zeros(0, np.int32)] * self.nlevels
        elem_levels = None
        # level 0 goes up once and is refined on the device (capi.ElementMesh: the arrays of mixed_mesh.refine, integer for integer and bit for bit); the
        # transfers and the Dirichlet lists are built from the resident meshes; every level comes down once for result["levels"], the flux faces and the top
        # level's boundary values -- or, with mesh_data "device", none does: pattern, plan and boundary data are made from the resident top level
        resident = [capi.ElementMesh.from_arrays(ctx, *levels[0])]
        P_dev, bdc_dev = [None], []
        K = gen = top_data = None
        try:
            for l in range(1, self.nlevels):
                if l < n_uniform:
                    resident.append(resident[-1].refine())
                else:
                    resident[-1].flag(flag)
                    resident.append(resident[-1].refine("resident"))
                if not resident_data:
                    levels.append(resident[-1].arrays())
            for l, m in enumerate(resident):
                if not m.homogeneous:
                    hanging[l] = m.amr_constraints(fam, amr_mode)[0]
                    P_amr[l] = m.amr_prolongator(fam, amr_mode)
            if selective_levels:
                elem_levels = resident[-1].elem_levels()[0]
            if transfers == "device":
                # the flags a mesh carries are those of level 0: a child face inherits its father's
                dirichlet = sorted({int(f) for f in np.unique(levels[0][3]) if f < -1 and self.face_bc(int(f))[0] == "dirichlet"})
                for l, m in enumerate(resident):
                    bdc_dev.append(m.boundary_dofs(fam, dirichlet))
                    if l:
                        P_dev.append(resident[l - 1].prolongator(m, fam))
            if resident_data:
                # pattern, plan and boundary data of the top level from its device copy; the faces of every flag that is not Dirichlet, each flag's list in
                # (element, face) order, for the flux terms
                m = resident[-1]
                K = m.matrix(fam)
                gen = capi.GenericAssembler.from_mesh(m, fam, K)
                other = sorted({int(f) for f in np.unique(levels[0][3]) if f < -1} - set(dirichlet))
                top_data = (m.boundary_owners(fam, dirichlet), {f: m.boundary_faces(fam, [f]) for f in other}, m.coords(), list(m.own), m.dim)
        except BaseException:
            for p in P_dev[1:] + [q for q in P_amr if q is not None] + [q for q in (gen, K) if q is not None]:
                p.destroy()
            raise
        finally:
            for m in resident:
                m.destroy()
        if resident_data:
            return self._run_resident(K, gen, top_data, P_dev, bdc_dev, P_amr, hanging, elem_levels, selective_levels, log, smoother, omega)
        if not self.mixed:
            g = self.geom
            levels = [(kind, ed[:, :mixed_mesh.NLOC[g]], xs, ff[:, :mixed_mesh.NFACES[g]], own) for kind, ed, xs, ff, own in levels]
        shapes = sorted(set(levels[0][0].tolist()))
        dim = levels[0][2].shape[1]
        fn_by = {s: [capi.fe_face_nodes(s, self.fe, f) for f in range(mixed_mesh.NFACES[s])] for s in shapes}
        groups = [[(s, np.nonzero(lv[0] == s)[0], mixed_mesh.CLASSES[s][fam]) for s in shapes] for lv in levels]     # (shape, its elements, dofs per element)
        ndofs = [lv[4][fam] for lv in levels]
        top = self.nlevels - 1
        kind, ed, xs, ff, _ = levels[top]
        ndof = ndofs[top]
        K = self._pattern_from_elements([ed[idx][:, :nc] for _, idx, nc in groups[top]], ndof)
        sol0 = np.zeros(ndof)
        bdc = []
        flux_faces, flux_idx, flux_exprs, tau_faces, tau_vals = [], [], [], [], []
        for l, (kl, edl, xl, ffl, _) in enumerate(levels):
            if transfers == "device" and l != top:                  # the list is there; values and flux faces belong to the top level alone
                bdc.append(bdc_dev[l])
                continue
            val = {}
            for iel, f in zip(*np.nonzero(ffl < -1)):               # elements and faces in order; a later face overwrites an earlier one (GenerateBdc)
                flag = int(ffl[iel, f])
                kind_bc, fn = self.face_bc(flag)
                nodes = edl[iel, fn_by[kl[iel]][f]]
                if kind_bc == "dirichlet":
                    for node in nodes:
                        x4 = np.zeros(4)
                        x4[:dim] = xl[node]
                        val[int(node)] = fn(x4) if (fn is not None and l == top) else 0.0
                elif l == top:
                    if fn is not None:                              # parsed flux (box inputs)
                        if fn not in flux_exprs:
                            flux_exprs.append(fn)
                        flux_faces.append(nodes)
                        flux_idx.append(flux_exprs.index(fn))
                    elif self.box is None and flag in self.file_flux:      # the constant flux of SetBoundaryCondition (mesh-file inputs)
                        tau_faces.append(nodes)
                        tau_vals.append(self.file_flux[flag])
            idx = np.array(sorted(val), dtype=np.int32)
            bdc.append(bdc_dev[l] if transfers == "device" else idx)
            if l == top:
                sol0[idx] = [val[i] for i in idx]
        P = P_dev if transfers == "device" else [None] + [self._prolongator_from_children(groups[l - 1], levels[l - 1][1], levels[l][1], ndofs[l - 1], ndofs[l])
                                                          for l in range(1, self.nlevels)]
        # the plan of the element loop, made once: every linear iteration assembles on the same mesh and pattern
        out = self._solve_elements(K, lambda: capi.GenericAssembler(ctx, kind if self.mixed else self.geom, self.fe, ed, xs, K), xs, ndof, dim, sol0, bdc, P, P_amr,
                                   hanging, elem_levels, selective_levels, (flux_faces, flux_idx, flux_exprs, tau_faces, tau_vals), log, smoother, omega)
        out["levels"] = [lv[1:4] for lv in levels]
        return out

    def run_elements_adaptive(self, max_amr_levels, threshold, norm="H1", neighbor_threshold=0.0, amr_mode="reference", log=None, smoother=capi.SMOOTH_GS_COLOR,
                              omega=1.0, keep_steps=False, exact=None, exact_gradient=None):
        """MGsolve with _AMRtest (LinearImplicitSystem.cpp:309-404, 529-558; SetAMRSetOptions(AMR, AMRlevels = max_amr_levels, AMRnorm = norm, AMRthreshold =
        threshold)): the nlevels uniform levels are built on the device and solved on the top one as run_elements(mesh_data="device") does; then, until the flags
        say converged or max_amr_levels levels have been added: AMREps = what the solve added to the top level's solution (the final solution minus the start
        vector, EPS <- P_amr EPS included); capi.ElementMesh.flag_by_error with the current threshold; refine("resident"); constraints, P_amr, transfer
        (PP <- PP P_amr of the level below where that one is non-homogeneous), pattern, plan and boundary data of the new level from the resident meshes; the
        solution prolonged with the transfer before its Dirichlet rows are zeroed, the boundary values imposed as run_elements does for its start vector; the
        solve on the new top level, with the adjusted threshold for the next step.  The set-up of the lower levels is rebuilt at every step.  The resident levels
        live until the method returns; none is downloaded but the final coordinates (keep_steps=True also brings down, for every step, "sol", "eps" and the
        level's (kind, ed, xs, ff, lev, level): result["steps"], for tests).
        The result is run_elements(mesh_data="device")'s of the last solve, with "amr_history" (per step: nflagged, nel, threshold_in, threshold_out, sums,
        converged), "elem_levels" and "hanging" of the final level and "nlevels".
        With exact -- an expression over "x,y,z,t" (text or capi.Expr) -- every "amr_history" entry also carries "l2_error" and "h1_error" of that step's
        solution (capi.ElementMesh.error_norms on the resident top level while the solution is uploaded for the flags): against the exact values at the Gauss
        points when exact_gradient (dim expressions) is given, else against the exact function's nodal interpolant.  max_amr_levels = 0 at consecutive nlevels
        gives the uniform convergence table of ex02."""
        from . import mixed_mesh
        ctx = self.ctx
        max_amr_levels = int(max_amr_levels)
        if max_amr_levels < 0:
            raise ValueError("max_amr_levels must not be negative, not %d" % max_amr_levels)
        if amr_mode not in ("reference", "coarsest"):
            raise ValueError("amr_mode must be \"reference\" or \"coarsest\", not %r" % (amr_mode,))
        norm_code = capi.amr_norm("run_elements_adaptive", norm)
        if exact is None and exact_gradient is not None:
            raise ValueError("exact_gradient without exact")
        fam = {"linear": 0, "serendipity": 1, "biquadratic": 2}[self.fe]
        level0 = mixed_mesh.tri_box(self.box[0], self.box[1], self.lo[:2], self.hi[:2]) if self.box is not None else mixed_mesh.read_gambit(self.mesh_file)
        all_flags = sorted({int(f) for f in np.unique(level0[3]) if f < -1})
        dirichlet = [f for f in all_flags if self.face_bc(f)[0] == "dirichlet"]
        other = sorted(set(all_flags) - set(dirichlet))
        resident = [capi.ElementMesh.from_arrays(ctx, *level0)]
        nlevels0, thr = self.nlevels, float(threshold)
        amr_history, steps, prev, out = [], [], None, None
        try:
            for _ in range(1, nlevels0):
                resident.append(resident[-1].refine())
            while True:
                nl, m = len(resident), resident[-1]
                top = nl - 1
                owned = []              # what this step made and has not handed to the solve yet
                try:
                    hanging, P_amr = [np.zeros(0, np.int32)] * nl, [None] * nl
                    for l, lv in enumerate(resident):
                        if not lv.homogeneous:
                            hanging[l] = lv.amr_constraints(fam, amr_mode)[0]
                            P_amr[l] = lv.amr_prolongator(fam, amr_mode)
                            owned.append(P_amr[l])
                    bdc, P = [], [None]
                    for l, lv in enumerate(resident):
                        bdc.append(lv.boundary_dofs(fam, dirichlet))
                        if l:
                            P.append(resident[l - 1].prolongator(lv, fam))
                            owned.append(P[-1])
                    start = None
                    if prev is not None:                              # the solution of the level below, through PP P_amr before any row is zeroed
                        v, w, s = ctx.vector_from(prev), ctx.vector(prev.size), ctx.vector(m.own[fam])
                        try:
                            if P_amr[top - 1] is not None:
                                w.matrix_mult(v, P_amr[top - 1])
                                v.assign(w)
                            s.matrix_mult(v, P[top])
                            start = s.to_numpy()
                        finally:
                            for q in (v, w, s):
                                q.destroy()
                    K = m.matrix(fam)
                    owned.append(K)
                    gen = capi.GenericAssembler.from_mesh(m, fam, K)
                    owned.append(gen)
                    top_data = (m.boundary_owners(fam, dirichlet), {f: m.boundary_faces(fam, [f]) for f in other}, m.coords(), list(m.own), m.dim)
                    elem_levels = m.elem_levels()[0]
                except BaseException:
                    for q in owned:
                        q.destroy()
                    raise
                keep = {}
                self.nlevels = nl                                     # the helpers below count the levels of the hierarchy they are given by this
                try:
                    out = self._run_resident(K, gen, top_data, P, bdc, P_amr, hanging, elem_levels, nl - nlevels0, log, smoother, omega, start=start, keep=keep)
                finally:
                    self.nlevels = nlevels0
                sol = out["solution"]
                eps = sol - keep["start"]
                SOLv, EPSv = ctx.vector_from(sol), ctx.vector_from(eps)
                try:
                    r = m.flag_by_error(fam, SOLv, EPSv, thr, norm_code, neighbor_threshold)
                    en = m.error_norms(fam, SOLv, exact=exact, gradient=exact_gradient) if exact is not None else None
                finally:
                    SOLv.destroy()
                    EPSv.destroy()
                amr_history.append({"nflagged": r["nflagged"], "nel": m.nel, "threshold_in": thr, "threshold_out": r["threshold"], "sums": r["sums"],
                                    "converged": r["converged"]})
                if en is not None:
                    amr_history[-1]["l2_error"], amr_history[-1]["h1_error"] = en["l2"], en["h1"]
                if log:
                    log("AMR step %d: %d of %d elements flagged, threshold %.6e -> %.6e%s" % (len(amr_history) - 1, r["nflagged"], m.nel, thr, r["threshold"],
                                                                                           ", converged" if r["converged"] else ""))
                if keep_steps:
                    kind, ed, xs, ff, _ = m.arrays()
                    steps.append({"sol": sol, "eps": eps, "flags": r["flags"], "mesh": (kind, ed, xs, ff, elem_levels, m.level)})
                if r["converged"] or nl - nlevels0 >= max_amr_levels:
                    break
                resident.append(m.refine("resident"))
                thr, prev = r["threshold"], sol
            out["amr_history"], out["nlevels"] = amr_history, len(resident)
            out["elem_levels"], out["hanging"] = elem_levels, hanging[-1]
            if keep_steps:
                out["steps"] = steps
            return out
        finally:
            for lv in resident:
                lv.destroy()

    def _run_resident(self, K, gen, top_data, P, bdc, P_amr, hanging, elem_levels, selective_levels, log, smoother, omega, start=None, keep=None):
        """the rest of run_elements with mesh_data "device": K and gen were made from the resident top level; top_data = (boundary_owners of the Dirichlet flags,
        {flag: boundary_faces} of the others, the top level's coordinates, own, dim).  The face loop of the host path, stated on the lists: a Dirichlet dof takes
        the function of the last face that holds it; the flux faces go in (element, face) order"""
        (b_dofs, b_flag, b_xy), faces, xs, own, dim = top_data
        fam = {"linear": 0, "serendipity": 1, "biquadratic": 2}[self.fe]
        ndof = own[fam]
        sol0 = np.zeros(ndof)
        if start is not None:                                     # run_elements_adaptive: a prolonged solution; every Dirichlet dof takes its boundary value
            sol0[:] = start
            sol0[b_dofs] = 0.0
        for f in np.unique(b_flag):
            fn = self.face_bc(int(f))[1]
            if fn is not None:
                sel = b_flag == f
                x4 = np.zeros((int(sel.sum()), 4))
                x4[:, :dim] = b_xy[sel]
                sol0[b_dofs[sel]] = fn(x4)
        flags = sorted(faces)
        where = np.concatenate([6 * faces[f][0].astype(np.int64) + faces[f][1] for f in flags] + [np.zeros(0, np.int64)])
        rows = [(f, faces[f][2][k, :faces[f][3][k]]) for f in flags for k in range(faces[f][0].size)]
        flux_faces, flux_idx, flux_exprs, tau_faces, tau_vals = [], [], [], [], []
        for k in np.argsort(where, kind="stable"):                # the flux faces alone, in the order of the face loop
            f, nodes = rows[k]
            fn = self.face_bc(f)[1]
            if fn is not None:                                    # parsed flux (box inputs)
                if fn not in flux_exprs:
                    flux_exprs.append(fn)
                flux_faces.append(nodes)
                flux_idx.append(flux_exprs.index(fn))
            elif self.box is None and f in self.file_flux:        # the constant flux of SetBoundaryCondition (mesh-file inputs)
                tau_faces.append(nodes)
                tau_vals.append(self.file_flux[f])
        return self._solve_elements(K, lambda: gen, xs, ndof, dim, sol0, list(bdc), P, P_amr, hanging, elem_levels, selective_levels,
                                    (flux_faces, flux_idx, flux_exprs, tau_faces, tau_vals), log, smoother, omega, keep)

    def _solve_elements(self, K, make_gen, xs, ndof, dim, sol0, bdc, P, P_amr, hanging, elem_levels, selective_levels, flux, log, smoother, omega, keep=None):
        """run_elements from the start vector on: K the top level's matrix, make_gen() its GenericAssembler, xs the top level's coordinates on the host, bdc[l] and
        P[l] of every level, flux = (flux_faces, flux_idx, flux_exprs, tau_faces, tau_vals) of the top level.  Returns the result dictionary without "levels".
        keep: a dict that receives "start", the vector the solve starts from (after it was made conforming)"""
        ctx, top = self.ctx, self.nlevels - 1
        flux_faces, flux_idx, flux_exprs, tau_faces, tau_vals = flux
        SOL, RES = ctx.vector(ndof), ctx.vector(ndof)
        SOL.upload(sol0)
        if selective_levels:
            bdc = [np.union1d(b, hanging[l]).astype(np.int32) for l, b in enumerate(bdc)]
            for l in range(1, self.nlevels):                          # PP[l] <- PP[l] * PPamr[l - 1] (LinearImplicitSystem.cpp:253-258), before the Dirichlet zeroing
                if P_amr[l - 1] is not None:
                    PA = P[l].matmul(P_amr[l - 1])
                    P[l].destroy()
                    P[l] = PA
            for q in P_amr[:top]:
                if q is not None:
                    q.destroy()
            if P_amr[top] is not None:                                # a conforming start
                RES.matrix_mult(SOL, P_amr[top])
                SOL.assign(RES)

        if keep is not None:
            keep["start"] = SOL.to_numpy()
        gen = make_gen()

        def assemble():
            gen.assemble(K, RES, sol=SOL, source=self.source, scale=1.0)
            if flux_faces:
                capi.assemble_neumann_edges(ctx, self.fe, np.array(flux_faces), np.array(flux_idx), flux_exprs, xs, RES)
            if tau_faces:                                             # by kind of face (a prism has quadrilaterals and triangles): the face element named
                for nn in sorted({len(f) for f in tau_faces}):
                    sel = [k for k, f in enumerate(tau_faces) if len(f) == nn]
                    fgeom = "lineface" if dim == 2 else "triface" if nn in (3, 6, 7) else "quadface"
                    capi.assemble_neumann_faces(ctx, fgeom, self.fe, np.array([tau_faces[k] for k in sel]), np.array([tau_vals[k] for k in sel]), xs, RES)

        try:
            history = self._mgsolve(K, P, bdc, SOL, RES, assemble, log, smoother, omega, P_amr=P_amr[top])
        finally:
            gen.destroy()
        out = {"solution": SOL.to_numpy(), "coords": xs[:ndof], "history": history, "converged": history[-1][1] < self.abs_tol, "dofs": ndof}
        if selective_levels:
            out["hanging"], out["elem_levels"] = hanging[top], elem_levels
        return out

    def _mgsolve(self, K, P, bdc, SOL, RES, assemble, log, smoother, omega, P_amr=None):
        """LinearImplicitSystem::MGsolve on a hierarchy built here: K the finest level's matrix, P[l] the transfer into level l (P[0] None), bdc[l] the Dirichlet
        dofs of level l, assemble() the callback that fills K and RES at SOL.  Rows of fine Dirichlet dofs and columns of coarse ones carry nothing in P
        (ZeroInterpolatorDirichletNodes).  Every linear iteration: the callback, the boundary rows, ||RES||_2 (stop below abs_conv_tol after the first, or after
        max_number_linear_iteration), the Galerkin chain PP^T KK PP and the boundary rows of every level, V-cycles under GMRES limited to 4 iterations (one level:
        the exact solve), SOL += EPS.  P_amr: the projection of a non-homogeneous finest level (LinearImplicitSystem.cpp:329-342, 487-491): after the callback
        RES <- P_amr^T RES and the operator of the cycle is P_amr^T K P_amr, whose boundary rows (bdc holds the hanging dofs too) are set; EPS <- P_amr EPS before
        SOL += EPS.  Returns the history [(Krylov steps, ||RES||_2)]; K, P and P_amr are destroyed"""
        top = self.nlevels - 1
        for l in range(1, self.nlevels):
            if bdc[l].size:
                P[l].mat_zero_rows(bdc[l], 0.0)
            if bdc[l - 1].size:
                P[l].zero_cols(bdc[l - 1])
        EPS = self.ctx.vector(RES.n_global)
        mg = capi.Multigrid(self.ctx, self.nlevels)
        A = [None] * self.nlevels
        A[top] = K if P_amr is None else None
        history = []
        its = 0
        for it in range(self.max_linear + 1):
            assemble()
            if P_amr is not None:
                EPS.matrix_mult_transpose(RES, P_amr)
                RES.assign(EPS)
                if A[top] is None:
                    A[top] = capi.Mat.ptap(P_amr, K)
                else:
                    A[top].ptap_numeric(P_amr, K)
            if bdc[top].size:
                A[top].mat_zero_rows(bdc[top], 1.0)
                RES.set(bdc[top], np.zeros(bdc[top].size))
            rn = RES.l2_norm()
            history.append((its, rn))
            if log:
                log("linear iteration %d: Linear Res L2norm = %.6e" % (it, rn))
            if (it > 0 and rn < self.abs_tol) or it == self.max_linear:
                break
            for l in range(top, 0, -1):
                if A[l - 1] is None:
                    A[l - 1] = capi.Mat.ptap(P[l], A[l])
                else:
                    A[l - 1].ptap_numeric(P[l], A[l])
            for l in range(top):
                if bdc[l].size:
                    A[l].mat_zero_rows(bdc[l], 1.0)
            for l in range(self.nlevels):
                mg.set_level(l, A[l], P[l], None, smoother, omega, self.npre if l > 0 else 1, self.npost if l > 0 else 0)
            mg.setup()
            EPS.zero()
            its, _ = mg.solve(RES, EPS, outer="gmres" if self.nlevels > 1 else "preonly", rtol=1e-12, atol=1e-20, maxit=4)
            if P_amr is not None:
                RES.matrix_mult(EPS, P_amr)
                EPS.assign(RES)
            SOL.add(1.0, EPS)
        mg.destroy()
        for m in A + P + ([K, P_amr] if P_amr is not None else []):
            if m is not None:
                m.destroy()
        return history

    def _pattern_from_elements(self, eds, ndof):
        """CSR pattern holding every (i, j) of every element; eds: one elem_dof array per shape.  Built on the device (fh_mat_create_from_elements) from one table
        padded to the widest shape with each element's first dof (a repeated dof adds no entry); the array version below serves rows the device builder's
        candidate lists do not hold"""
        width = max(ed.shape[1] for ed in eds)
        table = np.concatenate([np.concatenate([ed, np.broadcast_to(ed[:, :1], (ed.shape[0], width - ed.shape[1]))], axis=1) for ed in eds])
        try:
            return capi.Mat.from_elements(self.ctx, table, ndof)
        except capi.FemusHipError:
            pass
        keys = []
        for ed in eds:
            nc = ed.shape[1]
            r = np.repeat(ed, nc, axis=1).ravel().astype(np.int64)
            c = np.tile(ed, (1, nc)).ravel().astype(np.int64)
            keys.append(r * ndof + c)
        key = np.unique(np.concatenate(keys))
        rows, cols = key // ndof, key % ndof
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=ndof))])
        return capi.Mat.from_csr(self.ctx, ndof, ndof, indptr, cols)

    def _prolongator_from_children(self, groups, ed_c, ed_f, ndof_c, ndof_f):
        """PP of a level from the element prolongators (ElemType.cpp:439-532): fine element nchild e + j is child j of coarse element e; the row of a fine dof
        holds the coarse shape functions at its place in the father (the same row from every element that shares the dof).  groups: (shape, coarse elements of
        that shape, dofs per element)"""
        rows_l, cols_l, vals_l = [], [], []
        for geom, idx, nc in groups:                                # the order of ElemType.cpp's insertions: child, fine node, coarse function, element
            EP = capi.fe_elem_prolongator(geom, self.fe)
            nch = EP.shape[0]
            for j in range(nch):
                for n in range(nc):
                    rows = ed_f[nch * idx + j, n]
                    for k in np.nonzero(EP[j, n, :nc])[0]:
                        rows_l.append(rows)
                        cols_l.append(ed_c[idx, k])
                        vals_l.append(np.full(rows.size, EP[j, n, k]))
        rows, cols, vals = np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64), np.concatenate(vals_l)
        key = (rows * ndof_c + cols)[::-1]                          # INSERT_VALUES: the last insertion of an entry stays
        uniq, last = np.unique(key, return_index=True)
        rows, cols, vals = uniq // ndof_c, uniq % ndof_c, vals[::-1][last]
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=ndof_f))])
        return capi.Mat.from_csr(self.ctx, ndof_f, ndof_c, indptr, cols, vals)

    def _prolongator_from_links(self, groups, ed_c, ed_f, ndof_c, ndof_f, father, child):
        """PP into a level of mixed_mesh.refine_flagged, whose fine element f is child child[f] of father[f], or its unchanged copy (child -1).  First the
        insertions of _prolongator_from_children over the REFINED elements e alone, the fine row taken from the element whose (father, child) is (e, j); then
        the identity of the copies, ordered (shape, n < nc, e): exactly 1.0 at (ed_f[copy of e][n], ed_c[e][n]) (LinearImplicitSystem.cpp:761-811).  The last
        insertion of an entry stays, so a node a copy shares with a refined neighbour keeps the exact 1.0"""
        father, child = np.asarray(father, dtype=np.int64), np.asarray(child, dtype=np.int64)
        nch = int(child.max()) + 1 if child.size else 0
        fine_of = np.full((ed_c.shape[0], max(nch, 1)), -1, dtype=np.int64)       # [e, j] -> fine element; a copy sits at j = 0 of an element without children
        kids = child >= 0
        refined = np.zeros(ed_c.shape[0], dtype=bool)
        refined[father[kids]] = True
        fine_of[father, np.maximum(child, 0)] = np.arange(father.size)
        rows_l, cols_l, vals_l = [], [], []
        for geom, idx, nc in groups:
            EP = capi.fe_elem_prolongator(geom, self.fe)
            ref = idx[refined[idx]]
            for j in range(EP.shape[0] if ref.size else 0):
                for n in range(nc):
                    rows = ed_f[fine_of[ref, j], n]
                    for k in np.nonzero(EP[j, n, :nc])[0]:
                        rows_l.append(rows)
                        cols_l.append(ed_c[ref, k])
                        vals_l.append(np.full(rows.size, EP[j, n, k]))
        for geom, idx, nc in groups:
            cp = idx[~refined[idx]]
            for n in range(nc):
                rows_l.append(ed_f[fine_of[cp, 0], n])
                cols_l.append(ed_c[cp, n])
                vals_l.append(np.full(cp.size, 1.0))
        rows, cols, vals = np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64), np.concatenate(vals_l)
        key = (rows * ndof_c + cols)[::-1]                          # INSERT_VALUES: the last insertion of an entry stays
        uniq, last = np.unique(key, return_index=True)
        rows, cols, vals = uniq // ndof_c, uniq % ndof_c, vals[::-1][last]
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=ndof_f))])
        return capi.Mat.from_csr(self.ctx, ndof_f, ndof_c, indptr, cols, vals)

    # ---- the one-dimensional input (input/input1D.json: EDGE3 box) -------------------------------------------------------------------------------
    NU_1D, V_1D = 0.01, 1.0                      # main.cpp:392-395: in one dimension the callback is advection-diffusion with V = 1, nu = 0.01

    def line_mesh(self):
        """MeshGeneration.cpp:78-262 (nodes i / (2 nx), element i = {2 i, 2 i + 2, 2 i + 1}, face 0 of the first element "left", face 1 of the last
        "right") and the numbering every FEMuS mesh gets: vertices first, then the middles, each in order of first appearance"""
        nx, (xa, xb) = self.box[0], (self.lo[0], self.hi[0])
        x = np.array([(i / (2.0 * nx)) * (xb - xa) + xa for i in range(2 * nx + 1)])
        ed = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(nx)])
        new = np.full(2 * nx + 1, -1)
        k = 0
        for cls in ((0, 1), (2,)):
            for e in range(nx):
                for l in cls:
                    if new[ed[e, l]] < 0:
                        new[ed[e, l]] = k
                        k += 1
        xs = np.empty_like(x)
        xs[new] = x
        faces = {-2: (0, 0), -3: (nx - 1, 1)}                 # flag -> (element, local face = local node)
        return new[ed], xs, faces, nx + 1

    @staticmethod
    def refine_line(ed, xs, faces):
        """MeshRefinement::RefineMesh on EDGE3: element e -> children 2 e (at vertex 0) and 2 e + 1 (at vertex 1); vertex v of child j = coarse node
        fine2CoarseVertexMapping[j][v] ({0, 2}, {2, 1}); every child gets a new middle whose coordinate is the element prolongator's row (the quadratic map at
        xi = -1/2, +1/2); a child inherits the flag of the face its vertex lies on; then the numbering of every FEMuS mesh (vertices first, then middles, first touch)"""
        nel = ed.shape[0]
        f2c = ((0, 2), (2, 1))
        EP = capi.fe_elem_prolongator("line", "biquadratic")          # [child][local node][coarse function]
        raw = np.zeros((2 * nel, 3), dtype=np.int64)
        x = list(xs)
        for e in range(nel):
            for j in range(2):
                raw[2 * e + j, 0], raw[2 * e + j, 1] = ed[e, f2c[j][0]], ed[e, f2c[j][1]]
                raw[2 * e + j, 2] = len(x)
                x.append(sum(EP[j, 2, k] * xs[ed[e, k]] for k in range(3)))
        x = np.array(x)
        new = np.full(x.size, -1)
        k = 0
        for cls in ((0, 1), (2,)):
            for e in range(2 * nel):
                for l in cls:
                    if new[raw[e, l]] < 0:
                        new[raw[e, l]] = k
                        k += 1
        xf = np.empty_like(x)
        xf[new] = x
        ffaces = {flag: (2 * e + f, f) for flag, (e, f) in faces.items()}
        return new[raw], xf, ffaces, nel * 2 + 1

    def run_line(self, log=None, smoother=capi.SMOOTH_SOR, omega=1.0):
        """LinearImplicitSystem::MGsolve on the EDGE3 box with the callback's one-dimensional form (fh_assemble_advdiff_line) on the finest level, Galerkin
        operators below it, transfers from the line's element prolongator; one level (the shipped input): the exact solve.  smoother / omega: Richardson +
        SOR_PRECOND as main.cpp:240-242 sets them (scale 1 here: the natural-order sweep of a one-dimensional operator)"""
        ctx = self.ctx
        levels = [self.line_mesh()]
        for _ in range(1, self.nlevels):
            levels.append(self.refine_line(*levels[-1][:3]))
        nc = 2 if self.fe == "linear" else 3
        ndofs = [(nv if self.fe == "linear" else xs.size) for (_, xs, _, nv) in levels]
        top = self.nlevels - 1
        ed, xs, faces, nv = levels[top]
        ndof = ndofs[top]
        pairs = sorted({(int(a), int(b)) for e in ed for a in e[:nc] for b in e[:nc]})
        rows = np.array([p[0] for p in pairs])
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=ndof))])
        K = capi.Mat.from_csr(ctx, ndof, ndof, indptr, np.array([p[1] for p in pairs]))
        SOL, RES = ctx.vector(ndof), ctx.vector(ndof)
        sol0 = np.zeros(ndof)
        bdc, point_flux = [[] for _ in levels], []
        for flag in faces:
            kind, fn = self.face_bc(flag)
            for l, (edl, xl, fl, _) in enumerate(levels):
                e, f = fl[flag]
                node = int(edl[e, f])
                if kind == "dirichlet":
                    bdc[l].append(node)
                if l == top:
                    x4 = np.array([xl[node], 0.0, 0.0, 0.0])
                    if kind == "dirichlet":
                        sol0[node] = fn(x4) if fn is not None else 0.0
                    elif fn is not None:                      # non-homogeneous Neumann: the side "element" is a point, F[node] += g(x) (main.cpp:540-549)
                        point_flux.append((node, fn(x4)))
        bdc = [np.array(sorted(b), dtype=np.int32) for b in bdc]
        P = [None] + [self._prolongator_from_children([("line", np.arange(levels[l - 1][0].shape[0]), nc)], levels[l - 1][0], levels[l][0], ndofs[l - 1], ndofs[l])
                      for l in range(1, self.nlevels)]
        SOL.upload(sol0)

        def assemble():
            capi.assemble_advdiff_line(ctx, self.fe, ed, xs, K, RES, self.NU_1D, self.V_1D, sol=SOL, source=self.source)
            if point_flux:
                r = RES.to_numpy()
                for node, g in point_flux:
                    r[node] += g
                RES.upload(r)

        history = self._mgsolve(K, P, bdc, SOL, RES, assemble, log, smoother, omega)
        return {"solution": SOL.to_numpy(), "coords": xs[:ndof].reshape(-1, 1), "history": history, "converged": history[-1][1] < self.abs_tol, "dofs": ndof,
                "elem_dof": ed, "nodes": xs, "levels": [(l[0], l[1]) for l in levels]}

    def destroy(self):
        for e in list(self.bc_func.values()) + [self.source]:
            if e is not None:
                e.destroy()


if __name__ == "__main__":
    # python -m femus_amd.app_poisson input/input.json [output directory]   -- run from the application's directory, as the reference's executable is
    import sys
    import femus_amd
    if len(sys.argv) < 2:
        sys.exit("usage: python -m femus_amd.app_poisson <input.json> [output directory]")
    path = sys.argv[1]
    app = Poisson001(femus_amd.Context(0), path, base_dir=os.getcwd())
    out = app.run(log=print, output_dir=sys.argv[2] if len(sys.argv) > 2 else None) if app.dim > 1 else app.run(log=print)
    print("%d dofs, %d linear iteration(s), Linear Res L2norm %.3e, %s; max |Sol| = %.12g" % (out["dofs"], len(out["history"]), out["history"][-1][1],
                                                                                              "converged" if out["converged"] else "NOT converged",
                                                                                              float(np.abs(out["solution"]).max())))
    for f in out.get("files", []):
        print("wrote", f)
    app.destroy()
