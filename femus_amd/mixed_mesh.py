"""The meshes of applications/001_Poisson that the library's own mesh code does not build, on the host -- integers and coordinates only; all numerics run in
libfemus_hip.so: Gambit files of tetrahedra, prisms, triangles, or of several shapes (input/cube_Tet.neu, cube_Wedge.neu, cube_all_shapes*.neu: hexahedra,
tetrahedra and prisms in one file; the two-dimensional files of quadrilaterals and / or triangles the reference tree holds), and the TRI6 box.  A mesh is
(kind[nel] of "hex" / "tet" / "wedge" / "quad" / "tri", ed[nel, 27] padded with -1, xs[nnode, dim], ff[nel, 6] padded with -1, own[3]).

    read_gambit   GambitIO.cpp:101-330: HEX27 (type 4), TET10 (type 6), WEDGE18 (type 5), QUAD9 (type 2), TRI6 (type 3) ordered by (material, group, file index) as Mesh.cpp:626-690 orders them, nodes through
                  GambitToFemusVertexIndex (:55-69), faces through GambitToFemusFaceIndex (:84-86), flag = -(set name) - 1;
                  Mesh::AddBiquadraticNodesNotInMeshFile (Mesh.cpp:1207-1333): a node per TRIANGLE face -- shared between a tetrahedron and a prism as well --,
                  created by the first element that holds it, then a centre per tetrahedron / prism / triangle; coordinates with the weights of Mesh.cpp:105-122
    tri_box       MeshGeneration.cpp:283-650 (case 2, TRI6: lattice node i + j (2 nx + 1), two triangles per cell, faces named bottom / right / top / left = flags
                  -2 .. -5), the centre Mesh::AddBiquadraticNodesNotInMeshFile adds (-1/9 of the vertices + 4/9 of the middles, Mesh.cpp:124)
    refine        MeshRefinement::RefineMesh: children 8 e + j (4 e + j in two dimensions) of the father's shape, vertices through each shape's fine2CoarseVertexMapping (read off the element
                  prolongator), new edge / face nodes shared between neighbours of any shape, coordinates by the creating child's element prolongator
    refine_flagged  MeshRefinement::RefineMesh with an AMR flag (MeshRefinement.cpp:197-493, Elem.hpp:358-370): the flagged elements of the mesh's level give their
                  children, every other element one unchanged copy, in coarse element order; new nodes come from the children alone, by the keys and the
                  creating child of refine; the numbering walks all fine elements, copies included
    flag_elements   MeshRefinement::FlagElementsToRefine type 1: a function of the mean of an element's vertices and the level, elements of the level only
    amr_constraints  Mesh::GetAMRRestrictionAndAMRSolidMark (Mesh.cpp:1354-1830) for every shape, in the library on the host (fh_elem_amr_constraints_host): the hanging
                  dofs of a flagged level and their masters' weights
    boundary_faces / boundary_owners  the walk of GenerateBdc (MultiLevelSolution.cpp:762-800) as arrays: the faces of some flags in (element, face) order with the
                  family's nodes on them, and for every dof on them the flag of the last face that holds it -- the host statement of capi.ElementMesh's calls
    numbering     vertices, then edge middles, then the rest, each class in order of first appearance walking the elements
"""
import numpy as np

from . import capi

SHAPES = ("hex", "tet", "wedge", "quad", "tri")
NLOC = {"hex": 27, "tet": 15, "wedge": 21, "quad": 9, "tri": 7}
CLASSES = {"hex": (8, 20, 27), "tet": (4, 10, 15), "wedge": (6, 15, 21), "quad": (4, 8, 9), "tri": (3, 6, 7)}
NFACES = {"hex": 6, "tet": 4, "wedge": 5, "quad": 4, "tri": 3}
GAMBIT = {(4, 27): "hex", (6, 10): "tet", (5, 18): "wedge", (2, 9): "quad", (3, 6): "tri"}
G2F = {"hex": (4, 16, 0, 15, 23, 11, 7, 19, 3, 12, 20, 8, 25, 26, 24, 14, 22, 10, 5, 17, 1, 13, 21, 9, 6, 18, 2), "tet": (0, 4, 1, 6, 5, 2, 7, 8, 9, 3),
       "wedge": (3, 11, 5, 9, 10, 4, 12, 17, 14, 15, 16, 13, 0, 8, 2, 6, 7, 1), "quad": (0, 4, 1, 5, 2, 6, 3, 7, 8), "tri": (0, 3, 1, 4, 2, 5)}
GFACE = {"hex": (0, 4, 2, 5, 3, 1), "tet": (0, 1, 2, 3), "wedge": (2, 1, 0, 4, 3), "quad": (0, 1, 2, 3), "tri": (0, 1, 2)}
# Mesh.cpp:105-124: weights of the file's nodes in the nodes the file does not hold (tetrahedron: four faces and the centre; prism: two triangles and the centre;
# triangle: the centre)
ADDED = {"tet": np.array([[-1. / 9., -1. / 9., -1. / 9., 0, 4. / 9., 4. / 9., 4. / 9., 0, 0, 0], [-1. / 9., -1. / 9., 0, -1. / 9., 4. / 9., 0, 0, 4. / 9., 4. / 9., 0],
                          [0, -1. / 9., -1. / 9., -1. / 9., 0, 4. / 9., 0, 0, 4. / 9., 4. / 9.], [-1. / 9., 0, -1. / 9., -1. / 9., 0, 0, 4. / 9., 4. / 9., 0, 4. / 9.],
                          [-1. / 8.] * 4 + [1. / 4.] * 6]),
         "wedge": np.array([[-1. / 9.] * 3 + [0.] * 3 + [4. / 9.] * 3 + [0.] * 9, [0.] * 3 + [-1. / 9.] * 3 + [0.] * 3 + [4. / 9.] * 3 + [0.] * 6,
                            [0.] * 12 + [-1. / 9.] * 3 + [4. / 9.] * 3]),
         "tri": np.array([[-1. / 9.] * 3 + [4. / 9.] * 3])}
COMPLETE = ("hex", "quad")                 # shapes whose file elements hold every biquadratic node
_CLASSES = np.array([CLASSES[s] for s in SHAPES])         # [shape code][class]: the end of the class's local nodes
_T = {}


def tables(shape):
    """per shape: faces (local nodes of each face, vertices first), nvf (vertices per face), edges (the two vertices of each edge node), EP, f2c"""
    if shape not in _T:
        nv, ne, nl = CLASSES[shape]
        faces = [capi.fe_face_nodes(shape, "biquadratic", f) for f in range(NFACES[shape])]
        nvf = [{9: 4, 7: 3, 3: 2}[len(f)] for f in faces]             # quadrilateral, triangle, line
        x = np.array([capi.fe_node_ref_coords(shape, n) for n in range(nl)])
        edges = [[(a, b) for a in range(nv) for b in range(a + 1, nv) if np.allclose(0.5 * (x[a] + x[b]), x[m])][0] for m in range(nv, ne)]
        EP = capi.fe_elem_prolongator(shape, "biquadratic")
        f2c = np.array([[int(np.argmax(EP[j, v])) for v in range(nv)] for j in range(EP.shape[0])])
        _T[shape] = dict(faces=faces, nvf=nvf, edges=edges, EP=EP, f2c=f2c, face_local=[int(f[-1]) for f in faces])
    return _T[shape]


def first_touch(keys):
    """keys[n, w] integers (>= -2: -1 / -2 pad a short key).  Returns (id per row, index of the creating row per id): one id per distinct key row, numbered in
    order of first appearance.  The columns are packed into as few 64-bit words as their range allows (an edge or a triangle of a mesh below two million nodes
    is one word) and the words sorted; equal keys keep their order."""
    keys = np.asarray(keys, dtype=np.int64)
    n, w = keys.shape
    base = int(keys.max()) + 3 if n else 3
    words, cur, room = [], None, 1
    for c in range(w):
        col = keys[:, c] + 2
        if cur is not None and room * base < (1 << 62):
            cur = cur * base + col
            room *= base
        else:
            if cur is not None:
                words.append(cur)
            cur, room = col, base
    words.append(cur)
    if len(words) == 1 and room * n < (1 << 63):             # the row index fits beside the key: one sort of distinct values
        order = np.sort(words[0] * n + np.arange(n)) % n
    else:
        order = np.lexsort(words[::-1])
    new = np.ones(n, dtype=bool)
    new[1:] = False
    for wd in words:
        sw = wd[order]
        new[1:] |= sw[1:] != sw[:-1]
    group = np.cumsum(new) - 1
    first = order[new]                                   # the creating row of every group (equal keys in row order: the smallest index of the group)
    isfirst = np.zeros(n, dtype=bool)
    isfirst[first] = True
    rank = (np.cumsum(isfirst) - 1)[first]
    ids = np.empty(n, dtype=np.int64)
    ids[order] = rank[group]
    owner = np.empty(first.size, dtype=np.int64)
    owner[rank] = first
    return ids, owner


def _codes(kind):
    """the index in SHAPES of every element's shape"""
    code = np.zeros(len(kind), dtype=np.int64)
    for i, s in enumerate(SHAPES):
        code[kind == s] = i
    return code


def _renumber(code, raw, nnode):
    new = np.full(nnode, -1, dtype=np.int64)
    lo = np.zeros((raw.shape[0], 1), dtype=np.int64)
    k, own = 0, []
    for c in range(3):
        hi = _CLASSES[code, c][:, None]
        w = int(hi.max())
        col = np.arange(w)[None, :]
        seq = raw[:, :w][(col >= lo) & (col < hi)]            # element by element, local order
        seq = seq[new[seq] < 0]
        first = np.full(nnode, seq.size, dtype=np.int64)      # the position of every node's first appearance in seq
        np.minimum.at(first, seq, np.arange(seq.size))
        hit = np.zeros(seq.size + 1, dtype=bool)
        hit[first] = True
        uniq = seq[hit[:-1]]                                  # the class's nodes in order of first appearance
        new[uniq] = k + np.arange(uniq.size)
        k += uniq.size
        own.append(k)
        lo = hi
    return new, own


def _apply(new, raw):
    return np.where(raw >= 0, new[np.maximum(raw, 0)], -1)


def read_gambit(path, Lref=1.0, groups=False):
    tok = open(path).read().split()
    p = tok.index("NDFVL") + 1
    nvt, nel, ngroup, nbcd, dim, dim_nodes = (int(t) for t in tok[p:p + 6])
    if dim not in (2, 3):
        raise ValueError("%s: a %d-dimensional mesh" % (path, dim))
    if dim_nodes != dim:     # GambitIO.cpp:128, 246-270: the nodes carry NDFVL coordinates -- a surface in space (the Willmore / conformal applications)
        raise ValueError("%s: %d-dimensional elements with %d coordinates per node (a surface in space): not served" % (path, dim, dim_nodes))
    p = tok.index("COORDINATES") + 2
    xyz = np.array(tok[p:p + (1 + dim) * nvt], dtype=object).reshape(nvt, 1 + dim)[:, 1:].astype(float) / Lref
    p = tok.index("ELEMENTS/CELLS") + 2
    kind, raw = [], np.full((nel, 27), -1, dtype=np.int64)
    for e in range(nel):
        gt, nn = int(tok[p + 1]), int(tok[p + 2])
        if (gt, nn) not in GAMBIT or (NLOC[GAMBIT[(gt, nn)]] > 9) != (dim == 3):
            raise ValueError("%s: element %d of Gambit type %d with %d nodes: HEX27, TET10, WEDGE18, QUAD9 and TRI6 are served" % (path, e + 1, gt, nn))
        s = GAMBIT[(gt, nn)]
        kind.append(s)
        raw[e, list(G2F[s])] = np.array(tok[p + 3:p + 3 + nn], dtype=np.int64) - 1
        p += 3 + nn
    ff = np.full((nel, 6), -1, dtype=np.int64)
    q = 0
    for _ in range(nbcd):
        q = tok.index("CONDITIONS", q) + 2
        name, nface = int(tok[q]), int(tok[q + 2])
        q += 5
        for k in range(nface):
            e, f = int(tok[q + 3 * k]) - 1, int(tok[q + 3 * k + 2]) - 1
            ff[e, GFACE[kind[e]][f]] = -name - 1
        q += 3 * nface
    # triangle-face nodes, element by element and face by face; then the centres of tetrahedra and prisms
    ent_e, ent_l, keys = [], [], []
    for e in range(nel):
        T = tables(kind[e])
        for f in range(NFACES[kind[e]]):
            if T["nvf"][f] == 3 and dim == 3:
                ent_e.append(e)
                ent_l.append(T["face_local"][f])
                keys.append(sorted(raw[e, T["faces"][f][:3]].tolist()))
    nn = nvt
    if keys:
        ids, _ = first_touch(np.array(keys))
        raw[ent_e, ent_l] = nn + ids
        nn += int(ids.max()) + 1
    for e in range(nel):
        if kind[e] not in COMPLETE:
            raw[e, NLOC[kind[e]] - 1] = nn
            nn += 1
    coords = np.concatenate([xyz, np.zeros((nn - nvt, dim))])
    for e in range(nel):                                      # element by element: a shared face node keeps the later element's sum
        if kind[e] not in COMPLETE:
            W = ADDED[kind[e]]
            j0 = NLOC[kind[e]] - W.shape[0]
            for j in range(W.shape[0]):
                acc = np.zeros(dim)
                for i in range(j0):                           # the sum in the order of Mesh.cpp:1316-1324
                    acc += coords[raw[e, i]] * W[j][i]
                coords[raw[e, j0 + j]] = acc
    kind = np.array(kind)
    # GambitIO.cpp:290-321: group = the integer on the line under "GROUP:", material = its MATERIAL field; Mesh.cpp:626-690: the elements ordered by
    # (material, group, file index) -- after the added nodes were made in file order, before the nodes are numbered
    group, material = np.ones(nel, dtype=np.int64), np.zeros(nel, dtype=np.int64)
    q = 0
    for _ in range(ngroup):
        q = tok.index("GROUP:", q)
        ngel, mat, name = int(tok[q + 3]), int(tok[q + 5]), int(tok[q + 8])
        ids = np.array(tok[q + 10:q + 10 + ngel], dtype=np.int64) - 1
        group[ids], material[ids] = name, mat
        q += 10 + ngel
    order = np.lexsort((np.arange(nel), group, material))
    kind, raw, ff, group, material = kind[order], raw[order], ff[order], group[order], material[order]
    new, own = _renumber(_codes(kind), raw, nn)
    xs = np.empty_like(coords)
    xs[new] = coords
    out = (kind, _apply(new, raw), xs, ff, own)
    return out + (group, material) if groups else out


def tri_box(nx, ny, lo, hi):
    px = 2 * nx + 1
    jj, ii = np.meshgrid(np.arange(2 * ny + 1), np.arange(px), indexing="ij")
    xy = np.stack([(ii.ravel() / (2.0 * nx)) * (hi[0] - lo[0]) + lo[0], (jj.ravel() / (2.0 * ny)) * (hi[1] - lo[1]) + lo[1]], axis=1)
    idx = lambda i, j: i + j * px
    ed, ff = [], []
    for j in range(0, 2 * ny, 2):
        for i in range(0, 2 * nx, 2):
            ed.append([idx(i, j), idx(i + 2, j), idx(i + 2, j + 2), idx(i + 1, j), idx(i + 2, j + 1), idx(i + 1, j + 1)])
            ff.append([-2 if j == 0 else -1, -3 if i == 2 * (nx - 1) else -1, -1])
            ed.append([idx(i, j), idx(i + 2, j + 2), idx(i, j + 2), idx(i + 1, j + 1), idx(i + 1, j + 2), idx(i, j + 1)])
            ff.append([-1, -4 if j == 2 * (ny - 1) else -1, -5 if i == 0 else -1])
    nel, n6 = len(ed), xy.shape[0]
    raw = np.full((nel, 27), -1, dtype=np.int64)
    raw[:, :6] = ed
    raw[:, 6] = n6 + np.arange(nel)
    centres = np.zeros((nel, 2))
    for i in range(6):                                        # the sum in the order of Mesh.cpp:1316-1324
        centres += xy[raw[:, i]] * ADDED["tri"][0][i]
    coords = np.concatenate([xy, centres])
    new, own = _renumber(np.full(nel, SHAPES.index("tri")), raw, coords.shape[0])
    xs = np.empty_like(coords)
    xs[new] = coords
    fp = np.full((nel, 6), -1, dtype=np.int64)
    fp[:, :3] = ff
    return np.full(nel, "tri"), _apply(new, raw), xs, fp, own


def refine(kind, ed, xs, ff):
    nel, dim = ed.shape[0], xs.shape[1]
    nch = 8 if dim == 3 else 4
    code = _codes(kind)
    cc = np.repeat(code, nch)
    raw = np.full((nch * nel, 27), -1, dtype=np.int64)
    fff = np.full((nch * nel, 6), -1, dtype=np.int64)
    ent = {2: [], 3: [], 4: []}                               # (child, local node, key) of the shared new nodes by family: edges, triangles, quadrilaterals
    for i, s in enumerate(SHAPES):
        sel = np.nonzero(code == i)[0]
        if sel.size == 0:
            continue
        T = tables(s)
        nv = CLASSES[s][0]
        es = ed[sel]
        for j in range(nch):
            rows = nch * sel + j
            raw[rows, :nv] = es[:, T["f2c"][j]]
            for lf in range(NFACES[s]):
                for f in range(NFACES[s]):
                    if T["nvf"][lf] == T["nvf"][f] and all(int(T["f2c"][j][v]) in T["faces"][f].tolist() for v in T["faces"][lf][:T["nvf"][lf]]):
                        fff[rows, lf] = ff[sel, f]
        rows = (nch * sel[:, None] + np.arange(nch)[None, :]).ravel()
        v = raw[rows, :nv]
        E = np.array(T["edges"])
        a, b = v[:, E[:, 0]], v[:, E[:, 1]]
        ent[2].append((np.repeat(rows, len(E)), np.tile(nv + np.arange(len(E)), rows.size),
                       np.stack([np.minimum(a, b), np.maximum(a, b)], axis=2).reshape(-1, 2)))
        for n in ((3, 4) if dim == 3 else ()):                # (in two dimensions the faces ARE the edges)
            fs = [f for f in range(NFACES[s]) if T["nvf"][f] == n]
            if fs:
                key = np.sort(v[:, np.array([T["faces"][f][:n] for f in fs])], axis=2).reshape(-1, n)
                ent[n].append((np.repeat(rows, len(fs)), np.tile([T["face_local"][f] for f in fs], rows.size), key))
    # one key family at a time (an edge, a triangle and a quadrilateral never share a node): the first child that holds a key, in child-major order, creates its
    # node; the ids stand until _renumber numbers the nodes by their first appearance
    nxt = xs.shape[0]
    oc, ol = [], []
    for part in ent.values():
        if not part:
            continue
        c, loc, key = (np.concatenate(t) for t in zip(*part))
        if len(part) > 1:                                     # child by child (each shape's entries are in child, local order already)
            order = np.argsort(c, kind="stable")
            c, loc, key = c[order], loc[order], key[order]
        ids, owner = first_touch(key)
        raw[c, loc] = nxt + ids
        nxt += owner.size
        oc.append(c[owner])
        ol.append(loc[owner])
    allc = np.arange(nch * nel)
    centre = _CLASSES[cc, 2] - 1
    raw[allc, centre] = nxt + allc
    oc, ol = np.concatenate(oc + [allc]), np.concatenate(ol + [centre])       # creating (child, local node) of every new node
    pos = np.zeros((dim, oc.size))
    occ = cc[oc]
    xt = np.ascontiguousarray(xs.T)
    for i, s in enumerate(SHAPES):
        m = np.nonzero(occ == i)[0]
        if m.size:
            nl = NLOC[s]
            e, j = np.divmod(oc[m], nch)
            jl = j * nl + ol[m]
            EPt = tables(s)["EP"].transpose(2, 0, 1).reshape(nl, -1)        # [coarse function][child * nl + local node]
            edt = np.ascontiguousarray(ed[:, :nl].T)
            acc = np.zeros((dim, m.size))
            for k in range(nl):                                             # the sum over the father's nodes in their order
                w, node = EPt[k][jl], edt[k][e]
                for d in range(dim):
                    acc[d] += w * xt[d][node]
            pos[:, m] = acc
    coords = np.concatenate([xs, pos.T])
    new, own = _renumber(cc, raw, coords.shape[0])
    used = new >= 0
    xf = np.empty((own[2], dim))
    xf[new[used]] = coords[used]
    return np.repeat(kind, nch), _apply(new, raw), xf, fff, own


def refine_flagged(kind, ed, xs, ff, flags, lev=None, level=None):
    """selective refinement: (kind_f, ed_f, xs_f, ff_f, own_f, lev_f, father, child).  An element splits when flags[e] != 0 and lev[e] == level (an element of
    an older level never does); its nch children follow one another, of level + 1, father e, child j.  Every other element gives one copy -- its row of node
    ids, its face row, its level; father e, child -1.  New nodes are made by the children only, with the keys and the creating child of refine (a copy's edges
    and faces are at least father-sized: no child's new edge or face is one of them, so copies enter no key table); an old node keeps its coordinate bits.
    With every element flagged the first five results are refine's, with none the mesh comes back."""
    nel, dim = ed.shape[0], xs.shape[1]
    nch = 8 if dim == 3 else 4
    if lev is None:
        lev = np.full(nel, 0 if level is None else level, dtype=np.int64)
    lev = np.asarray(lev, dtype=np.int64)
    if level is None:
        level = int(lev.max()) if nel else 0
    eff = (np.asarray(flags).reshape(-1) != 0) & (lev == level)
    if eff.shape != (nel,):
        raise ValueError("refine_flagged: %d flags for %d elements" % (eff.size, nel))
    cnt = np.where(eff, nch, 1)
    start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    nel_f = int(start[-1])
    father = np.repeat(np.arange(nel, dtype=np.int64), cnt)
    child = np.where(eff[father], np.arange(nel_f) - start[father], -1)
    code = _codes(kind)
    cc = code[father]
    raw = np.full((nel_f, 27), -1, dtype=np.int64)
    fff = np.full((nel_f, 6), -1, dtype=np.int64)
    keep = np.nonzero(~eff)[0]
    raw[start[keep]], fff[start[keep]] = ed[keep], ff[keep]
    lev_f = np.where(child >= 0, level + 1, lev[father])
    ent = {2: [], 3: [], 4: []}                               # as in refine, over the children of the flagged elements
    for i, s in enumerate(SHAPES):
        sel = np.nonzero((code == i) & eff)[0]
        if sel.size == 0:
            continue
        T = tables(s)
        nv = CLASSES[s][0]
        es = ed[sel]
        for j in range(nch):
            rows = start[sel] + j
            raw[rows, :nv] = es[:, T["f2c"][j]]
            for lf in range(NFACES[s]):
                for f in range(NFACES[s]):
                    if T["nvf"][lf] == T["nvf"][f] and all(int(T["f2c"][j][v]) in T["faces"][f].tolist() for v in T["faces"][lf][:T["nvf"][lf]]):
                        fff[rows, lf] = ff[sel, f]
        rows = (start[sel][:, None] + np.arange(nch)[None, :]).ravel()
        v = raw[rows, :nv]
        E = np.array(T["edges"])
        a, b = v[:, E[:, 0]], v[:, E[:, 1]]
        ent[2].append((np.repeat(rows, len(E)), np.tile(nv + np.arange(len(E)), rows.size),
                       np.stack([np.minimum(a, b), np.maximum(a, b)], axis=2).reshape(-1, 2)))
        for n in ((3, 4) if dim == 3 else ()):
            fs = [f for f in range(NFACES[s]) if T["nvf"][f] == n]
            if fs:
                key = np.sort(v[:, np.array([T["faces"][f][:n] for f in fs])], axis=2).reshape(-1, n)
                ent[n].append((np.repeat(rows, len(fs)), np.tile([T["face_local"][f] for f in fs], rows.size), key))
    nxt = xs.shape[0]
    oc, ol = [], []
    for part in ent.values():
        if not part:
            continue
        c, loc, key = (np.concatenate(t) for t in zip(*part))
        if len(part) > 1:
            order = np.argsort(c, kind="stable")
            c, loc, key = c[order], loc[order], key[order]
        ids, owner = first_touch(key)
        raw[c, loc] = nxt + ids
        nxt += owner.size
        oc.append(c[owner])
        ol.append(loc[owner])
    fresh = np.nonzero(child >= 0)[0]
    centre = _CLASSES[cc[fresh], 2] - 1
    raw[fresh, centre] = nxt + np.arange(fresh.size)
    oc, ol = np.concatenate(oc + [fresh]).astype(np.int64), np.concatenate(ol + [centre]).astype(np.int64)
    pos = np.zeros((dim, oc.size))
    occ = cc[oc]
    xt = np.ascontiguousarray(xs.T)
    for i, s in enumerate(SHAPES):
        m = np.nonzero(occ == i)[0]
        if m.size:
            nl = NLOC[s]
            e, j = father[oc[m]], child[oc[m]]
            jl = j * nl + ol[m]
            EPt = tables(s)["EP"].transpose(2, 0, 1).reshape(nl, -1)
            edt = np.ascontiguousarray(ed[:, :nl].T)
            acc = np.zeros((dim, m.size))
            for k in range(nl):                                             # the sum over the father's nodes in their order
                w, node = EPt[k][jl], edt[k][e]
                for d in range(dim):
                    acc[d] += w * xt[d][node]
            pos[:, m] = acc
    coords = np.concatenate([xs, pos.T])
    new, own = _renumber(cc, raw, coords.shape[0])
    used = new >= 0
    xf = np.empty((own[2], dim))
    xf[new[used]] = coords[used]
    return kind[father], _apply(new, raw), xf, fff, own, lev_f, father, child


def flag_elements(kind, ed, xs, lev, level, fn):
    """fn(x[3], level) at the mean of the element's vertices, for the elements of the mesh's level; uint8[nel].  The mean is the vertices added in local order
    from +0.0, then one division by their number: the sum the device forms, so a centroid on a threshold flags the same on both sides"""
    nel, dim = ed.shape[0], xs.shape[1]
    out = np.zeros(nel, dtype=np.uint8)
    for e in range(nel):
        if lev[e] != level:
            continue
        nv = CLASSES[kind[e]][0]
        x = np.zeros(3)
        for v in range(nv):
            for d in range(dim):
                x[d] = x[d] + xs[ed[e, v], d]
        for d in range(dim):
            x[d] = x[d] / float(nv)
        out[e] = 1 if fn(x, level) else 0
    return out


_FACE_T = {}


def _face_tables(fam):
    """per shape code: loc[SHAPES, 6, 9] the family's local nodes on every face in the order of capi.fe_face_nodes, padded with -1, and n[SHAPES, 6] how many
    (0: the shape has no such face)"""
    if fam not in _FACE_T:
        fe = ("linear", "serendipity", "biquadratic")[fam]
        loc, n = np.full((len(SHAPES), 6, 9), -1, dtype=np.int64), np.zeros((len(SHAPES), 6), dtype=np.int64)
        for i, s in enumerate(SHAPES):
            for f in range(NFACES[s]):
                nodes = capi.fe_face_nodes(s, fe, f)
                loc[i, f, :nodes.size], n[i, f] = nodes, nodes.size
        _FACE_T[fam] = (loc, n)
    return _FACE_T[fam]


def _fam(fam):
    return capi.FE[fam] if isinstance(fam, str) else int(fam)


def boundary_faces(level, fam, flags):
    """the walk of GenerateBdc (MultiLevelSolution.cpp:762-800) over a level (kind, ed, xs, ff, ...): the faces whose flag is one of `flags`, elements in order
    and faces in order inside an element.  (elem[n], face[n], nodes[n, 9], nn[n]): nodes = ed[elem, fe_face_nodes(shape, family, face)] padded with -1, nn how
    many of them -- what the face loop of app_poisson.run_elements visits, in its order"""
    kind, ed, ff = level[0], np.asarray(level[1]), np.asarray(level[3])
    loc, n = _face_tables(_fam(fam))
    code = _codes(kind)
    hit = np.isin(ff, np.asarray(list(flags), dtype=np.int64)) & (np.arange(6)[None, :] < np.array([NFACES[s] for s in SHAPES])[code][:, None])
    elem, face = np.nonzero(hit)                                  # row-major: ascending (element, face)
    l = loc[code[elem], face]
    nodes = np.where(l >= 0, ed[elem[:, None], np.maximum(l, 0)], -1)
    return elem, face, nodes, n[code[elem], face]


def boundary_owners(level, fam, flags):
    """(dofs[n] ascending, owner_flag[n], coords[n, dim]): the dofs on the faces of boundary_faces, for each the flag of the LAST of those faces that holds it --
    in GenerateBdc a later face overwrites an earlier one, the rule of the dictionary in run_elements' face loop -- and its coordinates"""
    xs, ff = level[2], np.asarray(level[3])
    elem, face, nodes, nn = boundary_faces(level, fam, flags)
    k = np.broadcast_to(np.arange(elem.size)[:, None], nodes.shape)
    on = np.arange(9)[None, :] < nn[:, None]
    last = np.full(xs.shape[0], -1, dtype=np.int64)
    np.maximum.at(last, nodes[on], k[on])                         # faces are listed in ascending order: the last one is the largest index
    dofs = np.nonzero(last >= 0)[0]
    return dofs, ff[elem[last[dofs]], face[last[dofs]]], xs[dofs]


def amr_constraints(kind, ed, xs, ff, lev, fe, mode="reference"):
    """(hanging[n], ptr[n + 1], master[nnz], weight[nnz]) of a level whose elements have the levels lev[nel]: the hanging dofs of the family fe ("linear",
    "serendipity", "biquadratic") ascending, the masters ascending within a row.  mode "reference": chains resolved as the reference does; "coarsest": a node is
    described by the coarsest level that finds it and masters that hang themselves are expanded (rows sum to one).  Runs in the library, without a device"""
    import ctypes
    if mode not in ("reference", "coarsest"):
        raise capi.FemusHipError("mixed_mesh.amr_constraints: mode must be \"reference\" or \"coarsest\", not %r" % (mode,))
    kind, xs = np.asarray(kind), capi._f64(xs)
    code = np.zeros(kind.shape[0], dtype=np.int32)
    for name, c in capi.GEOM.items():
        code[kind == name] = c
    ed, ff, lev = capi._i32(ed), capi._i32(ff), capi._i32(lev)
    nel = kind.shape[0]
    if ed.shape != (nel, 27) or ff.shape != (nel, 6) or lev.shape != (nel,) or xs.ndim != 2:
        raise capi.FemusHipError("mixed_mesh.amr_constraints: ed must be [%d, 27], ff [%d, 6], lev [%d] and xs [nnode, dim]" % (nel, nel, nel))
    L = capi.load_library()
    k, md = capi.FE[fe] if isinstance(fe, str) else int(fe), 0 if mode == "reference" else 1
    args = (int(xs.shape[1]), nel, int(xs.shape[0]), capi._p(code), capi._p(ed), capi._p(xs), capi._p(ff), capi._p(lev), k, md)
    n, nnz = ctypes.c_int(0), ctypes.c_int(0)
    capi._chk(L.fh_elem_amr_constraints_host(*args, ctypes.byref(n), ctypes.byref(nnz), None, None, None, None))
    hang, ptr = np.empty(n.value, np.int32), np.empty(n.value + 1, np.int32)
    master, w = np.empty(nnz.value, np.int32), np.empty(nnz.value)
    capi._chk(L.fh_elem_amr_constraints_host(*args, ctypes.byref(n), ctypes.byref(nnz), capi._p(hang), capi._p(ptr), capi._p(master), capi._p(w)))
    return hang, ptr, master, w
