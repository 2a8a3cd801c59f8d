"""TEST INFRASTRUCTURE ONLY.  A literal restatement of Solution::FlagAMRRegionBasedOnErroNormAdaptive (Solution.cpp:843-1101) for one variable and one process,
in plain Python loops: the yardstick of fh_elem_error_flag_host and fh_elem_mesh_error_flag.  It keeps the ascending walk, the 0 / 1 / 2 state of the AMR
vector, the jel > iel / jel < iel branches, the += / -= on errTestTrue2, and takes the neighbours from a vertex-to-elements table built as
elem::BuildElementNearVertex / BuildElementNearElement (Elem.cpp:495-548) do.  Weight, phi and gradphi of every Gauss point come from
oracle.femus_oracle.ElemType.jacobian (the family's own Jacobian: the geometry map over the family's first nc nodes).

The expensive half -- the Gauss-point values of every element, which do not depend on the thresholds -- is gauss_values(); walk() is the rest of the routine."""
import math

import numpy as np

from oracle import femus_oracle as fo
from oracle import femus_oracle_mixed as om

SCALE2 = [[0.111111, 1.], [0.0204081632653, 0.111111], [0.0204081632653, 0.111111]]
FE = ("linear", "serendipity", "biquadratic")
NV = {s: om.CLASSES[s][0] for s in om.CLASSES}
NORM = {"L2": 0, "l2": 0, "H0": 0, "h0": 0, "H1": 1, "h1": 1}


def elem_type(shape, fe, order):
    """ElemType of any shape: the class itself for hexahedra and quadrilaterals; for the others an object of the class filled with the shape's tables, so that
    its jacobian() is the one that runs"""
    if shape in ("hex", "quad"):
        return fo.ElemType(shape, fe, order)
    et = object.__new__(fo.ElemType)
    w, phi, dphi = om.tables(shape, fe, order)
    et.geom, et.fe, et.order = shape, fe, order
    et.w, et.phi, et.dphi, et.d2phi = np.asarray(w), np.asarray(phi), np.asarray(dphi), None
    et.ng, et.nc, et.dim = et.w.size, et.phi.shape[1], et.dphi.shape[2]
    return et


def gauss_values(kind, ed, xs, fe, sol, eps, order="seventh"):
    """per element a list over its Gauss points of (weight, solig, solGradig[dim], errig, errGradig[dim], aerrig, aerrGradig[dim]): the sums of the two loops over
    i at Solution.cpp:928-936 and :1019-1027 (the gradient sums as for normType > 0), and the error's sums again with every product replaced by its absolute value"""
    fe = FE[fe] if not isinstance(fe, str) else fe
    dim = xs.shape[1]
    ets = {s: elem_type(s, fe, order) for s in sorted(set(kind.tolist()))}
    out = []
    for iel in range(kind.shape[0]):
        et = ets[kind[iel]]
        solDofs = et.nc
        dof = [int(ed[iel, i]) for i in range(solDofs)]
        s_loc = [float(sol[d]) for d in dof]
        e_loc = [float(eps[d]) for d in dof]
        x = [[float(xs[d, j]) for d in dof] for j in range(dim)]
        pts = []
        for ig in range(et.ng):
            weight, phi, phi_x = et.jacobian(x, ig)
            solig = errig = aerrig = 0.
            solGradig, errGradig, aerrGradig = [0.] * dim, [0.] * dim, [0.] * dim
            for i in range(solDofs):
                solig += phi[i] * s_loc[i]
                errig += phi[i] * e_loc[i]
                aerrig += abs(phi[i] * e_loc[i])
                for j in range(dim):
                    solGradig[j] += s_loc[i] * phi_x[i * dim + j]
                    errGradig[j] += e_loc[i] * phi_x[i * dim + j]
                    aerrGradig[j] += abs(e_loc[i] * phi_x[i * dim + j])
            pts.append((float(weight), float(solig), [float(v) for v in solGradig], float(errig), [float(v) for v in errGradig], float(aerrig),
                        [float(v) for v in aerrGradig]))
        out.append(pts)
    return out


def near_elements(kind, ed):
    """_elementNearElement: row iel = iel, then the other elements that share one of its vertices, ascending (a std::map's order)"""
    nel = kind.shape[0]
    near_vertex = {}
    for iel in range(nel):
        for inode in range(NV[kind[iel]]):
            near_vertex.setdefault(int(ed[iel, inode]), []).append(iel)
    rows = []
    for iel in range(nel):
        elements = {}
        for i in range(NV[kind[iel]]):
            for jel in near_vertex[int(ed[iel, i])]:
                if jel != iel:
                    elements[jel] = True
        rows.append([iel] + sorted(elements))
    return rows


def walk(values, kind, ed, lev, level, fe, norm, threshold, neighbor_threshold, dim):
    """the routine from its first element loop on.  Returns a dict: flags (the AMR vector at the end, 0 / 1), err2, vol, B (the integrand of err with absolute
    products), sums = [solNorm2, volume, volumeRefined, volumeTestFalse, errTestTrue2], threshold (the new one), nflagged, converged, and `strong` / `weak`
    (the two comparisons of every refinable element, for the conditions a test puts on its own inputs); errMoved, the magnitudes the walk added to and took
    from errTestTrue2 (its own rounding error is relative to that, not to what is left), and errTestTrue2_exact, the sum of err_i over the refinable elements
    that end unflagged (math.fsum)"""
    solType = FE.index(fe) if isinstance(fe, str) else int(fe)
    normType = NORM[norm] if isinstance(norm, str) else int(norm)
    nel = kind.shape[0]
    can_refine = [int(lev[iel]) == level for iel in range(nel)]
    scale2 = SCALE2[solType][normType]
    solNorm2 = volumeRefined = volume = 0.
    for iel in range(nel):
        for (weight, solig, solGradig, _e, _eg, _a, _ag) in values[iel]:
            solNorm2 += solig * solig * weight
            if normType > 0:
                for j in range(dim):
                    solNorm2 += solGradig[j] * solGradig[j] * weight
            volume += weight
            if can_refine[iel]:
                volumeRefined += weight
    volumeTestFalse = errTestTrue2 = errMoved = 0.
    eps2 = threshold * threshold * solNorm2 / volume if nel else 0.
    ielVolume, ielErrNorm2, B = [0.] * nel, [0.] * nel, [0.] * nel
    AMR = [0.] * nel
    near = near_elements(kind, ed)
    for iel in range(nel):
        if can_refine[iel]:
            for (weight, _s, _sg, errig, errGradig, aerrig, aerrGradig) in values[iel]:
                ielErrNorm2[iel] += scale2 * errig * errig * weight
                B[iel] += scale2 * aerrig * aerrig * abs(weight)
                if normType > 0:
                    for j in range(dim):
                        ielErrNorm2[iel] += scale2 * errGradig[j] * errGradig[j] * weight
                        B[iel] += scale2 * aerrGradig[j] * aerrGradig[j] * abs(weight)
                ielVolume[iel] += weight
            if ielErrNorm2[iel] > eps2 * ielVolume[iel] or (AMR[iel] == 2. and ielErrNorm2[iel] > neighbor_threshold * eps2 * ielVolume[iel]):
                AMR[iel] = 1.
                volumeTestFalse += ielVolume[iel]
                if ielErrNorm2[iel] > eps2 * ielVolume[iel]:
                    for j in range(1, len(near[iel])):
                        jel = near[iel][j]
                        if can_refine[jel]:
                            if jel > iel:
                                AMR[jel] = 2.
                            elif AMR[jel] == 0. and ielErrNorm2[jel] > neighbor_threshold * eps2 * ielVolume[jel]:
                                errTestTrue2 -= ielErrNorm2[jel]
                                errMoved += ielErrNorm2[jel]
                                AMR[jel] = 1.
                                volumeTestFalse += ielVolume[jel]
            else:
                AMR[iel] = 0.
                errTestTrue2 += ielErrNorm2[iel]
                errMoved += ielErrNorm2[iel]
    if volumeTestFalse != 0:
        new_threshold = math.sqrt(threshold * threshold * volumeRefined / volumeTestFalse - errTestTrue2 / solNorm2 * volume / volumeTestFalse)
    else:
        new_threshold = 1.
    counter = sum(abs(a) for a in AMR)
    ref = [iel for iel in range(nel) if can_refine[iel]]
    return {"flags": np.array([1 if a == 1. else 0 for a in AMR], dtype=np.uint8), "err2": np.array(ielErrNorm2), "vol": np.array(ielVolume), "B": np.array(B),
            "sums": np.array([solNorm2, volume, volumeRefined, volumeTestFalse, errTestTrue2]), "eps2": eps2, "threshold": new_threshold,
            "nflagged": int(counter), "converged": counter * 2 ** dim <= 1, "refinable": np.array(can_refine, dtype=bool), "near": near,
            "strong": np.array([can_refine[i] and ielErrNorm2[i] > eps2 * ielVolume[i] for i in range(nel)], dtype=bool),
            "weak": np.array([can_refine[i] and ielErrNorm2[i] > neighbor_threshold * eps2 * ielVolume[i] for i in range(nel)], dtype=bool),
            "nterms": sum(len(values[i]) for i in range(nel)), "nref": len(ref), "errMoved": errMoved,
            "errTestTrue2_exact": math.fsum(ielErrNorm2[i] for i in ref if AMR[i] != 1.)}


def flag_reference(kind, ed, xs, lev, level, fe, sol, eps, norm, threshold, neighbor_threshold=0., order="seventh"):
    return walk(gauss_values(kind, ed, xs, fe, sol, eps, order), kind, ed, lev, level, fe, norm, threshold, neighbor_threshold, xs.shape[1])
