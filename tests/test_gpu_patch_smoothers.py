"""GPU parity of the block Schwarz smoothers (femus_amd/csrc/fh_patch.hip: FH_SMOOTH_VANKA, FH_SMOOTH_ASM) on patches and matrices that are no mesh
(tests/patch_cases.py; tests/test_patch_cases_host.py shows on the host what they exercise and how good the reference is).

Two-level wrapper, as for the natural-order sweeps in test_gpu_multigrid.py: level 0 is the identity, level 1 is A with P = I, npost = 0, so one
cycle returns z + (b - A z) with z the pre-smoothing from zero.  Error = max-norm distance to the oracle over the largest entry of the oracle's
result; bound 1e-12 (the project's bound for sweeps on unstructured patterns; the float64 oracle alone stays below 1e-13 of a long double sweep).

What runs where (patch sizes in dofs):
  k_patch_extract, k_patch_invert_lds   1..96, one and two rows per lane, levels whose largest small patch is 51, 96 or 100
  k_patch_invert                        97..512 behind k_patch_invert_lds, 1..512 alone (patch_invert_lds 0): one, two and three strides of 256 threads
  k_vanka_color_fused                   <= 64 (register branch) and 65..512, LDS strides of max_patch 51, 98, 100, 258, 512 on patches from 1 dof
  k_vanka_color, k_vanka_persistent<1>, <2>   the same patches (persistent: the 1..98 list and the scattered patches)
  k_patch_ilu0                          blocks of 1..512 rows, given in any order; a block that restarts on a shifted diagonal
  the pivot search and the interchanges of both inversion kernels: the systems numbered [pressure | velocity], whose sorted patches start with a zero."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import patch_cases as pc
from femus_amd import capi
from femus_amd.navier_stokes import NavierStokesMG
from oracle import femus_oracle as fo
from oracle import femus_oracle_ns as ns

pytestmark = pytest.mark.gpu
BOUND, BOUND_KRYLOV = 1e-12, 1e-10
DEFAULTS = (("vanka_persistent", 0), ("vanka_fused", 1), ("patch_invert_lds", 1))
SADDLE = [("saddle", name, order, "last") for name in pc.SIZE_LISTS for order in pc.ORDERS]
PIVOTING = [("saddle", name, "ascending", "first") for name in pc.SIZE_LISTS]          # [pressure | velocity]: row exchanges in every patch
SCATTERED, SCATTERED_SORTED = ("scattered", False), ("scattered", True)
FIRST_SHUFFLED = ("saddle", "edges_2_98", "shuffled", "last")


def ident(case):
    if case[0] == "scattered":
        return "scattered-sorted" if case[1] else "scattered"
    return "%s-%s%s" % (case[1], case[2], "-pressure_block_first" if case[3] == "first" else "")


def params(cases):
    return [pytest.param(c, id=ident(c)) for c in cases]


def build(case):
    if case[0] == "scattered":
        return pc.scattered(0, case[1])
    return pc.saddle(pc.SIZE_LISTS[case[1]], 0, case[2], case[3])


def err(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def options(ctx, persistent=0, fused=1, invert_lds=1):
    ctx.set_option("vanka_persistent", persistent)
    ctx.set_option("vanka_fused", fused)
    ctx.set_option("patch_invert_lds", invert_lds)


def restore(ctx):
    for name, value in DEFAULTS:
        ctx.set_option(name, value)


def csr_lists(patches):
    return np.concatenate([[0], np.cumsum([len(d) for d in patches])]), np.concatenate([np.asarray(d) for d in patches])


class TwoLevel:
    """identity coarse level under A with the block smoother; everything it makes is destroyed by destroy()"""

    def __init__(self, ctx, A, smoother, omega, npre):
        n = A.shape[0]
        I = sp.identity(n, format="csr")
        self.ctx, self.n, self.made = ctx, n, []
        self.A0, self.A1, self.P = (self.keep(ctx.matrix_scipy(M)) for M in (I, A, I))
        self.mg = self.keep(capi.Multigrid(ctx, 2))
        self.mg.set_level(0, self.A0, None, None, 0, 1.0, 1, 0)
        self.mg.set_level(1, self.A1, self.P, None, smoother, omega, npre, 0)

    def keep(self, o):
        self.made.append(o)
        return o

    def set_patches(self, patches):
        self.mg.set_level_patches(1, *csr_lists(patches))
        return self

    def cycle(self, b):
        bv, x = self.keep(self.ctx.vector_from(b)), self.keep(self.ctx.vector(self.n))
        self.mg.vcycle(bv, x)
        return x.to_numpy().copy()

    def destroy(self):
        for o in reversed(self.made):
            o.destroy()
        self.made = []


@functools.lru_cache(maxsize=None)
def rhs(n):
    return fo.lcg_fill(n, 7)


@functools.lru_cache(maxsize=None)
def vanka_reference(case, omega=0.7, npre=2):
    """z + (b - A z), z = npre sweeps of the oracle's smoother on the oracle's colours of the patches as given"""
    A, patches = build(case)
    b = rhs(A.shape[0])
    sm = ns.VankaSmoother(A, patches, ns.color_patches(patches, A), omega)
    z = np.zeros(A.shape[0])
    for _ in range(npre):
        z = sm.sweep(b, z)
    ref = z + (b - A @ z)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def asm_smoother(case, n_exact):
    A, patches = build(case)
    return ns.AsmSmoother(A, patches, 1.0, n_exact=len(patches) if n_exact == "all" else n_exact)


@functools.lru_cache(maxsize=None)
def asm_reference(case, n_exact, solver="richardson", omega=0.8, npre=2):
    A, _ = build(case)
    b = rhs(A.shape[0])
    sm = asm_smoother(case, n_exact)
    if solver == "richardson":
        z = fo.smooth_precond(A, b, np.zeros_like(b), omega, npre, True, sm.apply)
    else:
        z = fo.smooth_gmres(A, b, np.zeros_like(b), npre, True, sm.apply)
    ref = z + (b - A @ z)
    ref.setflags(write=False)
    return ref


def vanka_cycle(ctx, case, omega=0.7, npre=2, cycles=1):
    A, patches = build(case)
    w = TwoLevel(ctx, A, capi.SMOOTH_VANKA, omega, npre)
    try:
        w.set_patches(patches).mg.setup()
        out = [w.cycle(rhs(A.shape[0])) for _ in range(cycles)]
    finally:
        w.destroy()
    return out[0] if cycles == 1 else out


# ---- a. Vanka ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persistent,fused,invert_lds", [(0, 1, 1), (0, 0, 1), (0, 1, 0)])
@pytest.mark.parametrize("case", params(SADDLE + PIVOTING + [SCATTERED]))
def test_vanka_sweeps_match_oracle(ctx, case, persistent, fused, invert_lds):
    """omega = 0.7, two sweeps (the second starts from a non-zero x): one launch per colour (fused), residual of the level + one launch per colour
    (unfused), patch inverses by the wave kernel in LDS and by the workgroup kernel on global memory"""
    try:
        options(ctx, persistent, fused, invert_lds)
        e = err(vanka_cycle(ctx, case), vanka_reference(case))
        print("vanka %s, vanka_persistent %d vanka_fused %d patch_invert_lds %d: %.2e from the oracle" % (ident(case), persistent, fused, invert_lds, e))
        assert e < BOUND
    finally:
        restore(ctx)


@pytest.mark.parametrize("persistent,fused,invert_lds", [(1, 1, 1), (2, 1, 0)])
@pytest.mark.parametrize("case", params([FIRST_SHUFFLED, SCATTERED]))
def test_vanka_persistent_sweeps_match_oracle(ctx, case, persistent, fused, invert_lds):
    """all colours of both sweeps in one launch, both forms of the device-wide barrier (grids of a handful of workgroups here)"""
    try:
        options(ctx, persistent, fused, invert_lds)
        e = err(vanka_cycle(ctx, case), vanka_reference(case))
        print("vanka %s, vanka_persistent %d patch_invert_lds %d: %.2e from the oracle" % (ident(case), persistent, invert_lds, e))
        assert e < BOUND
    finally:
        restore(ctx)


# ---- b. the same bits where the code says so -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", params([FIRST_SHUFFLED, ("saddle", "edges_2_98", "ascending", "first"), SCATTERED]))
def test_both_inversion_kernels_give_the_same_bits(ctx, case):
    """k_patch_invert_lds states that it keeps the pivot rule and the arithmetic per entry of k_patch_invert"""
    try:
        got = []
        for lds in (1, 0):
            options(ctx, 0, 1, lds)
            got.append(vanka_cycle(ctx, case))
        assert np.array_equal(got[0], got[1])
    finally:
        restore(ctx)


@pytest.mark.parametrize("case", params([FIRST_SHUFFLED, SCATTERED]))
def test_both_barrier_forms_give_the_same_bits(ctx, case):
    try:
        got = []
        for persistent in (1, 2):
            options(ctx, persistent, 1, 1)
            got.append(vanka_cycle(ctx, case))
        assert np.array_equal(got[0], got[1])
    finally:
        restore(ctx)


@pytest.mark.parametrize("persistent,fused", [(0, 1), (0, 0), (1, 1), (2, 1)])
@pytest.mark.parametrize("case", params([FIRST_SHUFFLED, SCATTERED]))
def test_repeated_cycles_and_a_fresh_object_give_the_same_bits(ctx, case, persistent, fused):
    """three cycles in a row on one object (the replayed graph; the barrier counters of the persistent sweep go back to zero), then a fresh Multigrid
    given the same matrix and patches"""
    try:
        options(ctx, persistent, fused, 1)
        first, second, third = vanka_cycle(ctx, case, cycles=3)
        assert np.array_equal(first, second) and np.array_equal(first, third)
        assert np.array_equal(first, vanka_cycle(ctx, case))
    finally:
        restore(ctx)


# ---- c. Vanka under the GMRES level solver -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", params([("saddle", "edges_256", "shuffled", "last"), ("saddle", "edges_2_98", "ascending", "first"), SCATTERED]))
def test_vanka_under_the_gmres_level_solver(ctx, case):
    """three GMRES iterations preconditioned by one Vanka sweep (omega = 1) from zero, against fo.smooth_gmres.  Bound 1e-10: the project's bound for
    Krylov steps against a host restatement, taken from test_fgmres_around_gmres_smoothed_cycles (test_gpu_multigrid.py), which holds cycles whose level
    solvers are GMRES to 1e-10 of the oracle's"""
    A, patches = build(case)
    b = rhs(A.shape[0])
    sm = ns.VankaSmoother(A, patches, ns.color_patches(patches, A), 1.0)
    z = fo.smooth_gmres(A, b, np.zeros_like(b), 3, True, lambda r: sm.sweep(r, np.zeros_like(r)))
    ref = z + (b - A @ z)
    w = TwoLevel(ctx, A, capi.SMOOTH_VANKA, 0.7, 3)
    try:
        w.set_patches(patches)
        w.mg.set_level_solver(1, "gmres", 30)
        w.mg.setup()
        e = err(w.cycle(b), ref)
        print("vanka %s under 3 GMRES iterations: %.2e from the oracle" % (ident(case), e))
        assert e < BOUND_KRYLOV
    finally:
        w.destroy()


# ---- d. PCASM ------------------------------------------------------------------------------------------------------------------------
def asm_cycle(ctx, case, n_exact, solver="richardson", omega=0.8, npre=2):
    A, patches = build(case)
    w = TwoLevel(ctx, A, capi.SMOOTH_ASM, omega, npre)
    try:
        w.set_patches(patches)
        w.mg.set_level_patches_exact(1, len(patches) if n_exact == "all" else n_exact)
        if solver == "gmres":
            w.mg.set_level_solver(1, "gmres", 30)
        w.mg.setup()
        return w.cycle(rhs(A.shape[0]))
    finally:
        w.destroy()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n_exact", [0, 2, "all"])
@pytest.mark.parametrize("case", params(SADDLE + [SCATTERED_SORTED, SCATTERED]))
def test_pcasm_blocks_match_oracle(ctx, case, n_exact, fused):
    """the blocks in their index order, ILU(0) of every block in ASCENDING dof order whatever order the caller listed it in (the reference sorts each
    block, LinearEquationSolverPetscAsm.cpp:253-254, and so does the oracle), the first n_exact blocks exactly; Richardson, omega = 0.8, two sweeps"""
    try:
        options(ctx, 0, fused, 1)
        e = err(asm_cycle(ctx, case, n_exact), asm_reference(case, n_exact))
        print("pcasm %s, %s exact blocks, vanka_fused %d: %.2e from the oracle" % (ident(case), n_exact, fused, e))
        assert e < BOUND
    finally:
        restore(ctx)


@pytest.mark.parametrize("case,n_exact", [pytest.param(("saddle", "edges_256", "ascending", "last"), 2, id="edges_256-ascending-2"),
                                          pytest.param(SCATTERED_SORTED, 0, id="scattered-sorted-0")])
def test_pcasm_under_the_gmres_level_solver(ctx, case, n_exact):
    """two GMRES iterations preconditioned by one PCASM application, the reference built as in test_pcasm_as_the_reference_configures_it"""
    e = err(asm_cycle(ctx, case, n_exact, "gmres"), asm_reference(case, n_exact, "gmres"))
    print("pcasm %s, %s exact blocks, GMRES level solver: %.2e from the oracle" % (ident(case), n_exact, e))
    assert e < BOUND_KRYLOV


# ---- e. a block that takes the shift -------------------------------------------------------------------------------------------------
def test_pcasm_block_that_takes_the_shift(ctx):
    """the matrix of test_ilu0_shift_on_a_zero_pivot (u_11 cancels exactly) in two overlapping blocks, rows 0..19 and 15..39: ILU(0) of the first
    restarts on A_pp + shift I -- the first time k_patch_ilu0 does -- and device and oracle take the same shift.  Asserts and bounds of that test:
    the entries that go through the shifted pivot (~ 2 shift = 4.4e-14, itself known to 0.3 %) agree to 1e-2, the others to 1e-9"""
    n = 40
    M = sp.lil_matrix((n, n))
    for i in range(n):
        M[i, i] = 2.0
        if i + 1 < n:
            M[i, i + 1] = M[i + 1, i] = -1.0
    M[0, 0], M[0, 1], M[1, 0], M[1, 1] = 1.0, 1.0, 1.0, 1.0
    M = M.tocsr()
    patches = [np.arange(0, 20), np.arange(15, 40)]
    sm = ns.AsmSmoother(M, patches, 1.0)
    assert sm.ilu[0][2] > 0.0 and sm.ilu[1][2] == 0.0
    b = fo.lcg_fill(n, 2)
    z = sm.apply(b)
    ref = z + (b - M @ z)
    w = TwoLevel(ctx, M, capi.SMOOTH_ASM, 1.0, 1)
    try:
        w.set_patches(patches).mg.setup()
        got = w.cycle(b)
    finally:
        w.destroy()
    rel = lambda a, r: np.linalg.norm(a - r) / np.linalg.norm(r)
    print("pcasm with a shifted block: %.2e overall, %.2e away from the shifted pivot" % (rel(got, ref), rel(got[5:], ref[5:])))
    assert np.all(np.isfinite(got)) and rel(got, ref) < 1e-2 and rel(got[5:], ref[5:]) < 1e-9


# ---- f. refusals -----------------------------------------------------------------------------------------------------------------------
def bad_lists(A, patches):
    """(what, patches, the call that refuses, words the message must hold)"""
    n = A.shape[0]
    dup = list(patches[4])
    dup[-1] = dup[0]
    return [("513 dofs", patches[:1] + [np.arange(513)] + patches[1:], "set", ["patch 1", "513"]),
            ("an empty patch", patches[:2] + [np.array([], dtype=np.int64)] + patches[2:], "set", ["patch 2", "0 dofs"]),
            ("a dof beyond the matrix", patches[:3] + [np.array([5, n, 7])] + patches[3:], "setup", ["dof %d" % n, "out of range"]),
            ("a dof listed twice", patches[:4] + [np.array(dup)] + patches[5:], "set", ["patch 4", "dof %d" % dup[0], "twice"])]


@pytest.mark.parametrize("which", range(4))
def test_refused_patch_lists(ctx, which):
    """a list the smoother cannot take raises, says what is wrong with it, and leaves the Multigrid usable: the good list after it gives the oracle's
    result"""
    A, patches = build(FIRST_SHUFFLED)
    what, bad, where, words = bad_lists(A, patches)[which]
    w = TwoLevel(ctx, A, capi.SMOOTH_VANKA, 0.7, 2)
    try:
        if where == "set":
            with pytest.raises(capi.FemusHipError) as ei:
                w.set_patches(bad)
        else:
            w.set_patches(bad)
            with pytest.raises(capi.FemusHipError) as ei:
                w.mg.setup()
        print("%s: %s" % (what, ei.value))
        assert all(s in str(ei.value) for s in words)
        w.set_patches(patches).mg.setup()
        e = err(w.cycle(rhs(A.shape[0])), vanka_reference(FIRST_SHUFFLED))
        assert e < BOUND
    finally:
        w.destroy()


@pytest.mark.parametrize("invert_lds", [1, 0])
def test_structurally_singular_patch_is_refused_at_setup(ctx, invert_lds):
    """two pressure dofs and nothing else: an exactly zero 2 x 2 matrix, refused by either inversion kernel, naming the patch"""
    A, patches = build(FIRST_SHUFFLED)
    n = A.shape[0]
    assert not A[[n - 1, n - 2]][:, [n - 1, n - 2]].toarray().any()
    w = TwoLevel(ctx, A, capi.SMOOTH_VANKA, 0.7, 2)
    try:
        options(ctx, 0, 1, invert_lds)
        w.set_patches(patches[:6] + [np.array([n - 1, n - 2])] + patches[6:])
        with pytest.raises(capi.FemusHipError) as ei:
            w.mg.setup()
        print("singular patch, patch_invert_lds %d: %s" % (invert_lds, ei.value))
        assert "patch 6" in str(ei.value) and "singular" in str(ei.value)
        w.set_patches(patches).mg.setup()
        assert err(w.cycle(rhs(n)), vanka_reference(FIRST_SHUFFLED)) < BOUND
    finally:
        restore(ctx)
        w.destroy()


# ---- g. the 3-D cycle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_vanka_vcycle_matches_oracle_in_three_dimensions(ctx, fused):
    """the body of test_vanka_vcycle_matches_oracle (test_gpu_ns.py) on the 2 x 2 x 2 HEX27 cavity with two levels: 2 312 unknowns, 125 patches of
    82..376 dofs -- the branch of k_vanka_color_fused beyond 64 dofs and every stride of k_patch_invert on the patches of a mesh.  Lid as in
    test_three_dimensional_cavity_matches_oracle; one multiplicative V(2,2) cycle on the Jacobian of a random state, bound 1e-9 as in two dimensions
    (largest patch condition number 8e2)"""
    LO, HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
    lo, hi = np.array(LO), np.array(HI)

    def bc(x, name, face):
        if name == "P":
            return bool(np.all(x < lo + 1e-8)), 0.0
        return True, (1.0 if (name == "U" and face == 6 and lo[0] < x[0] < hi[0]) else 0.0)

    pb = None
    try:
        options(ctx, 0, fused, 1)
        nu, nl, top = 0.05, 2, 1
        pb = NavierStokesMG(ctx, 2, 2, 2, nl, nu, boundary_condition=bc).init()
        ms, lays = ns.build_ns_levels(2, 2, 2, nl, LO, HI)
        bcs = [ns.cavity_bc(m, l, lid_flag=-7, lid_component=0) for m, l in zip(ms, lays)]
        sizes = np.diff(pb.patches[top][0])
        assert lays[top].n == 2312 and sizes.size == 125 and sizes.min() == 82 and sizes.max() == 376
        rng = np.random.default_rng(5)
        state = 0.3 * rng.standard_normal(lays[top].n)
        state[bcs[top][0]] = bcs[top][1]
        pb.SOL[top].upload(state)
        mg = pb.prepare(top)
        H = ns.newton_step_operators(ms, lays, bcs, top, state, nu, omega=pb.omega, npre=pb.npre, npost=pb.npost)
        for l in range(nl):
            assert np.array_equal(pb.bdc[l], bcs[l][0])
            assert abs(pb.A[(top, l)].to_scipy() - H.A[l]).max() <= 1e-11 * abs(H.A[l]).max()
        b = rng.standard_normal(lays[top].n)
        b[bcs[top][0]] = 0.0
        x = ctx.vector(lays[top].n)
        mg.vcycle(ctx.vector_from(b), x)
        ref = ns.vcycle(H, top, b)
        e = np.linalg.norm(x.to_numpy() - ref) / np.linalg.norm(ref)
        print("HEX27 cavity, vanka_fused %d: %.2e from the oracle's cycle" % (fused, e))
        assert e < 1e-9
    finally:
        restore(ctx)
        if pb is not None:
            pb.destroy()
