"""The small dense algebra of GMRES (femus_amd/csrc/fh_hessenberg.h: one Hessenberg column through the Givens rotations, the back substitution) without
a device: the functions the device kernel k_gm_step and the host-driven loop share, compiled into a stand-alone program (tests/krylov_host_main.cpp) and
fed fixed upper-Hessenberg matrices one column at a time, against numpy.linalg.lstsq on the same matrices.  The program is built a second time with the
address and undefined-behaviour sanitizers and run directly.

Tolerance: TOL_MULTIPLE * eps * cond(H).  Givens QR of an (m + 1) x m Hessenberg matrix is backward stable with a constant of a few units per rotation
(m <= 5 rotations per column), the SVD behind lstsq likewise, and the condition of the least-squares problem is cond(H) + cond(H)^2 * |r| / (|H| |y|)
with cond(H) < 10 and |r| < |H| |y| here -- 64 covers the sum of the two sides with room, and is far below any real error (a wrong sign or a
rotation left out moves the result by O(1))."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps
TOL_MULTIPLE = 64.0
BETA = 1.75


def hessenberg(m, seed):
    """well-conditioned upper-Hessenberg (m + 1) x m: diagonal 3 +- 0.5, subdiagonal 1 +- 0.25, the rest below 0.5 in size"""
    rng = np.random.RandomState(seed)
    H = np.triu(rng.uniform(-0.5, 0.5, (m + 1, m)), 1)
    H[np.arange(m), np.arange(m)] = 3.0 + rng.uniform(-0.5, 0.5, m)
    H[np.arange(1, m + 1), np.arange(m)] = 1.0 + rng.uniform(-0.25, 0.25, m)
    return H


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("krylov_host") / ("krylov_host_" + request.param))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "femus_amd", "csrc"),
                                                                             os.path.join(ROOT, "tests", "krylov_host_main.cpp"), "-o", exe])
    return exe


def run(program, H, maxit=None, rtol=0.0, atol=0.0, dtol=1e5):
    m = H.shape[1]
    text = "%d %d %.17g %.17g %.17g %.17g\n" % (m, m if maxit is None else maxit, BETA, rtol, atol, dtol)
    text += "\n".join(" ".join("%.17g" % v for v in row) for row in H) + "\n"
    p = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr        # a sanitizer report ends the program with an error
    out = {"rn": []}
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "rn":
            assert int(w[1]) == len(out["rn"])
            out["rn"].append(float(w[2]))
        elif w[0] in ("done", "kused"):
            out[w[0]] = int(w[1])
        elif w[0] == "y":
            out["y"] = np.array([float(v) for v in w[1:]])
    return out


def lstsq(H, k):
    """min | BETA e_1 - H[:k + 1, :k] y |: solution and residual norm"""
    rhs = np.zeros(k + 1)
    rhs[0] = BETA
    y = np.linalg.lstsq(H[:k + 1, :k], rhs, rcond=None)[0]
    return y, np.linalg.norm(rhs - H[:k + 1, :k] @ y)


@pytest.mark.parametrize("m,seed", [(1, 1), (2, 2), (5, 3), (5, 4)])
def test_columns_one_at_a_time_match_lstsq(program, m, seed):
    """restart 1, 2 and 5: the residual estimate after every column is the least-squares residual of the leading block, the back substitution gives
    the least-squares solution, and done is reported where the iteration count runs out (the last column)"""
    H = hessenberg(m, seed)
    cond = np.linalg.cond(H)
    assert cond < 10
    tol = TOL_MULTIPLE * EPS * cond
    out = run(program, H)
    assert out["done"] == m - 1 and out["kused"] == m and len(out["rn"]) == m
    for k in range(m):
        _, r = lstsq(H, k + 1)
        print("m %d column %d: residual estimate %.17g, lstsq %.17g, distance %.2e (bound %.2e)" % (m, k, out["rn"][k], r, abs(out["rn"][k] - r), tol * BETA))
        assert abs(out["rn"][k] - r) <= tol * BETA
    y, _ = lstsq(H, m)
    print("m %d: |y - y_lstsq| / |y_lstsq| = %.2e (bound %.2e)" % (m, np.linalg.norm(out["y"] - y) / np.linalg.norm(y), tol))
    assert np.linalg.norm(out["y"] - y) <= tol * np.linalg.norm(y)


def test_stops_at_the_tolerance(program):
    """the convergence test: with rtol between two consecutive residual estimates, done is reported at the first column below it"""
    H = hessenberg(5, 3)
    rn = run(program, H)["rn"]
    assert rn[1] > rn[2]
    out = run(program, H, maxit=100, rtol=0.5 * (rn[1] + rn[2]) / BETA)
    assert out["done"] == 2 and out["kused"] == 3
    y, _ = lstsq(H, 3)
    assert np.linalg.norm(out["y"] - y) <= TOL_MULTIPLE * EPS * np.linalg.cond(H) * np.linalg.norm(y)


def test_vanished_column(program):
    """the d == 0 branch: column k vanishes entirely -- H[k][k] is set to 1, done is reported at k, the estimate is zero and y stays finite"""
    H = hessenberg(5, 5)
    H[:, 2] = 0.0
    out = run(program, H, maxit=100)
    assert out["done"] == 2 and out["kused"] == 3 and out["rn"][2] == 0.0
    assert np.isfinite(out["y"]).all() and len(out["y"]) == 3


def test_happy_breakdown(program):
    """h_{k+1,k} = 0 with a non-zero diagonal: the Krylov space is invariant, done is reported at k, the estimate is exactly zero and y solves the
    square leading system"""
    H = hessenberg(5, 6)
    H[3, 2] = 0.0
    cond = np.linalg.cond(H[:3, :3])
    assert cond < 10
    out = run(program, H, maxit=100)
    assert out["done"] == 2 and out["kused"] == 3 and out["rn"][2] == 0.0
    rhs = np.zeros(3)
    rhs[0] = BETA
    y = np.linalg.solve(H[:3, :3], rhs)
    assert np.linalg.norm(out["y"] - y) <= TOL_MULTIPLE * EPS * cond * np.linalg.norm(y)
