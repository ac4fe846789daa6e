"""The tracker's host math (csrc/tsdf_track_host.h) through the stand-alone track_solve_main: the
6 x 6 Cholesky solve, Rodrigues' formula and the pose update against numpy float64. No GPU, no
engine library."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "track_solve_main")


def run(lines):
    """One answer line per command line, split into words."""
    text = "".join(" ".join([ln[0]] + [repr(float(v)) for v in ln[1:]]) + "\n" for ln in lines)
    r = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def rodrigues(w):
    """exp([w]x) in closed form; the series of the two coefficients below 1e-3 rad."""
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    K = skew(w)
    if t < 1e-3:
        a, b = 1 - t * t / 6 + t ** 4 / 120, 0.5 - t * t / 24 + t ** 4 / 720
    else:
        a, b = np.sin(t) / t, (1 - np.cos(t)) / (t * t)
    return np.eye(3) + a * K + b * K @ K


def quat_to_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_known_spd_system():
    """A x = r with A = M M^T + I from a fixed M and a known x: the solver returns x."""
    rng = np.random.default_rng(7)
    M = rng.normal(size=(6, 6))
    A = M @ M.T + np.eye(6)
    x = np.array([0.5, -1.25, 2.0, 1e-3, -3.0, 0.75])
    r = A @ x
    ans, = run([["solve", *A[np.triu_indices(6)], *r]])
    assert ans[0] == "ok"
    got = np.array([float(v) for v in ans[1:]])
    assert got.shape == (6,)
    # the error of a backward-stable solve: cond(A) * eps, with a factor 100 of room
    assert np.abs(got - x).max() <= 100 * np.linalg.cond(A) * np.finfo(np.float64).eps * np.abs(x).max()
    assert np.abs(got - np.linalg.solve(A, r)).max() <= 1e-10


def test_singular_systems_are_reported():
    """Rank 5 (a zero pivot), an indefinite matrix, all zeros and a NaN entry: each is 'singular'."""
    rank5 = np.diag([4.0, 9.0, 1.0, 1.0, 16.0, 1.0])
    rank5[2, 3] = rank5[3, 2] = 1.0  # the block [[1, 1], [1, 1]]: its second pivot is 1 - 1 * 1 = 0 exactly
    indefinite = np.diag([1.0, 2.0, 3.0, -1.0, 1.0, 1.0])
    nan = np.eye(6)
    nan[2, 4] = np.nan
    r = np.ones(6)
    out = run([["solve", *A[np.triu_indices(6)], *r] for A in (rank5, indefinite, np.zeros((6, 6)), nan)])
    assert [o[0] for o in out] == ["singular"] * 4
    assert run([["solve", *np.eye(6)[np.triu_indices(6)], *r]])[0][0] == "ok"


def test_exp_matches_closed_form():
    """Near 0 (both sides of the series threshold), near pi / 2 and at exactly 0."""
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    thetas = [0.0, 1e-9, 9.9e-5, 1.01e-4, 1e-3, 0.3, np.pi / 2 - 1e-6, np.pi / 2, np.pi / 2 + 1e-6]
    out = run([["exp", *(th * axis)] for th in thetas])
    for th, o in zip(thetas, out):
        R = np.array([float(v) for v in o]).reshape(3, 3)
        assert np.abs(R - rodrigues(th * axis)).max() <= 1e-15 + 4e-16 * 4, th
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14
    R = np.array([float(v) for v in out[7]]).reshape(3, 3)  # pi / 2: R maps a vector normal to the axis onto axis x v
    v = np.cross(axis, [1.0, 0.0, 0.0])
    assert np.abs(R @ v - np.cross(axis, v)).max() <= 1e-15


def test_pose_update_matches_numpy():
    """R_wc <- exp([omega]x) R_wc, p_wc <- exp([omega]x) p_wc + t from a float pose, to 1e-12; the
    rounded float pose is the nearest float quaternion (w >= 0) and translation of the result."""
    rng = np.random.default_rng(9)
    lines, want = [], []
    for k in range(6):
        q = rng.normal(size=4).astype(np.float32)
        q /= np.float32(np.linalg.norm(q))
        t = rng.normal(size=3).astype(np.float32) * np.float32(3)
        xi = rng.normal(size=6) * [0.02, 0.02, 0.02, 0.05, 0.05, 0.05] * (10.0 if k == 5 else 1.0)
        R_cw = quat_to_R(q)
        R_wc, p_wc = R_cw.T, -R_cw.T @ t.astype(np.float64)
        E = rodrigues(xi[:3])
        want.append((E @ R_wc, E @ p_wc + xi[3:]))
        lines.append(["update", *q, *t, *xi])
    for (R, p), o in zip(want, run(lines)):
        v = np.array([float(x) for x in o])
        assert v.shape == (9 + 3 + 7,)
        assert np.abs(v[:9].reshape(3, 3) - R).max() <= 1e-12
        assert np.abs(v[9:12] - p).max() <= 1e-12
        q2, t2 = v[12:16], v[16:19]
        assert q2[3] >= 0 and abs(np.linalg.norm(q2) - 1) <= 4e-7
        assert np.abs(quat_to_R(q2) - R.T).max() <= 1e-6  # float rounding of a unit quaternion
        assert np.abs(t2 - (-R.T @ p)).max() <= 4e-7 * max(1.0, np.abs(p).max())
