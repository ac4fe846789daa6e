"""The view-gain contract from its numpy restatement alone (_view_ref.py): the worked example's figures, the
identity with the free layer's observe, what `seen` removes, the greedy loop's monotonicity, and the esdf helpers
against host/uv_dose.h (view_host_main). No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _free_ref as fref
import _view_ref as vr
from tsdf_amd import esdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "view_host_main")
f32 = np.float32
# the worked example: rows of 3 words with a 6-bit last word, ny and nz no multiples of 8
ORIGIN, DIMS, VOXEL, MARGIN = (-20, -10, -3), (70, 21, 40), 0.01, 0.03
K, W, H, FAR, STEP = (20.0, 20.0, 7.5, 5.5), 16, 12, 0.6, 0.005
IDENT = ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
AWAY = ((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0))
OUTSIDE = ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.2))
WORKED = dict(depth=0.265, visible=2035, gain=1100)


def worked_state():
    st = np.zeros(DIMS[::-1], np.uint8)
    st[:30, :, :20] = 1
    st[30:34] = 2
    return st


def test_worked_example():
    st = worked_state()
    assert vr.samples(FAR, STEP) == 120
    gain, pred, vis = vr.view_gain(st, ORIGIN, VOXEL, K, W, H, [IDENT], FAR, STEP, MARGIN, FAR)
    # every pixel hits at j = 53: z = 0.265 sits on a .5 voxel tie, which half-away rounding sends to z = 27
    assert (pred == f32(WORKED["depth"])).all() and f32(53) * f32(STEP) == f32(0.265)
    assert (f32(0.265) / f32(VOXEL)) == f32(26.5) and (f32(52) * f32(STEP)) / f32(VOXEL) < f32(26.5)
    assert int(vis.sum()) == WORKED["visible"] and int((vis[0] & (st == 0)).sum()) == WORKED["gain"] == gain[0]
    assert not vis[0][30:].any()  # nothing in or behind the wall
    # the same camera turned 180 degrees about y, no return for a miss: an all-zero image and gain 0
    gain, pred, vis = vr.view_gain(st, ORIGIN, VOXEL, K, W, H, [AWAY], FAR, STEP, MARGIN, 0.0)
    assert (pred == 0).all() and gain[0] == 0 and not vis.any()
    # with the optimistic sensor it sees free space out to far -- all of it outside the box but a sliver
    gain, pred, _ = vr.view_gain(st, ORIGIN, VOXEL, K, W, H, [AWAY], FAR, STEP, MARGIN, FAR)
    assert (pred == f32(FAR)).all() and gain[0] == 4


def test_free_observe_identity_and_seen():
    """gain == the new bits on state-0 voxels of _free_ref.observe(pred) with max_depth 2 far; `seen` removes
    exactly the voxels it covers."""
    st = worked_state()
    views = [IDENT, OUTSIDE, AWAY]
    gain, pred, vis = vr.view_gain(st, ORIGIN, VOXEL, K, W, H, views, FAR, STEP, MARGIN, FAR)
    rng = np.random.default_rng(9)
    seen = rng.random(st.shape) < 0.4
    g2, p2, _ = vr.view_gain(st, ORIGIN, VOXEL, K, W, H, views, FAR, STEP, MARGIN, FAR, seen)
    assert np.array_equal(p2.view(np.uint32), pred.view(np.uint32))
    for i, (q, t) in enumerate(views):
        for before, want in ((np.zeros(st.shape, bool), gain[i]), (seen, g2[i])):
            layer = dict(bits=fref.pack(before), origin=ORIGIN, dims=DIMS)
            m = fref.observe(layer, fref.frame(pred[i], K, q, t, f32(2) * f32(FAR)), VOXEL, MARGIN)
            assert np.array_equal(m, vis[i])  # d <= 2 far holds for every predicted depth
            new = fref.unpack(layer["bits"], DIMS[0]) & ~before
            assert int((new & (st == 0)).sum()) == want
        assert g2[i] == gain[i] - int((vis[i] & (st == 0) & seen).sum())
    assert (g2[:2] < gain[:2]).all() and (gain[:2] > 0).all()


def test_greedy_is_monotone():
    st = worked_state()
    rng = np.random.default_rng(1)
    views = [IDENT, OUTSIDE, AWAY]
    for _ in range(5):
        q = rng.normal(size=4) * np.array([0.2, 0.2, 0.2, 1.0])
        q = (q / np.linalg.norm(q)).astype(f32)
        views.append((tuple(float(c) for c in q), tuple(float(c) for c in rng.uniform(-0.05, 0.05, 3).astype(f32))))
    chosen, gains, seen = vr.next_views(st, ORIGIN, VOXEL, MARGIN, K, W, H, views, 6, FAR, STEP, FAR)
    assert len(chosen) >= 3 and len(set(chosen)) == len(chosen)
    assert gains == sorted(gains, reverse=True) and gains[-1] > 0
    assert sum(gains) == int((seen & (st == 0)).sum())
    first = vr.view_gain(st, ORIGIN, VOXEL, K, W, H, views, FAR, STEP, MARGIN, FAR)[0]
    assert chosen[0] == int(np.argmax(first)) and gains[0] == int(first.max())
    # a round against everything already seen offers nothing
    assert not vr.view_gain(st, ORIGIN, VOXEL, K, W, H, [views[i] for i in chosen], FAR, STEP, MARGIN, FAR, seen)[0].any()


def test_binding_declares_view_gain():
    import tsdf_amd
    from tsdf_amd import _lib
    L = tsdf_amd.load_library()
    for name in ("tsdf_view_config_default", "tsdf_view_gain"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert C.sizeof(_lib.ViewConfig) == 64 and _lib.ViewConfig.K.offset == 32 and _lib.ViewConfig.far.offset == 48
    assert callable(tsdf_amd.Engine.view_gain) and tsdf_amd.VIEW_BATCH == 64
    text = open(os.path.join(ROOT, "include", "disinfect_tsdf.h")).read()
    assert re.search(r"#define TSDF_VIEW_BATCH 64\b", text)
    decl = re.search(r"int tsdf_view_gain\((.*?)\);", text, re.S).group(1)
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert len(params) == len(L.tsdf_view_gain.argtypes)
    for p, a in zip(params, L.tsdf_view_gain.argtypes):
        if "*" in p:
            assert a is C.c_void_p or issubclass(a, C._Pointer), p
        elif p.startswith("int32_t"):
            assert a is C.c_int32, p
        else:
            assert p.startswith("int ") and a is C.c_int, p
    assert L.tsdf_view_gain.restype is C.c_int
    # invalid arguments are refused before any device work; the defaults without an engine
    g = C.c_int64(7)
    assert L.tsdf_view_gain(None, None, None, None, None, 1, C.byref(g), None, 0) == 1 and g.value == 7
    c = _lib.ViewConfig(width=5, far=9.0)
    L.tsdf_view_config_default(None, C.byref(c))
    assert (c.width, c.far, c.miss_depth, c.step, c.margin) == (0, 3.0, 3.0, 0.0, 0.0)


def poses_of(line):
    return np.array([float(v) for v in line.split()], np.float32)


def test_esdf_helpers_match_host_header():
    rng = np.random.default_rng(4)
    cases = [((1, 2, 3), (2, 2, 3), (0, 0, 1)), ((0, 0, 0), (0, 0, 1), (0, 0, 1)), ((0, 0, 0), (0, 0, -2), (0, 0, 1)),
             ((0.5, 0, 0), (3, 0, 0), (1, 0, 0)), ((0, 0, 0), (-1, 1e-12, 0), (0, 0, 1)), ((0, 0, 0), (0, -1, 0), (0, 0, 1))]
    cases += [tuple(tuple(float(v) for v in rng.uniform(-2, 2, 3)) for _ in range(3)) for _ in range(40)]
    lines = [f"look_at {' '.join(repr(float(v)) for v in e + t + u)}" for e, t, u in cases]
    # a frontier result by hand: three clusters with goals across the box
    dims, origin, voxel = (12, 9, 7), (10, -5, 2), np.float32(0.02)
    tab = np.zeros(3, esdf_dtype())
    tab["goal"], tab["size"], tab["label"] = [0, 517, 12 * 9 * 7 - 1], [3, 4, 5], [0, 100, 200]
    res = dict(clusters=tab, origin=origin, dims=dims)
    yaws, pitch = 5, 0.25
    lines.append(f"candidates {dims[0]} {dims[1]} {dims[2]} {origin[0]} {origin[1]} {origin[2]} {float(voxel)!r} {yaws} {pitch} 3 " +
                 " ".join(f"{c['label']} {c['size']} 0 0 0 {c['goal']} {c['goal_key']}" for c in tab))
    lines += ["look_at 1 1 1 1 1 1 0 0 1", "nonsense"]
    r = subprocess.run([BIN], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines) and out[-1].startswith("error") and out[-2].startswith("error")
    for (e, t, u), line in zip(cases, out):
        p = esdf.look_at(e, t, u)
        assert p.q.dtype == np.float32 and np.array_equal(poses_of(line), np.concatenate([p.q, p.t])), (e, t, u)
        # z forward, the eye at the camera centre, the rotation a rotation
        d = np.array(t, np.float64) - np.array(e, np.float64)
        fwd = p.Apply(np.asarray(t, f32)).astype(np.float64)
        assert np.allclose(fwd, [0, 0, np.linalg.norm(d)], atol=1e-5) and np.allclose(p.Apply(np.asarray(e, f32)), 0, atol=1e-5)
        assert abs(float((p.q.astype(np.float64) ** 2).sum()) - 1) < 1e-6 and p.q[3] >= 0
    # up is up: with the default up, a point above the eye projects to negative y (y is down), x stays 0
    p = esdf.look_at((1, 2, 3), (2, 2, 3))
    assert np.allclose(p.Apply(np.array([1, 2, 4], f32)), [0, -1, 0], atol=1e-6)
    assert np.allclose(p.Apply(np.array([1, 1, 3], f32)), [1, 0, 0], atol=1e-6)  # world -y is to the right
    try:
        esdf.look_at((1, 1, 1), (1, 1, 1))
        assert False
    except ValueError:
        pass
    views, owner = esdf.view_candidates(res, voxel, yaws=yaws, pitch=pitch)
    got = poses_of(out[len(cases)]).reshape(-1, 8)
    assert len(views) == 3 * yaws == got.shape[0] and owner.dtype == np.int32
    assert np.array_equal(got[:, 0], owner) and owner.tolist() == sorted(owner.tolist())
    want = np.array([np.concatenate([v.q, v.t]) for v in views], np.float32)
    assert np.array_equal(got[:, 1:], want)
    goal = esdf.frontier_goals(res, voxel)["goal"]
    for v, c in zip(views, owner):
        assert np.allclose(v.Inverse().Apply(np.zeros(3, f32)), goal[c], atol=1e-5)  # the camera stands at the goal
        up = v.Inverse().Apply(np.array([0, 0, 1], f32)) - goal[c]                  # its optical axis, in the world
        assert abs(float(up[2]) - np.sin(pitch)) < 1e-5


def esdf_dtype():
    import tsdf_amd
    return tsdf_amd.COMPONENT_DTYPE
