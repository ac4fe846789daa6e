"""The travel field's restatement (tests/_travel_ref.py): Dijkstra against the vectorised relaxation, the
figures the GPU tests rely on, the walk-back rule, the tsdf_amd.esdf helpers against brute force, the
binding's declarations and the C++ helpers of host/uv_dose.h (travel_host_main). No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _edt_ref
import _travel_ref as tr
from tsdf_amd import esdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "travel_host_main")
SHAPES = [(7, 9, 12), (1, 1, 1), (5, 1, 8), (1, 9, 1), (9, 17, 20), (16, 16, 24)]
ORIGIN, DIMS, SEED = (-37, -35, -21), (77, 70, 59), (-20, -20, -5)
# clearance2, unknown_free -> passable = reached voxels, largest cost
SCENE = {(0, 0): (19100, 222), (4, 0): (14428, 225), (9, 0): (9644, 229), (0, 1): (300602, 273)}


def random_case(rng, shape, density, nseeds=3):
    ok = rng.random(shape) < density
    nz, ny, nx = shape
    seeds = np.stack([rng.integers(-1, nx + 1, nseeds), rng.integers(-1, ny + 1, nseeds),
                      rng.integers(-1, nz + 1, nseeds)], -1)
    free = np.argwhere(ok)
    if free.shape[0]:
        seeds = np.concatenate([seeds, free[rng.integers(0, free.shape[0], 2)][:, ::-1]])
    return ok, seeds


def test_dijkstra_is_the_relaxations_fixed_point():
    rng = np.random.default_rng(3)
    for shape in SHAPES:
        for density in (0.35, 0.6, 0.9):
            ok, seeds = random_case(rng, shape, density)
            a, sa = tr.field(ok, seeds)
            b, sb, _ = tr.sweep(ok, seeds)
            assert a.dtype == np.uint32 and np.array_equal(a, b) and sa == sb, (shape, density)
            assert (a[~ok] == tr.UNREACHED).all()
            assert sa == sum(1 for x, y, z in seeds.tolist()
                             if 0 <= x < shape[2] and 0 <= y < shape[1] and 0 <= z < shape[0] and ok[z, y, x])
    # no seed, and a single free voxel
    a, s = tr.field(np.ones((3, 4, 5), bool), np.zeros((0, 3), int))
    assert s == 0 and (a == tr.UNREACHED).all()
    a, s = tr.field(np.ones((1, 1, 1), bool), [(0, 0, 0), (0, 0, 0)])
    assert s == 2 and a.tolist() == [[[0]]]
    # an open box: the chamfer distance in closed form
    a, _ = tr.field(np.ones((6, 7, 8), bool), [(0, 0, 0)])
    z, y, x = np.meshgrid(np.arange(6), np.arange(7), np.arange(8), indexing="ij")
    d = np.sort(np.stack([x, y, z], -1), axis=-1)
    assert np.array_equal(a, 5 * d[..., 0] + 4 * (d[..., 1] - d[..., 0]) + 3 * (d[..., 2] - d[..., 1]))


def test_passable():
    d2 = np.array([0, 3, 4, 4, 9, 65025], np.uint16)
    st = np.array([1, 1, 1, 0, 2, 0], np.uint8)
    assert tr.passable(d2, st).tolist() == [True, True, True, False, False, False]
    assert tr.passable(d2, st, 4).tolist() == [False, False, True, False, False, False]
    assert tr.passable(d2, st, 4, True).tolist() == [False, False, True, True, False, True]
    assert tr.passable(d2, st, 65025, True).tolist() == [False] * 5 + [True]
    ok = np.random.default_rng(0).random((3, 4, 5)) < 0.5
    assert np.array_equal(tr.passable(*tr.arrays(ok)), ok)


def test_serpentine_figures():
    ok = tr.serpentine(40, 24, 20, pitch=4, gap=2)
    assert int(ok.sum()) == 14800
    a, s = tr.field(ok, [(0, 0, 0)])
    b, _, passes = tr.sweep(ok, [(0, 0, 0)])
    assert np.array_equal(a, b) and s == 1
    assert int((a != tr.UNREACHED).sum()) == 14800
    assert int(a[a != tr.UNREACHED].max()) == 694 and passes == 213


@pytest.fixture(scope="module")
def scene():
    dump = _edt_ref.records_dump(_edt_ref.scene_records())
    return _edt_ref.distance_field(dump, ORIGIN, DIMS)


@pytest.mark.parametrize("clearance2,unknown_free", sorted(SCENE))
def test_scene_figures(scene, clearance2, unknown_free):
    """The figures tests/test_gpu_travel.py relies on, from the restatement alone."""
    ok = tr.passable(scene["d2"], scene["state"], clearance2, bool(unknown_free))
    seed = np.array(SEED) - np.array(ORIGIN)
    a, s = tr.field(ok, [seed])
    reached = a != tr.UNREACHED
    assert s == 1
    assert (int(ok.sum()), int(reached.sum()), int(a[reached].max())) == (SCENE[clearance2, unknown_free][0],) * 2 + \
        (SCENE[clearance2, unknown_free][1],)
    if not unknown_free:
        assert np.array_equal(a, tr.sweep(ok, [seed])[0])


def check_paths(cost, targets, ps, lens):
    nz, ny, nx = cost.shape
    flat = cost.ravel().astype(np.int64)
    for (x, y, z), p, n in zip(targets, ps, lens):
        inside = 0 <= x < nx and 0 <= y < ny and 0 <= z < nz
        if not inside or cost[z, y, x] == tr.UNREACHED:
            assert n == 0 and p.size == 0
            continue
        assert n == p.size > 0 and p[0] == (z * ny + y) * nx + x and flat[p[-1]] == 0
        c = flat[p]
        v = np.stack([p % nx, p // nx % ny, p // (nx * ny)], -1).astype(np.int64)
        step = np.abs(np.diff(v, axis=0))
        assert (step.max(axis=1) == 1).all() if n > 1 else True
        assert np.array_equal(c[:-1] - c[1:], 2 + step.sum(axis=1))
        assert n - 1 <= c[0] // 3 and 5 * (n - 1) >= c[0]


def test_paths():
    rng = np.random.default_rng(5)
    for shape in [(7, 9, 12), (1, 9, 1), (9, 17, 20)]:
        ok, seeds = random_case(rng, shape, 0.7)
        cost, _ = tr.field(ok, seeds)
        nz, ny, nx = shape
        targets = np.stack([rng.integers(-1, nx + 1, 40), rng.integers(-1, ny + 1, 40), rng.integers(-1, nz + 1, 40)], -1)
        ps, lens = tr.paths(cost, targets)
        check_paths(cost, targets.tolist(), ps, lens)
        assert sum(1 for n in lens if n > 1) > 3 or shape == (1, 9, 1)
        # truncation keeps the full length
        qs, qlens = tr.paths(cost, targets, max_len=2)
        assert qlens == lens and all(np.array_equal(q, p[:2]) for q, p in zip(qs, ps))
    ok = tr.serpentine(40, 24, 20, pitch=4, gap=2)
    cost, _ = tr.field(ok, [(0, 0, 0)])
    far = np.argwhere(cost == 694)[0][::-1]
    ps, lens = tr.paths(cost, [far])
    check_paths(cost, [far.tolist()], ps, lens)
    assert lens[0] > 200
    # a field with a voxel that has no predecessor: the walk stops, the count negated
    bad = cost.copy()
    bad[cost < cost.ravel()[ps[0][4]]] = tr.UNREACHED  # (nothing cheaper than the walk's fifth voxel is left)
    qs, lens = tr.paths(bad, [far])
    assert lens == [-5] and np.array_equal(qs[0], ps[0][:5])


def test_pocket_is_unreached():
    ok = np.ones((12, 12, 12), bool)
    ok[3:9, 3:9, 3:9] = False
    ok[4:8, 4:8, 4:8] = True  # a pocket behind a one-voxel wall
    cost, s = tr.field(ok, [(0, 0, 0)])
    assert s == 1 and (cost[4:8, 4:8, 4:8] == tr.UNREACHED).all() and (cost[~ok] == tr.UNREACHED).all()
    outside = ok.copy()
    outside[4:8, 4:8, 4:8] = False
    assert (cost[outside] != tr.UNREACHED).all()
    # seeded inside, the pocket is all that is reached
    cost, _ = tr.field(ok, [(5, 5, 5)])
    assert int((cost != tr.UNREACHED).sum()) == 64 and (cost[outside] == tr.UNREACHED).all()
    # a diagonal step slips between two obstacles that touch at an edge: the contract's rule, stated
    ok = np.ones((1, 2, 2), bool)
    ok[0, 0, 1] = ok[0, 1, 0] = False
    assert tr.field(ok, [(0, 0, 0)])[0][0, 1, 1] == 4


def travel(cost, origin):
    cost = np.asarray(cost, np.uint32)
    return dict(cost=cost, origin=origin, dims=cost.shape[::-1], seeded=1, rounds=1)


def test_esdf_helpers():
    rng = np.random.default_rng(9)
    cost = rng.integers(0, 400, (4, 5, 6)).astype(np.uint32)
    cost[rng.random(cost.shape) < 0.3] = tr.UNREACHED
    t = travel(cost, (10, -5, 2))
    voxel = np.float32(0.02)
    m = esdf.travel_metres(t, voxel)
    assert m.dtype == np.float32 and m.shape == cost.shape
    for i in np.ndindex(cost.shape):
        want = np.inf if cost[i] == tr.UNREACHED else np.float32(np.float32(cost[i]) / np.float32(3)) * voxel
        assert m[i] == want
    pos = ((rng.integers(-2, 8, (60, 3)) + np.array([10, -5, 2])) * 0.02).astype(np.float32)
    for max_travel in (None, 1.5):
        mask, dist = esdf.reachable(t, voxel, pos, max_travel)
        assert mask.dtype == bool and dist.dtype == np.float32
        for k, v in enumerate(esdf.voxel_of(pos, voxel).tolist()):
            l = [v[0] - 10, v[1] + 5, v[2] - 2]
            inside = all(0 <= l[a] < (6, 5, 4)[a] for a in range(3))
            c = cost[l[2], l[1], l[0]] if inside else tr.UNREACHED
            want = np.inf if c == tr.UNREACHED else np.float32(np.float32(c) / np.float32(3)) * voxel
            assert dist[k] == want
            assert mask[k] == (c != tr.UNREACHED and (max_travel is None or want <= np.float32(max_travel)))
        assert mask.any() and not mask.all()
    # path_points: seed first, voxel v at v * voxel
    path = np.array([(3 * 5 + 4) * 6 + 5, (2 * 5 + 3) * 6 + 4, 0], np.int32)
    pts = esdf.path_points(t, voxel, path)
    assert pts.dtype == np.float32
    want = (np.array([[10, -5, 2], [14, -2, 4], [15, -1, 5]]).astype(np.float32) * voxel).astype(np.float32)
    assert np.array_equal(pts, want)
    assert esdf.path_points(t, voxel, np.zeros(0, np.int32)).shape == (0, 3)


def test_binding_declares_travel():
    import tsdf_amd
    from tsdf_amd import _lib
    L = tsdf_amd.load_library()
    for name in ("tsdf_travel_config_default", "tsdf_travel_field", "tsdf_travel_paths"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert C.sizeof(_lib.TravelConfig) == 20 and _lib.TSDF_TRAVEL_UNREACHED == tr.UNREACHED
    assert callable(tsdf_amd.Engine.travel_field) and callable(tsdf_amd.Engine.travel_paths)
    c = _lib.TravelConfig(dims=(C.c_int32 * 3)(7, 7, 7), clearance2=5, unknown_free=1)
    L.tsdf_travel_config_default(C.byref(c))
    assert list(c.dims) == [0, 0, 0] and (c.clearance2, c.unknown_free) == (0, 0)
    # the header's argument lists, parameter for parameter
    text = open(os.path.join(ROOT, "include", "disinfect_tsdf.h")).read()
    kinds = {"tsdf_travel_field": L.tsdf_travel_field, "tsdf_travel_paths": L.tsdf_travel_paths}
    for name, fn in kinds.items():
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        assert len(params) == len(fn.argtypes), name
        for p, a in zip(params, fn.argtypes):
            if "*" in p or "[" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            elif p.startswith("int32_t"):
                assert a is C.c_int32, (name, p)
            else:
                assert p.startswith("int ") and a is C.c_int, (name, p)
        assert fn.restype is C.c_int
    # invalid arguments are refused before any device work
    one = C.c_int32(7)
    assert L.tsdf_travel_field(None, None, None, None, None, 0, None, 0, C.byref(one), None) == 1 and one.value == 7
    assert L.tsdf_travel_paths(None, None, None, 0, None, 0, 0, None, None) == 1


def _run(lines):
    r = subprocess.run([BIN], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [ln.split() for ln in out]


def test_host_header_matches_numpy():
    rng = np.random.default_rng(12)
    num = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))
    ints = lambda a: " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))
    voxel = np.float32(0.02)
    coords = np.concatenate([(rng.standard_normal(40) * 0.3).astype(np.float32),
                             np.array([0.01, -0.01, 0.03, -0.03, 0.0099, 0.0, 0.05, -0.05], np.float32)])
    cost = rng.integers(0, 500, (4, 5, 6)).astype(np.uint32)
    cost[rng.random(cost.shape) < 0.3] = tr.UNREACHED
    t = travel(cost, (10, -5, 2))
    pos = ((rng.integers([-1, -1, -1], [7, 6, 5], (120, 3)) + np.array([10, -5, 2])) * 0.02 +
           rng.uniform(-0.004, 0.004, (120, 3))).astype(np.float32)
    out = _run([
        f"voxel {coords.size} {float(voxel)!r} 0.0 {num(coords)}",
        f"voxel {coords.size} {float(voxel)!r} 0.5 {num(coords)}",
        f"metres {cost.size} {float(voxel)!r} {ints(cost)}",
        f"reachable 6 5 4 10 -5 2 {float(voxel)!r} inf 0.0 120 {num(pos)} {ints(cost)}",
        f"reachable 6 5 4 10 -5 2 {float(voxel)!r} 1.5 0.5 120 {num(pos)} {ints(cost)}",
        "reachable 6 5 4 10 -5 2 0.02 inf 0.0 1 0.0 0.0 0.0 1 2 3",
    ])
    for row, off in ((out[0], 0.0), (out[1], 0.5)):
        want = esdf.voxel_of(np.stack([coords] * 3, -1), voxel, off)[:, 0]
        assert [int(v) for v in row] == want.tolist()
    assert np.array_equal(np.array([float(v) for v in out[2]], np.float32), esdf.travel_metres(t, voxel).ravel())
    for row, max_travel, off in ((out[3], None, 0.0), (out[4], 1.5, 0.5)):
        mask, dist = esdf.reachable(t, voxel, pos, max_travel, off)
        got = np.array([float(v) for v in row], np.float32).reshape(-1, 4)
        assert mask.sum() > 3 and np.array_equal(got[:, :3], pos[mask]) and np.array_equal(got[:, 3], dist[mask])
    assert out[5][0] == "error"
