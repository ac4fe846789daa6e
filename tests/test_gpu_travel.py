"""The travel field (tsdf_travel_field, tsdf_travel_paths) against tests/_travel_ref.py, the Python restatement
of the contract, byte for byte: on synthetic d2 / state arrays of many shapes, host and device memory, a maze
that needs more rounds than one host batch, scratch growth, refused arguments, an engine with pending frames,
a shard engine, the distance field of the analytic floor-and-box scene, and through the facade (travel_main).
Every expected value is an integer. The scene's figures were evaluated on the CPU (tests/test_travel_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _edt_ref
import _travel_ref as tr
from _edt_ref import NB_BITS, TRUNC, VOXEL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "travel_main")
SHAPES = [(7, 9, 12), (1, 1, 1), (5, 1, 8), (1, 9, 1), (9, 17, 20), (16, 16, 24), (9, 10, 21)]
ORIGIN, DIMS, SEED = (-37, -35, -21), (77, 70, 59), (-20, -20, -5)
SCENE = {(0, 0): (19100, 222), (4, 0): (14428, 225), (9, 0): (9644, 229), (0, 1): (300602, 273)}
BOX = (5, -11, 3)  # the synthetic fields' origin: seeds and targets are global voxels
TSDF_ERR_INVALID_ARG = 1
BATCH = 32  # kTravelBatch (tsdf_host_travel.hip): rounds between two reads of the control words


def make_engine(**kw):
    import tsdf_amd
    return tsdf_amd.Engine(VOXEL, TRUNC, max_width=64, max_height=64, num_block_bits=NB_BITS, **kw)


@pytest.fixture(scope="module")
def eng():
    # torch's HIP runtime first (conftest._torch_hip_first runs after module fixtures)
    import torch
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    e = make_engine()
    yield e
    e.close()


def dfield(d2, state, origin=BOX):
    d2, state = np.ascontiguousarray(d2, np.uint16), np.ascontiguousarray(state, np.uint8)
    return dict(d2=d2, state=state, origin=tuple(origin), dims=d2.shape[::-1], max_dist=255, unknown=False)


def glob(v, origin=BOX):
    return np.asarray(v, np.int64).reshape(-1, 3) + np.asarray(origin, np.int64)


def host(t):
    return dict(t, cost=t["cost"].cpu().numpy()) if hasattr(t["cost"], "is_cuda") else t


def check(eng, d2, state, seeds, clearance2=0, unknown_free=False, tag="", kinds=(False, True)):
    """Both memory kinds against Dijkstra on the restatement's passable(); returns the reference and a result."""
    ok = tr.passable(d2, state, clearance2, unknown_free)
    want, nseeded = tr.field(ok, seeds)
    got = None
    for device in kinds:
        got = eng.travel_field(dfield(d2, state), glob(seeds), clearance2, unknown_free, device=device)
        cost = host(got)["cost"]
        assert cost.dtype == np.uint32 and cost.shape == d2.shape and got["dims"] == d2.shape[::-1] and got["origin"] == BOX
        print(f"{tag} device={device}: differs at {int((cost != want).sum())} of {want.size}, reached "
              f"{int((want != tr.UNREACHED).sum())}, seeded {got['seeded']}, rounds {got['rounds']}")
        assert got["seeded"] == nseeded
        assert np.array_equal(cost, want)
    return want, got


def random_case(rng, shape, density, nseeds=3):
    ok = rng.random(shape) < density
    nz, ny, nx = shape
    seeds = np.stack([rng.integers(-1, nx + 1, nseeds), rng.integers(-1, ny + 1, nseeds),
                      rng.integers(-1, nz + 1, nseeds)], -1)
    free = np.argwhere(ok)
    if free.shape[0]:
        seeds = np.concatenate([seeds, free[rng.integers(0, free.shape[0], 2)][:, ::-1]])
    return ok, seeds


@pytest.mark.parametrize("density", [0.35, 0.6, 0.9])
def test_shapes(eng, density):
    """Dims of 1, dims that are no multiple of the tile, one tile and several."""
    rng = np.random.default_rng(int(density * 100))
    reached = 0
    for shape in SHAPES:
        ok, seeds = random_case(rng, shape, density)
        want, _ = check(eng, *tr.arrays(ok), seeds, tag=f"shape {shape} density {density}")
        reached += int((want != tr.UNREACHED).sum())
    assert reached > 1000
    assert eng.stats()["status"] == 0


def test_seeds(eng):
    """Seeds outside the box, impassable and duplicate ones; none at all; none usable."""
    ok = np.random.default_rng(1).random((9, 10, 21)) < 0.8
    ok[4, 5, 6], ok[0, 0, 0], ok[8, 9, 20] = True, False, True
    d2, st = tr.arrays(ok)
    seeds = [(6, 5, 4), (6, 5, 4), (0, 0, 0), (-1, 5, 4), (21, 0, 0), (3, 10, 2), (3, 3, 9), (20, 9, 8), (6, 5, 4),
             (2 ** 31 - 30, 0, 0), (0, -2 ** 31 + 30, 0)]
    want, got = check(eng, d2, st, seeds, tag="seeds")
    assert got["seeded"] == 4 and want[4, 5, 6] == 0 and want[8, 9, 20] == 0
    for s in (np.zeros((0, 3), int), [(0, 0, 0), (-5, 2, 2)]):
        want, got = check(eng, d2, st, s, tag="no seed")
        assert got["seeded"] == 0 and got["rounds"] == 0 and (want == tr.UNREACHED).all()


def test_border_seeds(eng):
    """A seed on a tile's border that is the only link into the neighbouring tile: no round lowers a seed, so
    the seed pass itself has to list the tiles it faces. One-voxel corridors along each axis seeded at local
    7 and at local 8, alone and inside a wider box; and a seed whose only passable neighbour lies across a
    tile face, edge or corner, for every direction."""
    for axis in range(3):
        for at in (7, 8, 0, 15, 16, 23):
            shape = [1, 1, 1]
            shape[2 - axis] = 24
            seed = [0, 0, 0]
            seed[axis] = at
            want, got = check(eng, *tr.arrays(np.ones(shape, bool)), [seed], tag=f"corridor axis {axis} seed {at}")
            assert want.max() == 3 * max(at, 23 - at) and (want != tr.UNREACHED).all()
            wide = [5, 5, 5]
            wide[2 - axis] = 24
            ok = np.zeros(wide, bool)
            line = [2, 2, 2]
            line[2 - axis] = slice(None)
            ok[tuple(line)] = True
            seed = [2, 2, 2]
            seed[axis] = at
            want, _ = check(eng, *tr.arrays(ok), [seed], tag=f"corridor in a box, axis {axis} seed {at}")
            assert int((want != tr.UNREACHED).sum()) == 24
    # two passable voxels, one a seed, a step apart across the tile border at 7 | 8
    n = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                d = (dx, dy, dz)
                if d == (0, 0, 0):
                    continue
                seed = [7 if v > 0 else (8 if v < 0 else 3) for v in d]
                other = [s + v for s, v in zip(seed, d)]
                ok = np.zeros((16, 16, 16), bool)
                ok[seed[2], seed[1], seed[0]] = ok[other[2], other[1], other[0]] = True
                want, _ = check(eng, *tr.arrays(ok), [seed], tag=f"seed {seed} -> {other}")
                assert want[other[2], other[1], other[0]] == 2 + sum(abs(v) for v in d)
                n += 1
    assert n == 26
    assert eng.stats()["status"] == 0


def test_state_and_clearance(eng):
    """unknown_free 0 and 1 on mixed states; clearance2 at 0, in the middle and above every d2."""
    rng = np.random.default_rng(2)
    shape = (9, 17, 20)
    st = rng.choice(np.array([0, 1, 2], np.uint8), shape, p=[0.4, 0.45, 0.15])
    d2 = rng.integers(0, 40, shape).astype(np.uint16)
    seeds = np.argwhere(st == 1)[:3, ::-1]
    counts = {}
    for unknown_free in (False, True):
        for c2 in (0, 9, 40):
            want, _ = check(eng, d2, st, seeds, c2, unknown_free, tag=f"unknown_free={unknown_free} clearance2={c2}")
            counts[unknown_free, c2] = int((want != tr.UNREACHED).sum())
    assert counts[False, 40] == 0 and counts[True, 40] == 0
    assert 0 < counts[False, 9] < counts[False, 0] < counts[True, 0] and counts[False, 9] < counts[True, 9]
    # the largest clearance: only d2 65025 passes
    d2[:] = 65025
    want, _ = check(eng, d2, st, seeds, 65025, True, tag="clearance2=65025", kinds=(False,))
    assert (want[st != 2] != tr.UNREACHED).sum() > 2000


@pytest.fixture(scope="module")
def maze():
    """64 x 64 x 8, a wall across every odd x with a one-voxel gap at alternating ends of y: the path from
    x = 0 runs the length of y 32 times and crosses more than 200 tile faces."""
    ok = tr.serpentine(64, 64, 8, pitch=2, gap=1)
    want, _ = tr.field(ok, [(0, 0, 0)])
    assert int((want != tr.UNREACHED).sum()) == int(ok.sum()) == 64 * 8 * 32 + 32 * 8
    return ok, want


def test_more_rounds_than_a_batch(eng, maze):
    """Where a lost wake-up or a wrong stop test shows: the rounds go on past the first read of the counter."""
    ok, want = maze
    for device in (False, True):
        got = eng.travel_field(dfield(*tr.arrays(ok)), glob([(0, 0, 0)]), device=device)
        cost = host(got)["cost"]
        print(f"maze device={device}: rounds {got['rounds']}, differs at {int((cost != want).sum())}, "
              f"largest cost {int(want[want != tr.UNREACHED].max())}")
        assert got["rounds"] > 2 * BATCH and got["seeded"] == 1
        assert np.array_equal(cost, want)
    # seeded at both ends: about half the rounds, the same contract
    ends = [(0, 0, 0), (62, 0, 7)]
    want2, got = check(eng, *tr.arrays(ok), ends, tag="maze, two seeds")
    assert BATCH < got["rounds"] < 0.75 * eng.travel_field(dfield(*tr.arrays(ok)), glob([(0, 0, 0)]))["rounds"]


def test_repeat_and_scratch_growth(maze):
    ok, want = maze
    rng = np.random.default_rng(4)
    small_ok, small_seeds = random_case(rng, (7, 9, 12), 0.8)
    small = dfield(*tr.arrays(small_ok))
    e = make_engine()  # (a fresh engine: its scratch starts empty)
    try:
        a = e.travel_field(small, glob(small_seeds))
        b = e.travel_field(small, glob(small_seeds))
        big = e.travel_field(dfield(*tr.arrays(ok)), glob([(0, 0, 0)]))
        c = e.travel_field(small, glob(small_seeds))
        d = e.travel_field(small, glob(small_seeds), device=True)
        assert np.array_equal(big["cost"], want)
        assert np.array_equal(a["cost"], tr.field(small_ok, small_seeds)[0])
        for other in (b, c, host(d)):
            assert np.array_equal(a["cost"], other["cost"]) and (a["seeded"], a["rounds"]) == (other["seeded"], other["rounds"])
        assert e.stats()["status"] == 0
    finally:
        e.close()


def test_arguments(eng):
    import tsdf_amd
    lib = tsdf_amd._lib
    L = lib.load()
    c = lib.TravelConfig()
    c.clearance2 = 7
    L.tsdf_travel_config_default(C.byref(c))
    assert (c.clearance2, c.unknown_free) == (0, 0) and list(c.dims) == [0, 0, 0]
    d2, st = np.full(27, 9, np.uint16), np.ones(27, np.uint8)
    seeds = np.array([1, 1, 1], np.int32)

    def call(h=0, dims=(3, 3, 3), clearance2=0, unknown_free=0, d2p=True, stp=True, costp=True, S=1, seedp=True,
             kind=0, cfg=True):
        c = lib.TravelConfig((C.c_int32 * 3)(*dims), clearance2, unknown_free)
        cost = np.full(27, 0xABCD1234, np.uint32)
        seeded, rounds = C.c_int32(-7), C.c_int32(-7)
        rc = L.tsdf_travel_field(eng._h if h == 0 else h, C.byref(c) if cfg else None, d2.ctypes.data if d2p else None,
                                 st.ctypes.data if stp else None, seeds.ctypes.data if seedp else None, S,
                                 cost.ctypes.data if costp else None, kind, C.byref(seeded), C.byref(rounds))
        return rc, bool((cost == 0xABCD1234).all()) and (seeded.value, rounds.value) == (-7, -7)

    assert call() == (0, False)
    assert call(S=0, seedp=False)[0] == 0
    bad = [dict(dims=(0, 3, 3)), dict(dims=(3, 2049, 3)), dict(dims=(3, 3, -1)), dict(dims=(2048, 2048, 65)),
           dict(clearance2=-1), dict(clearance2=65026), dict(unknown_free=2), dict(unknown_free=-1), dict(d2p=False),
           dict(stp=False), dict(costp=False), dict(S=-1), dict(S=1, seedp=False), dict(kind=2), dict(kind=-1),
           dict(cfg=False), dict(h=None)]
    for kw in bad:
        assert call(**kw) == (TSDF_ERR_INVALID_ARG, True), kw
    with pytest.raises(lib.TSDFError, match="invalid argument"):
        eng.travel_field(dfield(d2.reshape(3, 3, 3), st.reshape(3, 3, 3)), glob([(1, 1, 1)]), clearance2=65026)
    with pytest.raises(ValueError):
        eng.travel_field(dict(dfield(d2.reshape(3, 3, 3), st.reshape(3, 3, 3)), state=None), glob([(1, 1, 1)]))

    # tsdf_travel_paths
    cost = tr.field(np.ones((3, 3, 3), bool), [(0, 0, 0)])[0]
    tg = np.array([2, 2, 2], np.int32)

    def pcall(h=0, dims=(3, 3, 3), costp=True, kind=0, T=1, tgp=True, max_len=4, pathp=True, lenp=True):
        path, ln = np.full(4, -99, np.int32), np.full(1, -99, np.int32)
        rc = L.tsdf_travel_paths(eng._h if h == 0 else h, (C.c_int32 * 3)(*dims) if dims else None,
                                 cost.ctypes.data if costp else None, kind, tg.ctypes.data if tgp else None, T, max_len,
                                 path.ctypes.data if pathp else None, ln.ctypes.data if lenp else None)
        return rc, bool((path == -99).all() and (ln == -99).all())

    assert pcall() == (0, False)
    assert pcall(T=0, tgp=False, pathp=False, lenp=False) == (0, True)
    bad = [dict(dims=(0, 3, 3)), dict(dims=(3, 3, 2049)), dict(dims=None), dict(costp=False), dict(kind=3), dict(T=-1),
           dict(tgp=False), dict(max_len=-1), dict(pathp=False), dict(lenp=False), dict(h=None),
           dict(T=2 ** 20, max_len=2 ** 11)]
    for kw in bad:
        assert pcall(**kw) == (TSDF_ERR_INVALID_ARG, True), kw
    assert eng.stats()["status"] == 0


def test_shard_engine():
    """The call does not touch the volume: a shard engine serves as well as any other."""
    small = tr.serpentine(24, 20, 8, pitch=2, gap=1)
    want, _ = tr.field(small, [(0, 0, 0)])
    assert want[7, 0, 22] != tr.UNREACHED
    shard = make_engine(shard_index=1, shard_count=2)
    try:
        for device in (False, True):
            got = shard.travel_field(dfield(*tr.arrays(small)), glob([(0, 0, 0)]), device=device)
            assert np.array_equal(host(got)["cost"], want)
            ps = shard.travel_paths(got, glob([(22, 0, 7)]))
            assert np.array_equal(ps[0], tr.paths(want, [(22, 0, 7)])[0][0])
    finally:
        shard.close()


def test_pending_frames_stay_as_they_were():
    """Frames integrated back to back, the call between them: the volume ends bit-identical to that of an
    engine that never made it."""
    import tsdf_amd
    from tsdf_amd import synth
    cam = synth.camera(80, 60)
    ok = tr.serpentine(24, 20, 9, pitch=4, gap=2)
    want, _ = tr.field(ok, [(0, 0, 0)])
    dumps, pipelined = [], []
    for with_call in (True, False):
        old = os.environ.get("TSDF_PIPELINE")
        os.environ["TSDF_PIPELINE"] = "1"
        try:
            e = tsdf_amd.Engine(voxel_size=0.005, truncation=0.03, max_width=80, max_height=60, num_block_bits=14)
        finally:
            if old is None:
                del os.environ["TSDF_PIPELINE"]
            else:
                os.environ["TSDF_PIPELINE"] = old
        try:
            e.profile_begin()
            for k in range(5):
                fr = synth.render(cam, k)
                e.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, tsdf_amd.SE3(fr["q"], fr["t"]), 4.0)
                if with_call and k in (1, 2):
                    got = e.travel_field(dfield(*tr.arrays(ok)), glob([(0, 0, 0)]), device=k == 2)
                    assert np.array_equal(host(got)["cost"], want)
            e.synchronize()
            # update launches that carried the next frame's tiles: a call that completed the pending frame
            # would have cost one each time
            pipelined.append(e.profile_end()["pipelined"])
            dumps.append((e.dump(), e.stats()))
        finally:
            e.close()
    print("pipelined launches with the calls and without:", pipelined)
    assert pipelined[0] == pipelined[1] >= 3
    (a, sa), (b, sb) = dumps
    for k in ("entry_pos", "entry_idx", "heap", "rgbw"):
        assert np.array_equal(a[k], b[k]), k
    assert a["free"] == b["free"]
    for k in ("tsdf", "prob"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for k in ("frames", "total_visible", "total_updated", "total_alloc", "total_deleted", "active_blocks", "status"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    assert sa["status"] == 0 and sa["frames"] == 5


@pytest.fixture(scope="module")
def scene(eng):
    """The imported floor-and-box volume's distance field, the restatement's on its dump, and the travel
    fields of the pinned cases by Dijkstra (computed once)."""
    eng.import_blocks(_edt_ref.scene_records(), replace=True)
    ref = _edt_ref.distance_field(eng.dump(), ORIGIN, DIMS)
    seed = np.array(SEED) - np.array(ORIGIN)
    cost = {k: tr.field(tr.passable(ref["d2"], ref["state"], k[0], bool(k[1])), [seed])[0] for k in SCENE}
    return dict(field=eng.distance_field(ORIGIN, DIMS), ref=ref, cost=cost)


def test_scene_end_to_end(eng, scene):
    f, ref = scene["field"], scene["ref"]
    assert np.array_equal(f["d2"], ref["d2"]) and np.array_equal(f["state"], ref["state"])
    for (c2, uf), (reached, largest) in SCENE.items():
        want = scene["cost"][c2, uf]
        assert (int((want != tr.UNREACHED).sum()), int(want[want != tr.UNREACHED].max())) == (reached, largest)
        got = eng.travel_field(f, [SEED], c2, bool(uf))
        print(f"scene clearance2={c2} unknown_free={uf}: rounds {got['rounds']}, differs at {int((got['cost'] != want).sum())}")
        assert got["origin"] == ORIGIN and got["dims"] == DIMS and got["seeded"] == 1
        assert np.array_equal(got["cost"], want)
    # device arrays straight from the distance field
    fd = eng.distance_field(ORIGIN, DIMS, device=True)
    got = eng.travel_field(fd, [SEED], 4, False, device=True)
    assert got["cost"].is_cuda and np.array_equal(got["cost"].cpu().numpy(), scene["cost"][4, 0])
    assert eng.stats()["status"] == 0


def test_paths(eng, maze, scene):
    import torch
    from tsdf_amd import esdf
    ok, want = maze
    far = np.argwhere(want == want[want != tr.UNREACHED].max())[0][::-1]
    rng = np.random.default_rng(8)


    def some(cost, first):
        """`first`, 25 reached voxels, 15 anywhere in the box and two outside it."""
        reached = np.argwhere(cost != tr.UNREACHED)[:, ::-1]
        return np.concatenate([first, reached[rng.integers(0, reached.shape[0], 25)],
                               rng.integers(0, cost.shape[::-1], (15, 3)), [(-1, 0, 0), (0, cost.shape[1], 0)]])

    cases = [(want, BOX, some(want, [far, (0, 0, 0), (1, 5, 5), (0, 0, 8)])),
             (scene["cost"][0, 1], ORIGIN, some(scene["cost"][0, 1], [(0, 0, 0), (76, 69, 58), (17, 15, 16)])),
             (scene["cost"][4, 0], ORIGIN, some(scene["cost"][4, 0], [(17, 15, 16)]))]
    for cost, origin, targets in cases:
        ps, lens = tr.paths(cost, targets)
        assert sum(1 for n in lens if n > 1) > 5 and 0 in lens
        for device in (False, True):
            c = torch.as_tensor(cost, device=f"cuda:{eng.device}") if device else cost
            t = dict(cost=c, origin=origin, dims=cost.shape[::-1])
            got = eng.travel_paths(t, glob(targets, origin), max_len=16)  # (asks again: the longest is longer)
            assert len(got) == len(ps) and all(g.dtype == np.int32 for g in got)
            assert all(np.array_equal(g, p) for g, p in zip(got, ps)), device
    assert max(lens) > 16
    # world positions of a path: seed first
    t = dict(cost=want, origin=BOX, dims=want.shape[::-1])
    p = eng.travel_paths(t, glob([far]))[0]
    pts = esdf.path_points(t, VOXEL, p)
    assert len(p) > 600 and np.array_equal(pts[0], np.array(BOX).astype(np.float32) * np.float32(VOXEL))
    assert np.array_equal(pts[-1], (far + np.array(BOX)).astype(np.float32) * np.float32(VOXEL))


def test_paths_truncation_and_tampering(eng, maze):
    import torch
    import tsdf_amd
    L = tsdf_amd._lib.load()
    ok, want = maze
    far = np.argwhere(want == want[want != tr.UNREACHED].max())[0][::-1]
    targets = np.ascontiguousarray(np.array([far, (1, 0, 0), (0, 0, 0), (-1, 0, 0), (2, 0, 0)]), np.int32)
    assert not ok[0, 0, 1]
    full, lens = tr.paths(want, targets)
    assert lens[0] > 600 and lens[1:] == [0, 1, 0, lens[4]] and lens[4] > 60
    bad = want.copy()
    bad[want < want.ravel()[full[0][4]]] = tr.UNREACHED  # (nothing cheaper than the walk's fifth voxel is left)
    dims = (C.c_int32 * 3)(*want.shape[::-1])
    for cost in (want, bad):
        ref, wl = tr.paths(cost, targets)
        assert wl[0] == (lens[0] if cost is want else -5)
        for device in (False, True):
            c = torch.as_tensor(cost, device=f"cuda:{eng.device}") if device else cost
            path, ln = np.full((5, 8), -99, np.int32), np.full(5, -99, np.int32)
            if device:
                torch.cuda.synchronize()
            rc = L.tsdf_travel_paths(eng._h, dims, C.c_void_p(c.data_ptr()) if device else c.ctypes.data, int(device),
                                     targets.ctypes.data, 5, 8, path.ctypes.data, ln.ctypes.data)
            assert rc == 0 and ln.tolist() == wl, (device, ln.tolist())
            for k in range(5):
                n = min(abs(wl[k]), 8)
                assert np.array_equal(path[k, :n], ref[k][:n]) and (path[k, n:] == -99).all()
    with pytest.raises(ValueError, match="predecessor"):
        eng.travel_paths(dict(cost=bad, origin=BOX, dims=want.shape[::-1]), glob([far]))


def test_facade(scene, tmp_path):
    """DISINFSystem::query_travel_field and TSDFSystem::TravelPaths (travel_main) on the scene's records: the
    cube whose voxel centres are the main box, 2 cm clearance."""
    lo = [(ORIGIN[a] - 0.3) * VOXEL for a in range(3)]
    hi = [(ORIGIN[a] + DIMS[a] - 1 + 0.3) * VOXEL for a in range(3)]
    cube = " ".join(f"{lo[a]:.6f} {hi[a]:.6f}" for a in range(3))
    want = scene["cost"][4, 0]
    targets = np.argwhere(want == 225)[:1, ::-1].tolist() + [[0, 0, 0], [17, 15, 30]]
    tg = " ".join(str(v) for v in glob(targets, ORIGIN).reshape(-1))
    frm = " ".join(f"{SEED[a] * VOXEL:.6f}" for a in range(3))
    (tmp_path / "meta.txt").write_text(f"{VOXEL} {TRUNC} {NB_BITS} 255 1 0 {cube} 0.0199 0 {frm} {len(targets)} {tg}\n")
    _edt_ref.scene_records().tofile(tmp_path / "blocks.bin")
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    box = [int(v) for v in (tmp_path / "out_box.txt").read_text().split()]
    assert box[:7] == [*ORIGIN, *DIMS, 1] and box[7] > 0 and box[8] == int(want[0, 0, 0])
    cost = np.fromfile(tmp_path / "out_cost.bin", np.uint32).reshape(DIMS[::-1])
    assert np.array_equal(cost, want)
    got = [np.array(ln.split(), np.int32) for ln in (tmp_path / "out_paths.txt").read_text().split("\n")[:len(targets)]]
    ps, lens = tr.paths(want, targets)
    assert lens[0] > 40 and all(np.array_equal(g, p) for g, p in zip(got, ps))
