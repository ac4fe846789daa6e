"""tsdf_frontier_mark and tsdf_components on the GPU against their numpy restatement (_frontier_ref.py): labels
and the whole cluster table bit for bit, host and device memory. The figures asserted here are computed in
tests/test_frontier_cpu.py from the restatement alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _edt_ref
import _frontier_ref as fr
import _travel_ref as tr
from _edt_ref import NB_BITS, TRUNC, VOXEL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "frontier_main")
SHAPES = [(7, 9, 12), (1, 1, 1), (5, 1, 8), (1, 9, 1), (9, 17, 20), (16, 16, 24), (9, 10, 21)]
FIGURES = {0.04: 300, 0.1: 294, 0.3: 24}  # components over SHAPES (test_frontier_cpu.FIGURES)
ORIGIN, DIMS, SEED = (-37, -35, -21), (77, 70, 59), (-20, -20, -5)
SCENE = {False: (5528, 1, 5528), True: (5276, 1, 5276)}  # test_frontier_cpu.SCENE
BOX = (5, -11, 3)
TSDF_ERR_INVALID_ARG, TSDF_ERR_CAPACITY = 1, 4


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
    assert e.stats()["status"] == 0
    e.close()


def host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else a


def same_table(got, want):
    return got.dtype == want.dtype == fr.COMPONENT_DTYPE and got.shape == want.shape and got.tobytes() == want.tobytes()


def check(e, mask, key=None, min_size=1, tag="", kinds=(False, True), want=None):
    """Both memory kinds against the flood fill's labelling and its table; returns (labels, table, total)."""
    import torch
    mask = np.ascontiguousarray(mask)
    lab = fr.label_flood(mask) if want is None else want
    tab, total = fr.table(lab, key, min_size)
    m8 = mask.astype(np.uint8)
    for device in kinds:
        m = torch.as_tensor(m8, device=f"cuda:{e.device}") if device else m8
        k = key if key is None or not device else torch.as_tensor(key, device=f"cuda:{e.device}")
        got = e.components(m, mask.shape[::-1], key=k, min_size=min_size, device=device)
        gl = host(got["label"])
        print(f"{tag} device={device}: {total} components, {len(tab)} of {min_size}+ voxels, labels differ at "
              f"{int((gl != lab).sum())} of {lab.size}, table equal {same_table(got['clusters'], tab)}")
        assert bool(hasattr(got["label"], "is_cuda")) == device
        assert gl.dtype == np.uint32 and gl.shape == mask.shape and np.array_equal(gl, lab)
        assert (got["count"], got["total"]) == (len(tab), total)
        assert same_table(got["clusters"], tab)
    return lab, tab, total


@pytest.mark.parametrize("density", sorted(FIGURES))
def test_shapes(eng, density):
    """Dims of 1, dims that are no multiple of the tile, one tile and several; min_size; keys with ties."""
    rng = np.random.default_rng(7)
    total, ties = 0, 0
    for shape, mask in zip(SHAPES, fr.masks(SHAPES, density)):
        lab, tab, n = check(eng, mask, tag=f"shape {shape} density {density}")
        total += n
        check(eng, mask, min_size=3, tag="min_size 3", want=lab)
        key = rng.integers(0, 3, shape).astype(np.uint32) * np.uint32(0x40000001)
        _, tk, _ = check(eng, mask, key=key, tag="keys", want=lab)
        # a tie: another member of the cluster holds the goal's key at a greater index
        flat_k, flat_l = key.reshape(-1), lab.reshape(-1)
        for c in tk:
            same = np.flatnonzero((flat_l == c["label"]) & (flat_k == c["goal_key"]))
            assert same[0] == c["goal"]
            ties += same.size > 1
        check(eng, mask, key=key, min_size=3, tag="keys, min_size 3", want=lab, kinds=(True,))
    assert total == FIGURES[density] and ties > 3


def two_voxels(d, step):
    seed = [7 if v > 0 else (8 if v < 0 else 3) for v in d]
    other = [s + step * v for s, v in zip(seed, d)]
    mask = np.zeros((16, 16, 16), bool)
    mask[seed[2], seed[1], seed[0]] = mask[other[2], other[1], other[0]] = True
    return mask, sorted((p[2] * 16 + p[1]) * 16 + p[0] for p in (seed, other))


def test_across_every_tile_border(eng):
    """Two members a step apart across the 7 | 8 border, for all 26 directions, are one component labelled by
    the lesser voxel; two steps apart they are two."""
    n = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx, dy, dz) == (0, 0, 0):
                    continue
                mask, (lo, hi) = two_voxels((dx, dy, dz), 1)
                lab, tab, total = check(eng, mask, tag=f"step {(dx, dy, dz)}")
                assert total == 1 and tab["label"][0] == lo and tab["size"][0] == 2 and lab.reshape(-1)[hi] == lo
                mask, (lo, hi) = two_voxels((dx, dy, dz), 2)
                lab, tab, total = check(eng, mask, tag=f"two steps {(dx, dy, dz)}", kinds=(n % 2 == 0,))
                assert total == 2 and tab["label"].tolist() == [lo, hi]
                n += 1
    assert n == 26


def test_joined_only_through_a_neighbouring_tile(eng):
    """Tile 0 holds two roots (six for the comb) of one global component: the link runs through tile 1."""
    bars = np.zeros((8, 8, 16), bool)
    bars[3, 1, 0:8] = bars[3, 5, 0:8] = True
    assert fr.table(fr.label_flood(bars))[1] == 2
    bars[3, 1:6, 8] = True
    lab, tab, total = check(eng, bars, tag="bars")
    assert total == 1 and tab["label"][0] == (3 * 8 + 1) * 16 and tab["size"][0] == 21
    comb = np.zeros((8, 8, 16), bool)
    for y, z in ((0, 0), (3, 0), (6, 0), (0, 4), (3, 4), (6, 4)):
        comb[z, y, 0:8] = True
    assert fr.table(fr.label_flood(comb))[1] == 6
    comb[:, :, 8] = True
    for name, m in (("bars", bars), ("comb", comb)):
        for axes in ((0, 1, 2), (0, 2, 1), (2, 1, 0)):  # the long axis along x, y and z
            for flip in (False, True):  # the teeth in the first tile, and in the second
                t = np.ascontiguousarray(np.transpose(m, axes))
                t = np.ascontiguousarray(t[::-1, ::-1, ::-1]) if flip else t
                _, tab, total = check(eng, t, tag=f"{name} axes {axes} flip {flip}")
                assert total == 1 and tab["size"][0] == int(m.sum())


@pytest.fixture(scope="module")
def maze():
    ok = tr.serpentine(64, 64, 8, pitch=2, gap=1)
    return ok, fr.label_flood(ok)


def test_long_chains(eng, maze):
    """One component that crosses more than 200 tile faces, its least index at either end; the walls between."""
    ok, want = maze
    _, tab, total = check(eng, ok, tag="maze", want=want)
    assert total == 1 and (tab["label"][0], tab["size"][0]) == (0, 16640)
    assert tab["lo"][0].tolist() == [0, 0, 0] and tab["hi"][0].tolist() == [63, 63, 7]
    mirrored = np.ascontiguousarray(ok[::-1, :, ::-1])
    _, tab, total = check(eng, mirrored, tag="maze mirrored in x and z")
    assert total == 1 and tab["size"][0] == 16640 and tab["label"][0] == 0
    _, tab, total = check(eng, ~ok, tag="walls")
    assert total == 32 and set(tab["size"].tolist()) == {504}
    # keyed by the travel cost from the far end: the goal is that end
    cost, _ = tr.field(ok, [(62, 0, 7)])
    _, tab, _ = check(eng, ok, key=cost, tag="maze keyed", want=want)
    assert tab["goal"][0] == (7 * 64 + 0) * 64 + 62 and tab["goal_key"][0] == 0


def raw(e, mask, capacity, key=None, min_size=1, device=False, clusters=True, dims=None, h=0, maskp=True, labelp=True,
        countp=True, totalp=True, cfg=True, kind=None):
    """tsdf_components through ctypes: (rc, labels, table, count, total); sentinels where nothing was written."""
    import torch
    import tsdf_amd
    lib = tsdf_amd._lib
    L = lib.load()
    mask = np.ascontiguousarray(mask, np.uint8)
    d = mask.shape[::-1] if dims is None else dims
    c = lib.ComponentsConfig((C.c_int32 * 3)(*d), min_size)
    label = np.full(mask.shape, 0xABCD1234, np.uint32)
    tab = np.frombuffer(bytearray(b"\xAB" * (64 * max(capacity, 1))), fr.COMPONENT_DTYPE)
    count, total = C.c_int32(-7), C.c_int32(-7)
    if device:
        dm, dl = torch.as_tensor(mask, device=f"cuda:{e.device}"), torch.as_tensor(label, device=f"cuda:{e.device}")
        dk = None if key is None else torch.as_tensor(key, device=f"cuda:{e.device}")
        torch.cuda.synchronize()
        pm, pl, pk = dm.data_ptr(), dl.data_ptr(), None if dk is None else dk.data_ptr()
    else:
        pm, pl, pk = mask.ctypes.data, label.ctypes.data, None if key is None else key.ctypes.data
    rc = L.tsdf_components(e._h if h == 0 else h, C.byref(c) if cfg else None, pm if maskp else None, pk,
                           pl if labelp else None, (int(device) if kind is None else kind),
                           tab.ctypes.data if clusters else None, capacity, C.byref(count) if countp else None,
                           C.byref(total) if totalp else None)
    if device:
        label = dl.cpu().numpy()
    return rc, label, tab, count.value, total.value


def test_table_edges(eng):
    mask = fr.masks([(9, 17, 20)], 0.1)[0]
    key = np.random.default_rng(3).integers(0, 50, mask.shape).astype(np.uint32)
    lab = fr.label_flood(mask)
    want, total = fr.table(lab, key, 2)
    n = len(want)
    assert 3 < n < total
    untouched = bytes([0xAB]) * 64
    for device in (False, True):
        rc, gl, tab, count, tot = raw(eng, mask, n, key, 2, device)  # capacity == count
        assert rc == 0 and (count, tot) == (n, total) and np.array_equal(gl, lab) and same_table(tab, want)
        rc, gl, tab, count, tot = raw(eng, mask, n + 2, key, 2, device)  # room to spare stays as it was
        assert rc == 0 and same_table(tab[:n], want) and tab[n:].tobytes() == 2 * untouched
        rc, gl, tab, count, tot = raw(eng, mask, n - 1, key, 2, device)  # one too few
        assert rc == TSDF_ERR_CAPACITY and (count, tot) == (n, total) and np.array_equal(gl, lab)
        assert tab.tobytes() == (n - 1) * untouched
        rc, gl, tab, count, tot = raw(eng, mask, 0, key, 2, device, clusters=False)  # the query form
        assert rc == 0 and (count, tot) == (n, total) and np.array_equal(gl, lab)
        rc, gl, tab, count, tot = raw(eng, mask, 5, key, int(want["size"].max()) + 1, device)  # above every size
        assert rc == 0 and (count, tot) == (0, total) and np.array_equal(gl, lab) and tab.tobytes() == 5 * untouched
        rc, gl, tab, count, tot = raw(eng, mask, 0, key, 2, device, totalp=False)  # total may be NULL
        assert rc == 0 and count == n
    # empty and full masks, several tiles with ragged edges
    shape = (9, 17, 20)
    nz, ny, nx = shape
    lab, tab, total = check(eng, np.zeros(shape, bool), tag="empty")
    assert total == 0 and len(tab) == 0 and (lab == fr.NONE).all()
    lab, tab, total = check(eng, np.ones(shape, bool), tag="full")
    assert total == 1 and (lab == 0).all() and tab["size"][0] == nx * ny * nz
    assert tab["sum"][0].tolist() == [ny * nz * nx * (nx - 1) // 2, nx * nz * ny * (ny - 1) // 2, nx * ny * nz * (nz - 1) // 2]
    assert tab["lo"][0].tolist() == [0, 0, 0] and tab["hi"][0].tolist() == [nx - 1, ny - 1, nz - 1]
    assert (tab["goal"][0], tab["goal_key"][0]) == (0, 0)


def random_states(rng, shape):
    return rng.choice(np.array([0, 1, 2], np.uint8), size=shape, p=[0.4, 0.45, 0.15])


def check_mark(e, state, cost=None, tag=""):
    import torch
    want = fr.mark(state, cost)
    field = dict(d2=None, state=state, origin=BOX, dims=state.shape[::-1])
    travel = None if cost is None else dict(cost=cost, origin=BOX, dims=state.shape[::-1])
    for device in (False, True):
        f, t = field, travel
        if device:
            f = dict(field, state=torch.as_tensor(state, device=f"cuda:{e.device}"))
            t = None if travel is None else dict(travel, cost=torch.as_tensor(cost, device=f"cuda:{e.device}"))
        got = e.frontier_mask(f, t, device=device)
        m = host(got["mask"])
        print(f"{tag} device={device}: marked {int(want.sum())} of {want.size}, differs at {int((m != want).sum())}")
        assert m.dtype == np.uint8 and np.array_equal(m, want) and got["marked"] == int(want.sum())
        assert got["origin"] == BOX and got["dims"] == state.shape[::-1]
    # marked NULL: a device call does not synchronise; the mask is there once the stream is
    got = e.frontier_mask(f, t, device=True, count=False)
    assert got["marked"] is None and np.array_equal(got["mask"].cpu().numpy(), want)
    return want


def test_frontier_mark(eng):
    rng = np.random.default_rng(11)
    marked = 0
    for shape in SHAPES:
        state = random_states(rng, shape)
        marked += int(check_mark(eng, state, tag=f"mark {shape}").sum())
        # with a travel field over these states, and with costs unreached at random
        free = np.argwhere(state == 1)[:, ::-1]
        seeds = free[rng.integers(0, free.shape[0], 2)] + np.array(BOX) if free.shape[0] else np.zeros((0, 3), int)
        travel = eng.travel_field(dict(d2=np.full(shape, 100, np.uint16), state=state, origin=BOX, dims=shape[::-1]), seeds)
        w = check_mark(eng, state, travel["cost"], tag=f"mark {shape} with a travel field")
        assert w.sum() <= fr.mark(state).sum()
        cost = rng.integers(0, 9, shape).astype(np.uint32)
        cost[rng.random(shape) < 0.5] = fr.UNREACHED
        check_mark(eng, state, cost, tag=f"mark {shape} with random costs")
    assert marked > 1500
    # state 0 only outside the box: nothing to touch
    assert check_mark(eng, np.ones((9, 10, 21), np.uint8), tag="all free").sum() == 0
    assert check_mark(eng, rng.integers(1, 3, (9, 10, 21)).astype(np.uint8), tag="free and inside").sum() == 0
    # one unobserved voxel in a tile's corner: its six neighbours lie in four tiles
    state = np.ones((16, 16, 16), np.uint8)
    state[8, 8, 8] = 0
    assert check_mark(eng, state, tag="corner").sum() == 6


def test_arguments(eng):
    import tsdf_amd
    lib = tsdf_amd._lib
    L = lib.load()
    mask = np.zeros((3, 3, 3), np.uint8)
    mask[1, 1, 1] = mask[0, 0, 0] = 1

    def call(**kw):
        rc, label, tab, count, total = raw(eng, mask, kw.pop("capacity", 4), **kw)
        return rc, bool((label == 0xABCD1234).all()) and tab.tobytes() == bytes([0xAB]) * tab.nbytes and (count, total) == (-7, -7)

    assert call() == (0, False)
    bad = [dict(dims=(0, 3, 3)), dict(dims=(3, 2049, 3)), dict(dims=(3, 3, -1)), dict(dims=(2048, 2048, 65)),
           dict(min_size=0), dict(min_size=-3), dict(capacity=-1), dict(h=None), dict(cfg=False), dict(maskp=False),
           dict(labelp=False), dict(countp=False), dict(clusters=False, capacity=2), dict(kind=2), dict(kind=-1)]
    for kw in bad:
        assert call(**kw) == (TSDF_ERR_INVALID_ARG, True), kw
    with pytest.raises(lib.TSDFError, match="invalid argument"):
        eng.components(mask, (3, 3, 3), min_size=0)
    with pytest.raises(ValueError):
        eng.components(mask, (3, 3, 4))
    with pytest.raises(ValueError):
        eng.components(mask, (3, 3, 3), key=np.zeros((3, 3, 4), np.uint32))

    # tsdf_frontier_mark
    state = np.ones(27, np.uint8)
    state[13] = 0
    cost = np.zeros(27, np.uint32)

    def mcall(h=0, dims=(3, 3, 3), statep=True, costp=True, maskp=True, kind=0, markedp=True):
        out = np.full(27, 0xCD, np.uint8)
        n = C.c_int64(-7)
        rc = L.tsdf_frontier_mark(eng._h if h == 0 else h, (C.c_int32 * 3)(*dims) if dims else None,
                                  state.ctypes.data if statep else None, cost.ctypes.data if costp else None,
                                  out.ctypes.data if maskp else None, kind, C.byref(n) if markedp else None)
        return rc, bool((out == 0xCD).all()) and n.value == -7

    assert mcall() == (0, False)
    assert mcall(costp=False)[0] == 0 and mcall(markedp=False)[0] == 0
    bad = [dict(dims=(0, 3, 3)), dict(dims=(3, 3, 2049)), dict(dims=(2048, 2048, 65)), dict(dims=None), dict(statep=False),
           dict(maskp=False), dict(kind=3), dict(kind=-1), dict(h=None)]
    for kw in bad:
        assert mcall(**kw) == (TSDF_ERR_INVALID_ARG, True), kw
    field = dict(d2=None, state=state.reshape(3, 3, 3), origin=BOX, dims=(3, 3, 3))
    with pytest.raises(ValueError):
        eng.frontier_mask(dict(field, state=None))
    with pytest.raises(ValueError):
        eng.frontier_mask(field, dict(cost=cost.reshape(3, 3, 3), origin=(0, 0, 0), dims=(3, 3, 3)))
    with pytest.raises(ValueError):
        eng.frontiers(dict(field, dims=(3, 3, 4)))
    assert eng.stats()["status"] == 0


def test_repeat_and_scratch_growth(maze):
    """Small, the maze, small again on a fresh engine: the scratch grows, and a small box with many components
    makes the call count them before it sizes their accumulators."""
    ok, want = maze
    small = fr.masks([(7, 9, 12)], 0.04)[0]
    assert fr.table(fr.label_flood(small))[1] > 10
    e = make_engine()  # (a fresh engine: its scratch starts empty)
    try:
        a = check(e, small, tag="small", kinds=(False,))
        check(e, small, tag="small again", kinds=(False, True), want=a[0])
        check(e, ok, tag="maze", want=want)
        check(e, ~ok, tag="walls", kinds=(True,))
        check(e, small, tag="small after the maze", want=a[0])
        dense = fr.masks([(64, 64, 64)], 0.03)[0]  # more components than a voxel in 512: labelled twice
        _, _, total = check(e, dense, tag="many components", kinds=(True, False))
        assert total > max(4096, dense.size >> 9)
        check(e, dense, tag="many components again", kinds=(True,))
        assert e.stats()["status"] == 0
    finally:
        e.close()


def test_shard_engine(maze):
    """The calls do not touch the volume: a shard engine serves as well as any other."""
    shard = make_engine(shard_index=1, shard_count=2)
    try:
        check(shard, fr.masks([(9, 17, 20)], 0.1)[0], tag="shard")
        check_mark(shard, random_states(np.random.default_rng(5), (9, 17, 20)), tag="shard mark")
    finally:
        shard.close()


def test_pending_frames_stay_as_they_were():
    """Frames integrated back to back, the calls between them: the volume ends bit-identical to that of an
    engine that never made them, with the same number of pipelined launches."""
    import tsdf_amd
    from tsdf_amd import synth
    cam = synth.camera(80, 60)
    mask = fr.masks([(9, 17, 20)], 0.1)[0]
    state = random_states(np.random.default_rng(6), (9, 17, 20))
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
                f = synth.render(cam, k)
                e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], cam.K, tsdf_amd.SE3(f["q"], f["t"]), 4.0)
                if with_call and k in (1, 2):
                    check(e, mask, tag="between frames", kinds=(k == 2,))
                    check_mark(e, state, tag="between frames")
            e.synchronize()
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


def test_frames_end_to_end():
    """Frames, the free layer, the distance field, free_apply, the travel field, Engine.frontiers: labels and
    table equal the restatement run on the arrays the GPU returned."""
    import tsdf_amd
    from tsdf_amd import esdf, synth
    voxel, trunc = 0.02, 0.08
    cam = synth.camera(80, 60)
    frames = [synth.render(cam, k) for k in (0, 10, 20)]
    last = tsdf_amd.SE3(frames[-1]["q"], frames[-1]["t"])

    def in_front(z):
        p = last.Inverse().Apply(np.array([0.0, 0.0, z], np.float32))
        return np.round(p.astype(np.float64) / voxel).astype(np.int64)

    dims = (100, 100, 60)
    origin = tuple(int(v) for v in in_front(1.0) - np.array(dims) // 2)
    seed = in_front(0.3)
    for device in (False, True):
        e = tsdf_amd.Engine(voxel, trunc, max_width=80, max_height=60, num_block_bits=13)
        try:
            layer = esdf.free_layer(origin, dims, device=device)
            for f in frames:
                pose = tsdf_amd.SE3(f["q"], f["t"])
                e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], cam.K, pose, 4.0)
                e.free_observe(layer, f["depth"], cam.K, pose, 4.0)
            field = e.free_apply(layer, e.distance_field(origin, dims, device=device))
            travel = e.travel_field(field, [seed], clearance2=4, unknown_free=False, device=device)
            got = e.frontiers(field, travel, min_size=4, device=device)
            state, cost = host(field["state"]), host(travel["cost"])
            mask = fr.mark(state, cost)
            lab = fr.label_flood(mask)
            tab, total = fr.table(lab, cost, 4)
            print(f"frames device={device}: promoted {field['promoted']}, seeded {travel['seeded']}, reached "
                  f"{int((cost != fr.UNREACHED).sum())}, marked {got['marked']}, components {got['total']}, clusters "
                  f"{got['count']}, largest {int(tab['size'].max()) if len(tab) else 0}")
            assert travel["seeded"] == 1 and got["marked"] == int(mask.sum()) > 100 and len(tab) >= 1
            assert got["origin"] == origin and got["dims"] == dims
            assert np.array_equal(host(got["mask"]), mask) and np.array_equal(host(got["label"]), lab)
            assert (got["count"], got["total"]) == (len(tab), total) and same_table(got["clusters"], tab)
            # every goal is a frontier voxel the arm reaches, no farther than any other of its cluster
            goals = esdf.frontier_goals(got, voxel)
            flat = cost.reshape(-1)
            assert (flat[tab["goal"]] == tab["goal_key"]).all() and np.isfinite(goals["metres"]).all()
            k = int(np.argmax(tab["size"]))
            vox = esdf.frontier_voxels(got, k) - np.array(origin)
            assert vox.shape[0] == tab["size"][k] and cost[vox[:, 2], vox[:, 1], vox[:, 0]].min() == tab["goal_key"][k]
            assert e.stats()["status"] == 0
        finally:
            e.close()


@pytest.fixture(scope="module")
def scene(eng):
    eng.import_blocks(_edt_ref.scene_records(), replace=True)
    return eng.distance_field(ORIGIN, DIMS)


@pytest.mark.parametrize("with_travel", [False, True])
def test_scene(eng, scene, with_travel):
    """The floor-and-box scene: the figures of test_frontier_cpu.test_scene_figures."""
    travel = eng.travel_field(scene, [SEED], 4, False) if with_travel else None
    got = eng.frontiers(scene, travel, min_size=8)
    cost = None if travel is None else travel["cost"]
    mask = fr.mark(scene["state"], cost)
    lab = fr.label_flood(mask)
    tab, total = fr.table(lab, cost, 8)
    assert (got["marked"], got["count"], int(got["clusters"]["size"].max())) == SCENE[with_travel]
    assert np.array_equal(got["mask"], mask) and np.array_equal(got["label"], lab)
    assert got["total"] == total and same_table(got["clusters"], tab)


def test_facade(eng, scene, tmp_path):
    """DISINFSystem::query_frontiers (frontier_main) on the scene's records reproduces the Python result."""
    from tsdf_amd import esdf
    travel = eng.travel_field(scene, [SEED], 4, False)
    want = eng.frontiers(scene, travel, min_size=8)
    lo = [(ORIGIN[a] - 0.3) * VOXEL for a in range(3)]
    hi = [(ORIGIN[a] + DIMS[a] - 1 + 0.3) * VOXEL for a in range(3)]
    cube = " ".join(f"{lo[a]:.6f} {hi[a]:.6f}" for a in range(3))
    frm = " ".join(f"{SEED[a] * VOXEL:.6f}" for a in range(3))
    (tmp_path / "meta.txt").write_text(f"{VOXEL} {TRUNC} {NB_BITS} 255 {cube} 0.0199 0 {frm} 8\n")
    _edt_ref.scene_records().tofile(tmp_path / "blocks.bin")
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print("frontier_main:", r.stdout.strip())
    assert [int(v) for v in r.stdout.split()] == [*ORIGIN, *DIMS, want["marked"], want["total"], want["count"]]
    assert np.array_equal(np.fromfile(tmp_path / "out_mask.bin", np.uint8).reshape(DIMS[::-1]), want["mask"])
    assert np.array_equal(np.fromfile(tmp_path / "out_label.bin", np.uint32).reshape(DIMS[::-1]), want["label"])
    assert same_table(np.fromfile(tmp_path / "out_clusters.bin", fr.COMPONENT_DTYPE), want["clusters"])
    g = esdf.frontier_goals(want, np.float32(VOXEL))
    goals = np.fromfile(tmp_path / "out_goals.bin", np.float32).reshape(-1, 7)
    assert np.array_equal(goals[:, :3], g["goal"]) and np.array_equal(goals[:, 3:6], g["centroid"])
    assert np.array_equal(goals[:, 6], g["metres"])
