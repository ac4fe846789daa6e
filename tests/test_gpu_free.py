"""Observed free space (tsdf_free_observe, tsdf_free_apply) against tests/_free_ref.py, the numpy restatement of
the contract, bit for bit: boxes of many shapes on rendered frames with rotated poses, host and device memory,
the census stream that stands on every gate of the test (tests/_free_cases.py), accumulation and the full-word
skip, the brick culls with the camera inside the box and an engine created without them, apply between boxes
that nest, overlap and miss each other, refused arguments, a shard engine, an engine with pending frames, the
wall-with-a-gap scenario end to end on device arrays, and the facade (free_main). Every comparison is exact."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _free_cases as fc
import _free_ref as fref
import _geo_edges as ge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "free_main")
VOXEL, TRUNC, MAX_DEPTH = 0.02, 0.08, 4.0
TSDF_ERR_INVALID_ARG = 1
f32 = np.float32


def make_engine(voxel=VOXEL, trunc=TRUNC, w=80, h=60, env=None, nb_bits=13, **kw):
    import tsdf_amd
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return tsdf_amd.Engine(voxel, trunc, max_width=w, max_height=h, num_block_bits=nb_bits, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def eng():
    # torch's HIP runtime first (conftest._torch_hip_first runs after module fixtures)
    import torch
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    e = make_engine()
    yield e
    e.close()


@functools.lru_cache(None)
def synth_frame(k):
    """Rendered 80 x 60 frame k with its rotated pose, as a _free_ref frame."""
    from tsdf_amd import synth
    cam = synth.camera(80, 60)
    s = synth.render(cam, k)
    return fref.frame(s["depth"], cam.K, s["q"], s["t"], MAX_DEPTH)


@pytest.fixture(scope="module")
def synth_frames():
    return [synth_frame(k) for k in (0, 40, 200)]


def pose_of(fr):
    import tsdf_amd
    return tsdf_amd.SE3(fr["q"], fr["t"])


def in_front(fr, metres, voxel=VOXEL):
    """The global voxel nearest to the point `metres` (x, y, z in camera space) of a frame's camera."""
    p = pose_of(fr).Inverse().Apply(np.asarray(metres, f32))
    return np.round(p.astype(np.float64) / voxel).astype(np.int64)


def words(layer):
    b = layer["bits"]
    return b.cpu().numpy().view(np.uint32) if hasattr(b, "is_cuda") else b


def observe(e, origin, dims, frames, device, voxel=VOXEL, pre=None):
    """A layer (cleared, or holding `pre`) after the frames, as host words."""
    from tsdf_amd import esdf
    layer = esdf.free_layer(origin, dims, device=device)
    if pre is not None:
        if device:
            import torch
            layer["bits"].copy_(torch.as_tensor(pre.view(np.int32), device=layer["bits"].device))
        else:
            layer["bits"][:] = pre
    for fr in frames:
        assert e.free_observe(layer, fr["depth"], fr["K"], pose_of(fr), float(fr["max_depth"])) is layer
    return words(layer)


def check(e, origin, dims, frames, voxel=VOXEL, trunc=TRUNC, tag="", want=None):
    """Both memory kinds against the restatement; returns the mask."""
    if want is None:
        want = np.zeros(tuple(dims)[::-1], bool)
        for fr in frames:
            want |= fref.frame_mask(origin, dims, fr, voxel, trunc)
    for device in (False, True):
        got = observe(e, origin, dims, frames, device, voxel)
        diff = int((fref.unpack(got, dims[0]) != want).sum())
        print(f"{tag} box {tuple(origin)} + {tuple(dims)} device={device}: free {int(want.sum())} of {want.size}, "
              f"differs at {diff}, padding {fref.padding(got, dims[0]):#x}")
        assert got.shape == (dims[2], dims[1], (dims[0] + 31) // 32)
        assert np.array_equal(got, fref.pack(want))
        assert fref.padding(got, dims[0]) == 0
    return want


def test_shapes(eng, synth_frames):
    """Row lengths around the word and the wave (1, 31 .. 33, 63 .. 65, 130), 1, 3 and 9 rows and slabs, odd
    origins, in front of three rotated cameras."""
    free, total, k = 0, 0, 0
    for nx in (1, 31, 32, 33, 63, 64, 65, 130):
        for ny, nz in ((1, 1), (3, 9), (9, 3), (1, 9), (9, 1), (3, 3))[k % 2::2]:
            fr = synth_frames[k % 3]
            origin = in_front(fr, (0.0, 0.0, 0.9)) - np.array([nx // 2, ny // 2, nz // 2]) + (k % 2)
            m = check(eng, origin.tolist(), (nx, ny, nz), [fr], tag="shapes")
            free, total, k = free + int(m.sum()), total + m.size, k + 1
    print(f"shapes: {free} free of {total}")
    assert 2000 < free < total - 2000
    assert eng.stats()["status"] == 0


def test_gates():
    """The census stream (tests/test_free_cpu.py asserts it stands on every gate), frame by frame and accumulated."""
    e = make_engine(ge.VOXEL, ge.TRUNC, ge.W, ge.H)
    try:
        frames = fc.census_frames()
        for name in fc.CENSUS_FRAMES:
            check(e, fc.CENSUS_ORIGIN, fc.CENSUS_DIMS, [frames[name]], ge.VOXEL, ge.TRUNC, tag=f"gates {name}",
                  want=fc.census_terms(name)["free"])
        union = np.zeros(fc.CENSUS_DIMS[::-1], bool)
        for name in fc.CENSUS_FRAMES:
            union |= fc.census_terms(name)["free"]
        check(e, fc.CENSUS_ORIGIN, fc.CENSUS_DIMS, [frames[k] for k in fc.CENSUS_FRAMES], ge.VOXEL, ge.TRUNC,
              tag="gates, all", want=union)
        assert e.stats()["status"] == 0
    finally:
        e.close()


def test_accumulate(eng):
    """Five frames ORed; a frame twice; a layer that already holds random bits and all-ones words."""
    synth_frames = [synth_frame(k) for k in (0, 10, 20, 30, 40)]
    dims = (70, 20, 12)  # (a row's last word has 6 bits in range)
    origin = (in_front(synth_frames[0], (0.0, 0.0, 2.0)) - np.array([35, 10, 6])).tolist()
    single = [fref.frame_mask(origin, dims, fr, VOXEL, TRUNC) for fr in synth_frames]
    union = np.logical_or.reduce(single)
    print("accumulate: per frame", [int(m.sum()) for m in single], "union", int(union.sum()))
    assert union.sum() > max(m.sum() for m in single) > 1000
    check(eng, origin, dims, synth_frames, tag="accumulate", want=union)
    check(eng, origin, dims, [synth_frames[1], synth_frames[1]], tag="twice", want=single[1])
    rng = np.random.default_rng(5)
    pre = rng.integers(0, 2 ** 32, (dims[2], dims[1], 3), dtype=np.uint64).astype(np.uint32)
    pre[rng.random(pre.shape) < 0.3] = 0xFFFFFFFF
    pre[::2, ::3, 2] = 0x3F           # every bit in range of a last word, padding clear
    pre[1::2, ::3, 2] = 0xFFFFFFC0    # only padding bits (a caller's): they stay, nothing in range is skipped
    pre[0, 0, :] = 0
    for device in (False, True):
        got = observe(eng, origin, dims, [synth_frames[0]], device, pre=pre)
        assert np.array_equal(got, pre | fref.pack(single[0])), device
    assert ((pre | fref.pack(single[0])) != pre).sum() > 100


CULL_MAX_DEPTH = 0.5
CULL_CAMERA_LOCAL = (65, 40, 10)  # the camera centre's voxel in the big box (found by a search over placements)


def cull_frame():
    """A camera for a box it stands in: 80 x 60, turned 41 degrees about a skew axis so that the frustum's planes
    cut obliquely through the bricks' long axis and leave whole bricks on the far side of each, depths 0.3 ..
    0.5 m with holes and pixels beyond max_depth = 0.5, so that the far end of the frustum lies inside the box."""
    import tsdf_amd
    from tsdf_amd import synth
    cam = synth.camera(80, 60)
    axis = np.array([-0.64, -0.12, 0.76])
    axis /= np.linalg.norm(axis)
    half = np.deg2rad(41.0) / 2
    q = np.concatenate([axis * np.sin(half), [np.cos(half)]]).astype(f32)
    rng = np.random.default_rng(9)
    depth = (0.3 + 0.2 * rng.random((60, 80))).astype(f32)
    depth[rng.random((60, 80)) < 0.05] = 0
    depth[rng.random((60, 80)) < 0.05] = 0.8
    centre = np.array([0.31, -0.17, 0.52], f32)  # the camera centre in the world
    t = -tsdf_amd.SE3(q, np.zeros(3, f32)).Apply(centre)
    return fref.frame(depth, cam.K, q, t, CULL_MAX_DEPTH)


def test_culls():
    """The camera inside a 128 x 64 x 64 box: bricks behind the camera plane, outside each side plane, beyond
    max_depth and across each of those surfaces; small boxes wholly inside each culled region; and the same
    calls on an engine created under TSDF_FREE_CULL=0. All equal the restatement."""
    fr = cull_frame()
    big_dims = (128, 64, 64)
    big_origin = (in_front(fr, (0, 0, 0)) - np.array(CULL_CAMERA_LOCAL)).tolist()
    want = fref.frame_mask(big_origin, big_dims, fr, VOXEL, TRUNC)
    T = fref.terms(fref.box_points(big_origin, big_dims), fr, VOXEL, TRUNC)
    with np.errstate(invalid="ignore"):
        regions = dict(behind=T["hz"] <= 0, beyond=T["hz"] >= CULL_MAX_DEPTH, left=(T["hz"] > 0) & (T["uq"] < -1.5),
                       right=(T["hz"] > 0) & (T["uq"] > 80.5), top=(T["hz"] > 0) & (T["vq"] < -1.5),
                       bottom=(T["hz"] > 0) & (T["vq"] > 60.5))
    # whole 64 x 8 x 8 bricks in each region, and bricks a region's surface cuts through
    for name, r in regions.items():
        b = r.reshape(8, 8, 8, 8, 2, 64).transpose(0, 2, 4, 1, 3, 5).reshape(8, 8, 2, -1)
        print(f"culls: {name}: {int(b.all(-1).sum())} bricks inside, {int((b.any(-1) & ~b.all(-1)).sum())} across")
        assert b.all(-1).sum() >= 1 and (b.any(-1) & ~b.all(-1)).sum() >= 1, name
    assert 1000 < want.sum() < want.size // 2
    far = dict(behind=(0, 0, -1.0), beyond=(0, 0, 2.0), left=(-2.0, 0, 0.6), right=(2.0, 0, 0.6), top=(0, -2.0, 0.6),
               bottom=(0, 2.0, 0.6))
    engines = [make_engine(), make_engine(env={"TSDF_FREE_CULL": "0"})]
    try:
        for e, tag in zip(engines, ("culls on", "culls off")):
            check(e, big_origin, big_dims, [fr], tag=tag, want=want)
            for name, p in far.items():
                origin = (in_front(fr, p) - np.array([32, 4, 4])).tolist()
                m = check(e, origin, (64, 8, 8), [fr], tag=f"{tag}, wholly {name}")
                assert not m.any(), name
            assert e.stats()["status"] == 0
    finally:
        for e in engines:
            e.close()


def test_apply(eng):
    """Nested, partly overlapping and disjoint boxes, states 0 / 1 / 2, both memory kinds, with and without the
    count."""
    import torch
    from tsdf_amd import esdf
    rng = np.random.default_rng(11)
    lo, ld = (-9, 4, 17), (70, 9, 11)
    mask = rng.random(ld[::-1]) < 0.5
    cases = [((-5, 5, 18), (40, 7, 9)), ((-20, 1, 12), (45, 9, 9)), ((-9, 4, 17), (70, 9, 11)), ((-30, -2, 10), (130, 20, 25)),
             ((61, 4, 17), (12, 9, 11)), ((-9, 13, 17), (70, 3, 11)), ((30, 8, 20), (1, 1, 1))]
    some = 0
    for origin, dims in cases:
        state = rng.integers(0, 3, dims[::-1]).astype(np.uint8)
        d2 = rng.integers(0, 500, dims[::-1]).astype(np.uint16)
        want, n = fref.apply(mask, lo, state, origin)
        some += n
        for device in (False, True):
            layer = esdf.free_layer(lo, ld, device=device)
            if device:
                layer["bits"].copy_(torch.as_tensor(fref.pack(mask).view(np.int32), device=layer["bits"].device))
                field = dict(d2=torch.as_tensor(d2, device=layer["bits"].device),
                             state=torch.as_tensor(state, device=layer["bits"].device), origin=origin, dims=dims)
            else:
                layer["bits"][:] = fref.pack(mask)
                field = dict(d2=d2, state=state, origin=origin, dims=dims)
            for count in (True, False):
                out = eng.free_apply(layer, field, count=count)
                got = out["state"].cpu().numpy() if device else out["state"]
                print(f"apply {origin} + {dims} device={device} count={count}: promoted {out['promoted']} (want {n}), "
                      f"differs at {int((got != want).sum())}")
                assert out["promoted"] == (n if count else None)
                assert np.array_equal(got, want)
                assert out["d2"] is field["d2"] and out["origin"] == origin and out["dims"] == dims
                # the input is left as it was
                assert np.array_equal(field["state"].cpu().numpy() if device else field["state"], state)
                assert np.array_equal(field["d2"].cpu().numpy() if device else field["d2"], d2)
            assert np.array_equal(words(layer), fref.pack(mask))
    assert some > 2000 and fref.apply(mask, lo, np.zeros((11, 9, 12), np.uint8), (61, 4, 17))[1] == 0
    assert eng.stats()["status"] == 0


def test_arguments(eng, synth_frames):
    import tsdf_amd
    lib = tsdf_amd._lib
    L = lib.load()
    fr = synth_frames[0]
    depth = fr["depth"]
    K = lib.Intrinsics(*[float(v) for v in fr["K"]])
    P = pose_of(fr)._c()
    org = in_front(fr, (0, 0, 0.9)).tolist()

    def ocall(h=0, origin=org, dims=(40, 4, 4), boxp=True, bitsp=True, depthp=True, w=80, hh=60, kind=0, Kp=True, Pp=True,
              max_depth=4.0):
        bits = np.full(4 * 4 * 2, 0x0F0F0F0F, np.uint32)
        box = lib.FreeBox((C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*dims))
        rc = L.tsdf_free_observe(eng._h if h == 0 else h, C.byref(box) if boxp else None, bits.ctypes.data if bitsp else None,
                                 depth.ctypes.data if depthp else None, w, hh, kind, C.byref(K) if Kp else None,
                                 C.byref(P) if Pp else None, max_depth)
        return rc, bool((bits == 0x0F0F0F0F).all())

    assert ocall() == (0, False)
    bad = [dict(dims=(0, 4, 4)), dict(dims=(40, 2049, 4)), dict(dims=(40, 4, -1)), dict(dims=(2048, 2048, 65)),
           dict(origin=(262144 - 39, 0, 0)), dict(origin=(0, -262145, 0)), dict(boxp=False), dict(bitsp=False),
           dict(depthp=False), dict(w=0), dict(w=81), dict(hh=0), dict(hh=61), dict(kind=2), dict(kind=-1), dict(Kp=False),
           dict(Pp=False), dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=float("nan")), dict(h=None)]
    for kw in bad:
        assert ocall(**kw) == (TSDF_ERR_INVALID_ARG, True), kw
    assert ocall(origin=(262144 - 40, -262144, 0))[0] == 0  # the last and the first block of the range

    lbits = np.full(4 * 4 * 2, 0xFFFFFFFF, np.uint32)

    def acall(h=0, lorigin=(0, 0, 0), ldims=(40, 4, 4), boxp=True, bitsp=True, origin=(0, 0, 0), dims=(8, 4, 4), originp=True,
              dimsp=True, statep=True, kind=0):
        state = np.zeros(8 * 4 * 4, np.uint8)
        box = lib.FreeBox((C.c_int32 * 3)(*lorigin), (C.c_int32 * 3)(*ldims))
        n = C.c_int64(-7)
        rc = L.tsdf_free_apply(eng._h if h == 0 else h, C.byref(box) if boxp else None, lbits.ctypes.data if bitsp else None,
                               (C.c_int32 * 3)(*origin) if originp else None, (C.c_int32 * 3)(*dims) if dimsp else None,
                               state.ctypes.data if statep else None, kind, C.byref(n))
        return rc, bool((state == 0).all()) and n.value == -7

    assert acall() == (0, False)
    bad = [dict(ldims=(0, 4, 4)), dict(ldims=(40, 4, 2049)), dict(lorigin=(262144, 0, 0)), dict(boxp=False), dict(bitsp=False),
           dict(dims=(0, 4, 4)), dict(dims=(8, -4, 4)), dict(dims=(2048, 2048, 65)), dict(origin=(0, 0, -262145)),
           dict(origin=(0, 262144 - 3, 0)), dict(originp=False), dict(dimsp=False), dict(statep=False), dict(kind=2),
           dict(h=None)]
    for kw in bad:
        assert acall(**kw) == (TSDF_ERR_INVALID_ARG, True), kw
    from tsdf_amd import esdf
    with pytest.raises(lib.TSDFError, match="invalid argument"):
        eng.free_observe(esdf.free_layer(org, (40, 4, 4)), depth, fr["K"], pose_of(fr), 0.0)
    with pytest.raises(ValueError):
        eng.free_observe(dict(bits=np.zeros((4, 4, 1), np.uint32), origin=org, dims=(40, 4, 4)), depth, fr["K"], pose_of(fr), 4.0)
    with pytest.raises(ValueError):
        eng.free_apply(esdf.free_layer(org, (40, 4, 4)), dict(d2=None, state=None, origin=org, dims=(4, 4, 4)))
    assert eng.stats()["status"] == 0


def test_shard_engine(synth_frames):
    """The calls do not touch the volume: a shard engine serves as well as any other."""
    fr = synth_frames[1]
    origin = (in_front(fr, (0, 0, 1.0)) - np.array([33, 5, 4])).tolist()
    shard = make_engine(shard_index=1, shard_count=2)
    try:
        m = check(shard, origin, (67, 10, 9), [fr], tag="shard")
        assert m.sum() > 500
        state = np.zeros((9, 10, 67), np.uint8)
        from tsdf_amd import esdf
        layer = esdf.free_layer(origin, (67, 10, 9))
        layer["bits"][:] = fref.pack(m)
        out = shard.free_apply(layer, dict(d2=None, state=state, origin=origin, dims=(67, 10, 9)))
        assert out["promoted"] == int(m.sum()) and np.array_equal(out["state"] == 1, m)
    finally:
        shard.close()


def test_pending_frames_stay_as_they_were():
    """Frames integrated back to back from device memory, an observe of each frame's own device depth between
    them: the volume ends bit-identical to that of an engine that never called it, with the same number of
    pipelined launches."""
    import torch
    import tsdf_amd
    from tsdf_amd import esdf, synth
    cam = synth.camera(80, 60)
    frames = [synth.render(cam, k) for k in range(5)]
    origin = (in_front(fref.frame(frames[0]["depth"], cam.K, frames[0]["q"], frames[0]["t"], 4.0), (0, 0, 2.3), 0.005)
              - np.array([48, 20, 12])).tolist()
    dims = (96, 40, 24)
    want = np.zeros(dims[::-1], bool)
    for s in frames:
        want |= fref.frame_mask(origin, dims, fref.frame(s["depth"], cam.K, s["q"], s["t"], 4.0), 0.005, 0.03)
    dumps, pipelined = [], []
    for with_call in (True, False):
        e = make_engine(0.005, 0.03, env={"TSDF_PIPELINE": "1"}, nb_bits=14)
        try:
            layer = esdf.free_layer(origin, dims, device=True)
            keep = []
            e.profile_begin()
            for s in frames:
                dev = [None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")
                       for a in (s["rgb"], s["depth"], s["ht"], s["lt"])]
                keep.append(dev)
                pose = tsdf_amd.SE3(s["q"], s["t"])
                e.integrate(*dev, cam.K, pose, 4.0)
                if with_call:
                    e.free_observe(layer, dev[1], cam.K, pose, 4.0)
            e.synchronize()
            pipelined.append(e.profile_end()["pipelined"])
            dumps.append((e.dump(), e.stats()))
            if with_call:
                got = words(layer)
                print(f"pending: free {int(want.sum())}, differs at {int((fref.unpack(got, dims[0]) != want).sum())}")
                assert want.sum() > 10000 and np.array_equal(got, fref.pack(want))
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


def test_scenario_end_to_end():
    """The wall with a gap through the engine, device arrays from the distance field to the travel field: the
    volume alone does not start, the optimistic field leaks, the promoted field floods the room and stays in it."""
    import tsdf_amd
    from tsdf_amd import esdf
    s = fc.scenario()
    depth = fc.scenario_depth()
    seed = np.array(fc.S_SEED_LOCAL) + np.array(fc.S_ORIGIN)
    e = tsdf_amd.Engine(fc.S_VOXEL, fc.S_TRUNC, max_width=fc.S_W, max_height=fc.S_H, num_block_bits=fc.S_NB_BITS)
    try:
        pose = tsdf_amd.SE3(fc.S_Q, fc.S_T)
        for _ in range(3):
            e.integrate(np.zeros((fc.S_H, fc.S_W, 3), np.uint8), depth, None, None, fc.S_K, pose, fc.S_MAX_DEPTH)
        field = e.distance_field(fc.S_ORIGIN, fc.S_DIMS, max_dist=fc.S_MAX_DIST, device=True)
        assert np.array_equal(field["d2"].cpu().numpy(), s["field"]["d2"])
        assert np.array_equal(field["state"].cpu().numpy(), s["field"]["state"])
        layer = esdf.free_layer(fc.S_ORIGIN, fc.S_DIMS, device=True)
        e.free_observe(layer, depth, fc.S_K, pose, fc.S_MAX_DEPTH)
        assert np.array_equal(esdf.free_mask(layer), s["mask"]) and esdf.free_fraction(layer) == s["mask"].mean()
        promoted = e.free_apply(layer, field)
        assert promoted["state"].is_cuda and promoted["d2"] is field["d2"]
        assert promoted["promoted"] == s["promoted"][1] == 44832
        assert np.array_equal(promoted["state"].cpu().numpy(), s["promoted"][0])
        for name, f, unknown_free in (("volume_strict", field, False), ("volume_optimistic", field, True),
                                      ("promoted", promoted, False)):
            got = e.travel_field(f, [seed], fc.S_CLEARANCE2, unknown_free, device=True)
            cost = got["cost"].cpu().numpy()
            print(f"scenario {name}: seeded {got['seeded']}, (reached, behind the wall, largest cost) {fc.reached(cost)}")
            assert got["cost"].is_cuda and got["seeded"] == s["cost"][name][1]
            assert np.array_equal(cost, s["cost"][name][0])
        assert s["cost"]["volume_strict"][1] == 0 and fc.reached(s["cost"]["volume_optimistic"][0])[1] > 0
        assert fc.reached(s["cost"]["promoted"][0]) == (50766, 0, 187)
        assert e.stats()["status"] == 0
    finally:
        e.close()


def test_facade(tmp_path):
    """DISINFSystem::enable_free_space, frames, query_free_space and query_travel_field(unknown_free = false)
    (free_main) on the scenario: the counts it prints and the arrays it writes."""
    s = fc.scenario()
    v = fc.S_VOXEL
    lo = [(fc.S_ORIGIN[a] - 0.3) * v for a in range(3)]
    hi = [(fc.S_ORIGIN[a] + fc.S_DIMS[a] - 1 + 0.3) * v for a in range(3)]
    cube = " ".join(f"{lo[a]:.6f} {hi[a]:.6f}" for a in range(3))
    frm = " ".join(f"{(fc.S_SEED_LOCAL[a] + fc.S_ORIGIN[a]) * v:.6f}" for a in range(3))
    k = " ".join(str(float(x)) for x in fc.S_K)
    (tmp_path / "meta.txt").write_text(f"{v} {fc.S_TRUNC} {fc.S_NB_BITS} {fc.S_MAX_DEPTH} {fc.S_W} {fc.S_H} {k} 3 {cube} {cube} "
                                       f"{fc.S_MAX_DIST} 0.0199 {frm}\n")
    fc.scenario_depth().tofile(tmp_path / "depth.bin")
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print("free_main:", r.stdout.strip())
    out = [int(x) for x in r.stdout.split()]
    want_cost = s["cost"]["promoted"][0]
    assert out == [*fc.S_ORIGIN, *fc.S_DIMS, 2, int(s["mask"].sum()), s["promoted"][1], 0, 1, fc.reached(want_cost)[0]]
    assert np.array_equal(np.fromfile(tmp_path / "out_state.bin", np.uint8).reshape(fc.S_DIMS[::-1]), s["promoted"][0])
    assert np.array_equal(np.fromfile(tmp_path / "out_cost.bin", np.uint32).reshape(fc.S_DIMS[::-1]), want_cost)
    bits = np.fromfile(tmp_path / "out_bits.bin", np.uint32).reshape(fc.S_DIMS[2], fc.S_DIMS[1], -1)
    assert np.array_equal(bits, fref.pack(s["mask"]))
