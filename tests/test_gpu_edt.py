"""The Euclidean distance field (tsdf_distance_field) against tests/_edt_ref.py, the numpy restatement of
the contract, byte for byte; against geometry computed directly; across boxes, memory kinds and scratch
growth; its refused arguments; and through the facade (edt_main). Every expected value is an integer.

The volume is the analytic floor-and-box scene of the UV dose tests, imported as block records (1 cm
voxels, 4 cm truncation, 2^13 blocks, 136 of them allocated): a floor whose zero crossing is at voxel
z = -7.5 and a box x, y in [-4.5, 3.5], z in [-7.5, 8.5], sampled for x, y in [-32, 32), z in [-16, 32).
The figures asserted about it were evaluated with the restatement on the CPU (tests/test_edt_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _edt_ref
from _edt_ref import NB_BITS, TRUNC, VOXEL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "edt_main")
ORIGIN, DIMS = (-37, -35, -21), (77, 70, 59)  # odd, not block aligned, past the volume on every side
TSDF_ERR_INVALID_ARG = 1


def make_engine(recs=None, **kw):
    import tsdf_amd
    eng = tsdf_amd.Engine(VOXEL, TRUNC, max_width=64, max_height=64, num_block_bits=NB_BITS, **kw)
    if recs is not None:
        eng.import_blocks(recs, replace=True)
    return eng


@pytest.fixture(scope="module")
def scene():
    """The engine holding the volume, its dump, and the restatement of the main box (computed once)."""
    # torch's HIP runtime first (conftest._torch_hip_first runs after module fixtures)
    import torch
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    recs = _edt_ref.scene_records()
    assert recs.shape[0] == 136
    eng = make_engine(recs)
    dump = eng.dump()
    state, site = _edt_ref.classes(dump, ORIGIN, DIMS)
    s = dict(eng=eng, recs=recs, dump=dump, state=state, site=site, ref={})
    for R in (255, 6, 5):
        s["ref"][R, False] = _edt_ref.transform(site, R)
    for R in (255, 6):
        s["ref"][R, True] = _edt_ref.transform(site | (state == 0), R)
    yield s
    eng.close()


def sub(a, origin, dims, base=ORIGIN):
    """The part of array a (a box at `base`) that the box (origin, dims) covers."""
    o = [origin[i] - base[i] for i in range(3)]
    return a[o[2]:o[2] + dims[2], o[1]:o[1] + dims[1], o[0]:o[0] + dims[0]]


def test_restatement(scene):
    eng, ref, state, site = scene["eng"], scene["ref"], scene["state"], scene["site"]
    # the case is not trivial
    assert int(site.sum()) == 4516
    assert np.bincount(state.ravel(), minlength=3).tolist() == [281502, 19100, 17408]
    assert int(ref[255, False].max()) == 2098 and not (ref[255, False] == 255 * 255).any()
    assert int((ref[6, False] == 36).sum()) == 257182
    assert int((ref[255, True] == 0).sum()) == 286018 and int(ref[255, True].max()) == 10
    for R in (255, 6):
        for unknown in (False, True):
            f = eng.distance_field(ORIGIN, DIMS, max_dist=R, unknown=unknown)
            assert f["d2"].dtype == np.uint16 and f["d2"].shape == DIMS[::-1] and f["state"].dtype == np.uint8
            assert (f["origin"], f["dims"], f["max_dist"]) == (ORIGIN, DIMS, R)
            print(f"restatement R={R} unknown={unknown}: d2 differs at", int((f["d2"] != ref[R, unknown]).sum()),
                  "state differs at", int((f["state"] != state).sum()))
            assert np.array_equal(f["state"], state)
            assert np.array_equal(f["d2"], ref[R, unknown])
    f = eng.distance_field(ORIGIN, DIMS, state=False)
    assert f["state"] is None and np.array_equal(f["d2"], ref[255, False])
    # min_weight above every weight of the volume: nothing observed
    f = eng.distance_field(ORIGIN, DIMS, max_dist=6, min_weight=11)
    assert not f["state"].any() and (f["d2"] == 36).all()
    assert eng.stats()["status"] == 0


def test_geometry(scene):
    """Above the floor, far from the box: the distance to the floor's top layer of inside voxels (z = -8)."""
    f = scene["eng"].distance_field(ORIGIN, DIMS)
    x, y = -20 - ORIGIN[0], -20 - ORIGIN[1]
    z0 = -ORIGIN[2]
    assert f["d2"][z0 - 8:z0 + 4, y, x].tolist() == [k * k for k in range(12)]
    assert f["state"][z0 - 10:z0, y, x].tolist() == [2, 2, 2, 1, 1, 1, 1, 0, 0, 0]


def direct(origin, dims, sites, R):
    """min(R^2, min over the sites of |v - s|^2), computed directly."""
    z, y, x = np.meshgrid(*(np.arange(origin[a], origin[a] + dims[a], dtype=np.int64) for a in (2, 1, 0)), indexing="ij")
    d = np.full(z.shape, R * R, np.int64)
    for s in sites:
        d = np.minimum(d, (x - s[0]) ** 2 + (y - s[1]) ** 2 + (z - s[2]) ** 2)
    return d.astype(np.uint16)


def test_single_sites():
    """One site in a corner region of a 120 x 90 x 70 box, then two at opposite corners: the longest
    windows of a pass, nothing to leave early for."""
    origin, dims = (-2, -3, -1), (120, 90, 70)
    a, b = (3, 3, 3), (115, 83, 67)
    for sites in ((a,), (a, b)):
        eng = make_engine(_edt_ref.site_records(sites))
        try:
            for R in (255, 50):
                f = eng.distance_field(origin, dims, max_dist=R)
                want = direct(origin, dims, sites, R)
                print(f"single sites {len(sites)} R={R}: differs at", int((f["d2"] != want).sum()), "max", int(want.max()))
                assert np.array_equal(f["d2"], want)
                assert int((f["state"] == 2).sum()) == len(sites) and int((f["state"] == 1).sum()) == 6 * len(sites)
            assert int(direct(origin, dims, sites, 255).max()) > 100 * 100
        finally:
            eng.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_long_lines(scene, axis):
    """A line longer than any workgroup tile through the scene, with distances beyond R."""
    eng, dump = scene["eng"], scene["dump"]
    origin, dims = [((-300, 0, 0), (700, 2, 3)), ((0, -300, 0), (2, 700, 3)), ((0, 0, -300), (3, 2, 700))][axis]
    want = _edt_ref.distance_field(dump, origin, dims)
    if axis == 0:
        assert int(want["site"].sum()) == 12 and int((want["d2"] == 255 * 255).sum()) == 1104
    assert want["site"].any() and (want["d2"] == 255 * 255).any()
    f = eng.distance_field(origin, dims)
    print(f"long line axis {axis}: differs at", int((f["d2"] != want["d2"]).sum()))
    assert np.array_equal(f["d2"], want["d2"]) and np.array_equal(f["state"], want["state"])
    want = _edt_ref.transform(want["site"], 100)
    assert np.array_equal(eng.distance_field(origin, dims, max_dist=100)["d2"], want)


def test_box_independence(scene):
    eng, ref, state = scene["eng"], scene["ref"], scene["state"]
    so, sd = (-20, -18, -12), (33, 29, 21)
    f = eng.distance_field(so, sd, max_dist=5)
    assert np.array_equal(f["state"], sub(state, so, sd))
    inner = (slice(5, -5),) * 3
    assert np.array_equal(f["d2"][inner], sub(ref[5, False], so, sd)[inner])
    assert (f["d2"][inner] < 25).any() and (f["d2"][inner] == 25).any()
    # a box whose top face is the floor's top inside layer (z = -8), the free neighbours above outside it, and
    # whose side faces cut through the floor: the neighbours come from the volume
    co, cd = (-20, -18, -12), (33, 29, 5)
    c = eng.distance_field(co, cd, max_dist=5)
    assert np.array_equal(c["state"], sub(state, co, cd))
    site = sub(scene["site"], co, cd)
    assert site[-1].sum() > 800 and not site[:-1].any() and np.array_equal(c["d2"] == 0, site)
    assert np.array_equal(c["d2"], _edt_ref.transform(site, 5))


def test_empty_and_tiny(scene):
    eng = scene["eng"]
    f = eng.distance_field((200, 200, 200), (19, 9, 11), max_dist=7)
    assert (f["d2"] == 49).all() and not f["state"].any()
    f = eng.distance_field((200, 200, 200), (19, 9, 11), max_dist=7, unknown=True)
    assert not f["d2"].any() and not f["state"].any()
    on = np.argwhere(scene["site"])[1234][::-1] + np.array(ORIGIN)
    f = eng.distance_field(tuple(on), (1, 1, 1))
    assert f["d2"].tolist() == [[[0]]] and f["state"].tolist() == [[[2]]]
    f = eng.distance_field((-20, -20, 0), (1, 1, 1))
    assert f["d2"].tolist() == [[[255 * 255]]] and f["state"].tolist() == [[[0]]]
    f = eng.distance_field((-20, -20, -5), (1, 1, 1), max_dist=9)
    assert f["d2"].tolist() == [[[81]]] and f["state"].tolist() == [[[1]]]


def test_fused_frames():
    """Three fused frames and no synchronisation: the call completes the pending pipelined frame. The box
    is around the surface the middle of the last frame sees, 111 voxels per axis at most."""
    import tsdf_amd
    from tsdf_amd import esdf, synth
    voxel = 0.005
    cam = synth.camera(160, 120)
    eng = tsdf_amd.Engine(voxel_size=voxel, truncation=0.03, max_width=160, max_height=120, num_block_bits=14)
    try:
        for k in range(3):
            fr = synth.render(cam, k)
            eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, tsdf_amd.SE3(fr["q"], fr["t"]), 4.0)
        (R_wc, p_wc), _ = synth.pose(2)
        v, u = np.meshgrid(np.arange(48, 72), np.arange(64, 96), indexing="ij")
        z = fr["depth"][v, u].astype(np.float64)
        pc = np.stack([(u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z], -1)[z > 0]
        origin, dims = esdf.box_around(pc @ R_wc.T + p_wc, voxel, 0.1)
        dims = tuple(min(d, 111) for d in dims)
        f = eng.distance_field(origin, dims, max_dist=40)
        want = _edt_ref.distance_field(eng.dump(), origin, dims, max_dist=40)
        print("fused: box", origin, dims, "sites", int(want["site"].sum()), "d2 differs at",
              int((f["d2"] != want["d2"]).sum()), "at the cap", int((want["d2"] == 1600).sum()))
        assert int(want["site"].sum()) > 1000
        assert np.array_equal(f["state"], want["state"])
        assert np.array_equal(f["d2"], want["d2"])
        assert eng.stats()["status"] == 0
    finally:
        eng.close()


def test_memory_kinds_and_scratch(scene):
    import torch
    recs, ref, state = scene["recs"], scene["ref"], scene["state"]
    eng = make_engine(recs)  # (a fresh engine: its scratch starts empty)
    so, sd = (-20, -18, -12), (33, 29, 21)
    bo, bd = (-60, -45, -30), (120, 90, 70)
    small = eng.distance_field(so, sd, max_dist=6)
    assert np.array_equal(small["state"], sub(state, so, sd))
    big = eng.distance_field(bo, bd)
    assert np.array_equal(sub(big["state"], ORIGIN, DIMS, bo), state)
    assert np.array_equal(sub(big["d2"], (-20, -20, -8), (1, 1, 12), bo).ravel(), [k * k for k in range(12)])
    again = eng.distance_field(so, sd, max_dist=6)
    assert np.array_equal(again["d2"], small["d2"]) and np.array_equal(again["state"], small["state"])
    dev = eng.distance_field(bo, bd, device=True)
    assert dev["d2"].is_cuda and dev["d2"].dtype == torch.uint16 and dev["state"].dtype == torch.uint8
    assert np.array_equal(dev["d2"].cpu().numpy(), big["d2"]) and np.array_equal(dev["state"].cpu().numpy(), big["state"])
    dev = eng.distance_field(ORIGIN, DIMS, max_dist=6, unknown=True, state=False, device=True)
    assert dev["state"] is None and np.array_equal(dev["d2"].cpu().numpy(), ref[6, True])
    assert eng.stats()["status"] == 0
    eng.close()


def test_arguments(scene):
    import tsdf_amd
    eng, lib = scene["eng"], tsdf_amd._lib
    L = lib.load()
    c = lib.EdtConfig()
    L.tsdf_edt_config_default(C.byref(c))
    assert (c.max_dist, c.min_weight, c.sites) == (255, 1, 1) and list(c.origin) + list(c.dims) == [0] * 6

    def call(h=None, d2=True, **kw):
        c = lib.EdtConfig()
        L.tsdf_edt_config_default(C.byref(c))
        c.dims = (C.c_int32 * 3)(3, 3, 3)
        for k, v in kw.items():
            setattr(c, k, (C.c_int32 * 3)(*v) if k in ("origin", "dims") else v)
        a, b = np.full(27, 0xABCD, np.uint16), np.full(27, 0xEE, np.uint8)
        out = lib.EdtOut(a.ctypes.data if d2 else None, b.ctypes.data, 0)
        rc = L.tsdf_distance_field(h or eng._h, C.byref(c), C.byref(out))
        return rc, bool((a == 0xABCD).all() and (b == 0xEE).all())

    assert call() == (0, False)
    bad = [dict(dims=(0, 3, 3)), dict(dims=(3, 2049, 3)), dict(dims=(3, 3, -1)), dict(dims=(2048, 2048, 65)),
           dict(max_dist=0), dict(max_dist=256), dict(sites=0), dict(sites=2), dict(sites=4), dict(min_weight=-1),
           dict(d2=False), dict(origin=(32767 * 8 + 6, 0, 0)), dict(origin=(0, -32768 * 8, 0)),
           dict(origin=(0, 0, 2 ** 31 - 2))]
    for kw in bad:
        assert call(**kw) == (TSDF_ERR_INVALID_ARG, True), kw
    assert call(origin=(32767 * 8 + 4, 0, 0))[0] == 0 and call(origin=(0, -32768 * 8 + 1, 0))[0] == 0
    with pytest.raises(lib.TSDFError, match="invalid argument"):
        eng.distance_field((0, 0, 0), (2048, 2048, 65))
    with pytest.raises(lib.TSDFError, match="invalid argument"):
        eng.distance_field((0, 0, 0), (3, 3, 3), max_dist=256)
    shard = make_engine(shard_index=0, shard_count=2)
    try:
        assert call(h=shard._h) == (TSDF_ERR_INVALID_ARG, True)
    finally:
        shard.close()
    # the calls only read the volume
    after = eng.dump()
    for k, v in scene["dump"].items():
        assert np.array_equal(np.asarray(v), np.asarray(after[k])), k
    assert eng.stats()["status"] == 0


def test_facade(scene, tmp_path):
    """DISINFSystem::query_distance_field (edt_main) on the same records: the cube whose voxel centres are
    the main box."""
    lo = [(ORIGIN[a] - 0.3) * VOXEL for a in range(3)]
    hi = [(ORIGIN[a] + DIMS[a] - 1 + 0.3) * VOXEL for a in range(3)]
    cube = " ".join(f"{lo[a]:.6f} {hi[a]:.6f}" for a in range(3))
    (tmp_path / "meta.txt").write_text(f"{VOXEL} {TRUNC} {NB_BITS} 255 1 0 {cube}\n")
    scene["recs"].tofile(tmp_path / "blocks.bin")
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    box = (tmp_path / "out_box.txt").read_text().split()
    assert [int(v) for v in box[:7]] == [*ORIGIN, *DIMS, 255]
    d2 = np.fromfile(tmp_path / "out_d2.bin", np.uint16).reshape(DIMS[::-1])
    st = np.fromfile(tmp_path / "out_state.bin", np.uint8).reshape(DIMS[::-1])
    assert np.array_equal(d2, scene["ref"][255, False]) and np.array_equal(st, scene["state"])
    assert int(box[7]) == int(d2[0, 0, 0]) and float(box[8]) == pytest.approx(np.sqrt(float(d2[0, 0, 0])), rel=1e-5)
