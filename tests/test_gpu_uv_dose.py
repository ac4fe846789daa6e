"""UV dose on surface points (tsdf_surface_normals / tsdf_uv_dose) against tests/_uv_ref.py, the numpy
restatement of the contract, bit for bit; against geometry and the analytic law; and through the facade.

The volume is analytic and imported as block records (no frames): 1 cm voxels, 4 cm truncation, 2^13
blocks. The signed distance is the minimum of a floor whose zero crossing is at voxel z = -7.5 and a box
x, y in [-4.5, 3.5], z in [-7.5, 8.5] (voxels), sampled in the voxel cube x, y in [-32, 32), z in [-16, 32):
voxels with |sd| <= 4 cm hold clip(sd / 0.04, -1, 1) and weight 10, every other voxel of a block that holds
such a voxel tsdf 1 and weight 0, and no other block exists. prob is 0.9 on box voxels, 0.2 on floor voxels.
Emitter A is 10 J at (-0.22, 0, 0.24) m."""
import os
import subprocess

import numpy as np
import pytest

import _uv_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "dose_main")
VOXEL, TRUNC, NB_BITS = 0.01, 0.04, 13
f32 = np.float32
BOX_LO, BOX_HI = np.array([-4.5, -4.5, -7.5]), np.array([3.5, 3.5, 8.5])
FLOOR_Z = -7.5
A = np.array([[-0.22, 0.0, 0.24, 10.0]], f32)
FAR = np.array([[0.0, 0.0, 6.0, 10.0]], f32)      # out of range (max_range 5)
BELOW = np.array([[0.1, 0.1, -0.5, 10.0]], f32)   # under the floor: c <= 0 for a receiver facing up
TSDF_ERR_INVALID_ARG = 1


def box_sd(g):
    """Signed distance [voxels] of points g (..., 3) to the box."""
    q = np.abs(g - (BOX_LO + BOX_HI) / 2) - (BOX_HI - BOX_LO) / 2
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(axis=-1), 0)


def scene_records():
    x, y, z = np.meshgrid(np.arange(-32, 32), np.arange(-32, 32), np.arange(-16, 32), indexing="ij")
    g = np.stack([x, y, z], -1).astype(np.float64)
    sb, sf = box_sd(g), g[..., 2] - FLOOR_Z
    sd = np.minimum(sb, sf) * VOXEL
    near = np.abs(sd) <= TRUNC
    tsdf = np.where(near, np.clip(sd / TRUNC, -1, 1), 1.0).astype(f32)
    prob = np.where(sb <= sf, 0.9, 0.2).astype(f32)
    recs = []
    for bx in range(-4, 4):
        for by in range(-4, 4):
            for bz in range(-2, 4):
                sl = (slice(8 * bx + 32, 8 * bx + 40), slice(8 * by + 32, 8 * by + 40), slice(8 * bz + 16, 8 * bz + 24))
                if not near[sl].any():
                    continue
                rec = np.zeros(6160, np.uint8)
                rec[:8].view(np.int16)[:3] = (bx, by, bz)
                # voxel offset x + 8 y + 64 z: (z, y, x) order in memory
                rec[16:16 + 2048].view(f32)[:] = tsdf[sl].transpose(2, 1, 0).reshape(-1)
                rec[16 + 2048:16 + 4096].view(f32)[:] = prob[sl].transpose(2, 1, 0).reshape(-1)
                rgbw = np.zeros((512, 4), np.uint8)
                rgbw[:, :3] = 128
                rgbw[:, 3] = np.where(near[sl].transpose(2, 1, 0).reshape(-1), 10, 0)
                rec[16 + 4096:].reshape(512, 4)[:] = rgbw
                recs.append(rec)
    return np.stack(recs)


@pytest.fixture(scope="module")
def scene():
    """The engine holding the volume, its dump, the floor receivers and their reference doses."""
    # torch's HIP runtime first (conftest._torch_hip_first runs after module fixtures)
    import torch
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")
    import tsdf_amd
    recs = scene_records()
    assert 120 <= recs.shape[0] <= 150, recs.shape  # (about 136 blocks)
    eng = tsdf_amd.Engine(VOXEL, TRUNC, max_width=64, max_height=64, num_block_bits=NB_BITS)
    eng.import_blocks(recs, replace=True)
    dump = eng.dump()
    i, j = np.meshgrid(np.arange(-30, 30), np.arange(-30, 30), indexing="ij")
    vox = np.stack([i + 0.25, j + 0.25, np.full(i.shape, FLOOR_Z)], -1).reshape(-1, 3)
    pts = (vox.astype(f32) * f32(VOXEL)).astype(f32)
    nrm = np.tile(np.array([0, 0, 1], f32), (pts.shape[0], 1))
    em3 = np.concatenate([A, FAR, BELOW])
    ref3, counted3, _ = _uv_ref.dose(dump, pts, nrm, em3, VOXEL)
    refA, countedA, visA = _uv_ref.dose(dump, pts, nrm, A, VOXEL)
    s = dict(eng=eng, recs=recs, dump=dump, pts=pts, nrm=nrm, em3=em3, ref3=ref3, counted3=counted3, refA=refA,
             countedA=countedA, visA=visA)
    yield s
    eng.close()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def test_restatement(scene):
    eng, pts, nrm, em3, ref3 = (scene[k] for k in ("eng", "pts", "nrm", "em3", "ref3"))
    assert pts.shape[0] == 3600
    # the second and third emitter count nowhere, the first somewhere
    assert scene["counted3"][:, 0].any() and not scene["counted3"][:, 1:].any()
    got = eng.uv_dose(pts, nrm, em3)
    print("restatement: max |got - ref| =", np.abs(got - ref3).max(), "nonzero", np.count_nonzero(ref3))
    assert np.count_nonzero(ref3) > 2000
    assert same(got, ref3)
    assert same(eng.uv_dose(pts, nrm, em3, use_grid=0), ref3)
    import torch
    dev = eng.uv_dose(torch.as_tensor(pts, device="cuda"), torch.as_tensor(nrm, device="cuda"), em3, device=True)
    assert dev.is_cuda and same(dev.cpu().numpy(), ref3)
    for sl in (slice(1234, 1235), slice(700, 767)):
        assert same(eng.uv_dose(pts[sl], nrm[sl], em3), ref3[sl])


def segment_hits_box(o, e, lo, hi):
    """Whether the segments o[i] -> e meet the box [lo, hi] (float64 slabs)."""
    d = e[None, :] - o
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
    par = d == 0  # parallel to a slab: inside it or never
    inside = (o >= lo) & (o <= hi)
    tn = np.where(par, np.where(inside, -np.inf, np.inf), tn)
    tf = np.where(par, np.where(inside, np.inf, -np.inf), tf)
    return np.maximum(tn.max(axis=1), 0.0) <= np.minimum(tf.min(axis=1), 1.0)


def test_geometry(scene):
    """Shadows against the box's geometric shadow, lit doses against E cos(theta) / (4 pi r^2) in float64.
    (A numpy prototype of the contract on this scene found 398 of the 3600 receivers shadowed and a lit
    dose within 3e-7 of the analytic value.)"""
    eng, pts, nrm = scene["eng"], scene["pts"], scene["nrm"]
    got = eng.uv_dose(pts, nrm, A)
    assert same(got, scene["refA"])
    assert scene["countedA"].all()  # every receiver is in range of A and faces it
    shadowed = got == 0
    p = pts.astype(np.float64) / VOXEL
    o = p + np.array([0, 0, 2.0])  # the ray origins: bias = 2 voxels along the normal
    e = A[0, :3].astype(np.float64) / VOXEL
    under = np.all((p[:, :2] >= BOX_LO[:2] - 1.5) & (p[:, :2] <= BOX_HI[:2] + 1.5), axis=1)
    in_dilated = segment_hits_box(o, e, BOX_LO - 1.5, BOX_HI + 1.5)
    in_eroded = segment_hits_box(o, e, BOX_LO + 1.5, BOX_HI - 1.5)
    print("geometry: shadowed", shadowed.sum(), "of", shadowed.size, "under the box", under.sum())
    assert not (shadowed & ~in_dilated & ~under).any()
    assert not (~shadowed & in_eroded).any()
    assert 0.05 <= shadowed.mean() <= 0.20
    lit = ~shadowed
    d = A[0, :3].astype(np.float64) - pts.astype(np.float64)
    r2 = (d * d).sum(axis=1)
    want = 10.0 * (d[:, 2] / np.sqrt(r2)) / (4 * np.pi * r2)
    err = np.abs(got[lit] - want[lit]) / want[lit]
    print("geometry: max relative error of a lit dose", err.max())
    assert err.max() <= 1e-5


def test_accumulation_and_edges(scene):
    import tsdf_amd
    eng, pts, nrm, dump = scene["eng"], scene["pts"], scene["nrm"], scene["dump"]
    X = np.array([[-0.22, 0.0, 0.24, 10.0], [0.2, 0.15, 0.3, 4.0]], f32)
    Y = np.array([[0.0, -0.25, 0.2, 7.0]], f32)
    dx, dy = eng.uv_dose(pts, nrm, X), eng.uv_dose(pts, nrm, Y)
    d = eng.uv_dose(pts, nrm, X)
    d2 = eng.uv_dose(pts, nrm, Y, dose=d)
    assert d2 is d and same(d, dx + dy) and np.count_nonzero(dy) > 0
    # m = 0 and n = 0 write nothing
    start = np.linspace(-1.0, 1.0, pts.shape[0]).astype(f32)
    start[0] = -0.0
    d = start.copy()
    eng.uv_dose(pts, nrm, np.zeros((0, 4), f32), dose=d)
    assert same(d, start)
    assert eng.uv_dose(pts[:0], nrm[:0], A).shape == (0,)
    assert eng.surface_normals(pts[:0]).shape == (0, 3)
    # a receiver with a zero normal is unchanged
    nz = nrm.copy()
    nz[::3] = 0
    d = start.copy()
    eng.uv_dose(pts, nz, A, dose=d)
    assert same(d[::3], start[::3])
    ref, _, _ = _uv_ref.dose(dump, pts, nz, A, VOXEL, dose0=start)
    assert same(d, ref)
    # refused arguments
    L, lib = tsdf_amd._lib.load(), tsdf_amd._lib
    for bad in (dict(min_range=0.0), dict(min_range=-1.0), dict(max_range=5.0, step=5.0 / 65537)):
        with pytest.raises(lib.TSDFError, match="invalid argument"):
            eng.uv_dose(pts, nrm, A, **bad)
    import ctypes as C
    c = lib.UvConfig()
    L.tsdf_uv_config_default(eng._h, C.byref(c))
    assert (c.bias, c.step) == (f32(2) * f32(VOXEL), f32(VOXEL)) and (c.min_weight, c.use_grid) == (1, 1)
    assert (c.min_range, c.max_range, c.sample_offset) == (f32(0.05), 5.0, 0.0)
    c.min_range = 0.0
    out = np.zeros(1, f32)
    rc = L.tsdf_uv_dose(eng._h, pts.ctypes.data, nrm.ctypes.data, 1, A.ctypes.data, 1, C.byref(c), out.ctypes.data, 0)
    assert rc == TSDF_ERR_INVALID_ARG
    shard = tsdf_amd.Engine(VOXEL, TRUNC, max_width=64, max_height=64, num_block_bits=NB_BITS, shard_index=0,
                            shard_count=2)
    try:
        n3 = np.zeros((1, 3), f32)
        assert L.tsdf_uv_dose(shard._h, pts.ctypes.data, nrm.ctypes.data, 1, A.ctypes.data, 1, None, out.ctypes.data,
                              0) == TSDF_ERR_INVALID_ARG
        assert L.tsdf_surface_normals(shard._h, pts.ctypes.data, 1, 0.0, n3.ctypes.data, 0) == TSDF_ERR_INVALID_ARG
    finally:
        shard.close()
    # the calls only read the volume
    after = eng.dump()
    assert sorted(after) == sorted(dump)
    for k, v in dump.items():
        assert np.array_equal(np.asarray(v), np.asarray(after[k])), k
    assert eng.stats()["status"] == 0


def test_grid_fallback(scene):
    """An emitter at 25 m: the box of the rays is wider than a block grid, the march takes hash lookups."""
    eng, dump = scene["eng"], scene["dump"]
    pts, nrm = scene["pts"][::7], scene["nrm"][::7]
    em = np.array([[-0.5, 0.3, 25.0, 1000.0]], f32)
    ref, counted, vis = _uv_ref.dose(dump, pts, nrm, em, VOXEL, max_range=30.0)
    assert counted.all() and vis.any() and not vis.all()
    got = eng.uv_dose(pts, nrm, em, max_range=30.0)
    assert same(got, ref)


def mesh_vertices(eng):
    m = eng.extract_mesh_indexed()
    return m, m["positions"].astype(np.float64) / VOXEL - 0.5  # voxel coordinates (the mesh's half-voxel shift)


def test_mesh_path(scene):
    """Mesh vertices as receivers (sample_offset 0.5). Floor-top vertices are taken at least 6 voxels from
    the box and, because a voxel of a missing block reads +1, at least 2 voxels inside the rim of the voxel
    cube: there the nearest voxel's x and y differences are exactly 0."""
    eng, dump = scene["eng"], scene["dump"]
    m, v = mesh_vertices(eng)
    pos = m["positions"]
    nrm = eng.surface_normals(pos, 0.5)
    assert same(nrm, _uv_ref.normals(dump, pos, VOXEL, 0.5))
    far = box_sd(v) >= 6
    inner = np.all(np.abs(v[:, :2] + 0.5) <= 29.5, axis=1)
    top = far & inner & (np.abs(v[:, 2] - FLOOR_Z) < 0.01)
    sheet = (v[:, 2] < -10) & (nrm[:, 2] < 0)
    print("mesh path: vertices", pos.shape[0], "floor-top", top.sum(), "under-floor sheet", sheet.sum())
    assert top.sum() > 1000 and sheet.sum() > 1000
    assert np.array_equal(nrm[top], np.tile(np.array([0, 0, 1], f32), (top.sum(), 1)))
    got = eng.uv_dose(pos, nrm, A, sample_offset=0.5)
    ref, _, _ = _uv_ref.dose(dump, pos, nrm, A, VOXEL, sample_offset=0.5)
    assert same(got, ref)
    assert same(eng.uv_dose(pos, None, A, sample_offset=0.5), ref)  # normals=None: surface_normals first
    assert not got[sheet].any()
    lit = top & (got > 0)
    assert lit.sum() > 500
    d = A[0, :3].astype(np.float64) - pos[lit].astype(np.float64)
    r2 = (d * d).sum(axis=1)
    want = 10.0 * (d[:, 2] / np.sqrt(r2)) / (4 * np.pi * r2)
    err = np.abs(got[lit] - want) / want
    print("mesh path: max relative error of a lit floor-top dose", err.max())
    assert err.max() <= 1e-5


def test_facade(scene, tmp_path):
    """DISINFSystem::query_mesh + irradiate (dose_main) on the same records: Python's normals and dose."""
    eng = scene["eng"]
    (tmp_path / "meta.txt").write_text(f"{VOXEL} {TRUNC} {NB_BITS} 1\n")
    scene["recs"].tofile(tmp_path / "blocks.bin")
    A.tofile(tmp_path / "emitters.bin")
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = eng.extract_mesh_indexed()
    n = m["positions"].shape[0]
    assert int((tmp_path / "out_counts.txt").read_text()) == n
    verts = np.fromfile(tmp_path / "out_verts.bin", f32).reshape(n, 3)
    assert same(verts, m["positions"])
    assert np.array_equal(np.fromfile(tmp_path / "out_keys.bin", np.int32).reshape(n, 4), m["keys"])
    nrm = eng.surface_normals(m["positions"], 0.5)
    assert same(np.fromfile(tmp_path / "out_normals.bin", f32).reshape(n, 3), nrm)
    dose = eng.uv_dose(m["positions"], nrm, A, sample_offset=0.5)
    assert np.count_nonzero(dose) > 1000
    assert same(np.fromfile(tmp_path / "out_dose.bin", f32), dose)
