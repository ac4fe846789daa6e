"""Grow-only device scratch (DevBuf, csrc/tsdf_host.h): a request that makes a buffer grow gives the
same bits as the same request on an engine whose buffer starts at that size.

Engine A integrates three frames; engine B is a fresh engine restored from A's snapshot. For each
scratch, A makes a small request and then a larger one, B only the larger one: the two larger results
are equal bit for bit, and the larger request is checked to be larger, so a buffer really grew. The
tests run in file order on the two engines (tk_stage and the view grid are shared by several calls;
each test still grows a buffer of its own).
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 48, 36
VOXEL, TRUNC, NB, MAX_DEPTH = 0.005, 0.03, 14, 4.0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def same(x, y, tag):
    if isinstance(x, dict):
        assert x.keys() == y.keys(), tag
        for k in x:
            same(x[k], y[k], f"{tag}: {k}")
        return
    x, y = np.asarray(x), np.asarray(y)
    assert x.shape == y.shape and x.dtype == y.dtype, tag
    assert np.array_equal(bits(x), bits(y)), f"{tag} differs"


@pytest.fixture(scope="module")
def vol():
    import tsdf_amd
    from tsdf_amd import synth
    cam = synth.camera(W, H)
    kw = dict(voxel_size=VOXEL, truncation=TRUNC, max_width=W, max_height=H, num_block_bits=NB)
    a, b = tsdf_amd.Engine(**kw), tsdf_amd.Engine(**kw)
    frames = [synth.render(cam, f) for f in range(3)]
    for fr in frames:
        a.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, tsdf_amd.SE3(fr["q"], fr["t"]), MAX_DEPTH)
    b.restore(a.snapshot())
    # one live block the surface crosses, found in the dump (tsdf_debug_dump uses no engine scratch)
    d = a.dump(pool=True)
    live = np.flatnonzero(d["entry_idx"] >= 0)
    vox = d["entry_idx"][live][:, None].astype(np.int64) * 512 + np.arange(512)
    seen = d["rgbw"][vox, 3] > 0
    mixed = np.minimum((seen & (d["tsdf"][vox] < 0)).sum(1), (seen & (d["tsdf"][vox] > 0)).sum(1))
    bx, by, bz = (int(v) for v in d["entry_pos"][live[int(np.argmax(mixed))], :3])
    lo = lambda c: (c * 8 - 0.5) * VOXEL
    hi = lambda c: (c * 8 + 7.5) * VOXEL
    cube = tsdf_amd.BoundingCube(lo(bx), hi(bx), lo(by), hi(by), lo(bz), hi(bz))
    # voxel coordinates inside live blocks, for the hash-level hook
    offs = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = (d["entry_pos"][live[:8], :3].astype(np.int32)[:, None, :] * 8 + offs[None]).reshape(-1, 3)
    v = types.SimpleNamespace(a=a, b=b, cam=cam, small_cam=synth.camera(W // 2, H // 2), frames=frames, cube=cube,
                              pts=pts.astype(np.int16), pose=tsdf_amd.SE3(frames[2]["q"], frames[2]["t"]))
    yield v
    assert a.stats()["status"] == 0 and b.stats()["status"] == 0
    a.close()
    b.close()


def grow(v, call, size, tag):
    """A: small(A) then large(A); B: large(B). `size` counts what a result holds."""
    small, large = call(v.a, True), call(v.a, False)
    assert size(large) > size(small) > 0, f"{tag}: {size(small)} then {size(large)}: nothing grows"
    same(large, call(v.b, False), tag)
    assert v.a.stats()["status"] == 0 and v.b.stats()["status"] == 0, tag
    return large


def test_query(vol):
    got = grow(vol, lambda e, small: e.query(vol.cube if small else None), len, "query")
    assert len(vol.a.query(vol.cube)) == 512  # (the bounded request was one block)
    assert len(got) % 512 == 0


def test_extract_mesh(vol):
    grow(vol, lambda e, small: e.extract_mesh(vol.cube if small else None), len, "extract_mesh")


def test_extract_mesh_indexed(vol):
    call = lambda e, small: e.extract_mesh_indexed(vol.cube if small else None)
    small, large = call(vol.a, True), call(vol.a, False)
    for k in ("positions", "indices"):  # more vertices and more triangles
        assert len(large[k]) > len(small[k]) > 0, k
    same(large, call(vol.b, False), "extract_mesh_indexed")


def test_raycast_surface(vol):
    def call(e, small):
        c = vol.small_cam if small else vol.cam
        return e.raycast_surface(c.K, c.width, c.height, vol.pose, MAX_DEPTH)
    got = grow(vol, call, lambda m: m["depth"].size, "raycast_surface")
    assert np.count_nonzero(got["depth"]) > got["depth"].size // 2  # (the maps see the surface)


def test_track(vol):
    from tsdf_amd import synth

    def call(e, small):
        c = vol.small_cam if small else vol.cam
        depth = synth.render(c, 2)["depth"] if small else vol.frames[2]["depth"]
        pose, info = e.track(depth, c.K, vol.pose, MAX_DEPTH)
        return dict(q=np.asarray(pose.q, np.float32), t=np.asarray(pose.t, np.float32),
                    iterations=np.int32(info["iterations"]), inliers=np.int32(info["inliers"]),
                    rmse=np.float32(info["rmse"]), status=np.int32(info["status"]))
    small, large = call(vol.a, True), call(vol.a, False)
    assert large["inliers"] > small["inliers"] > 0 and large["iterations"] > 0
    same(large, call(vol.b, False), "track")


def test_uv_dose(vol):
    c = vol.cam
    maps = vol.a.raycast_surface(c.K, c.width, c.height, vol.pose, MAX_DEPTH, maps=("depth",))
    hit = maps["depth"] > 0
    pts, nrm = maps["point"][hit], maps["normal"][hit]
    centre = vol.pose.Inverse().GetT()  # the camera centre in the world: it sees every receiver
    em = np.zeros((40, 4), np.float32)
    em[:, :3] = centre + 0.01 * np.stack([np.arange(40) % 5, np.arange(40) // 5 % 4, np.arange(40) // 20], 1)
    em[:, 3] = 1.0 + np.arange(40)
    call = lambda e, small: e.uv_dose(pts, nrm, em[:1] if small else em)
    small, large = call(vol.a, True), call(vol.a, False)
    assert len(pts) > 0 and large.sum() > small.sum() > 0  # (40 emitters irradiate more than the first)
    same(large, call(vol.b, False), "uv_dose")


def test_hash_retrieve(vol):
    assert len(vol.pts) >= 2000
    got = grow(vol, lambda e, small: e.hash_retrieve(vol.pts[:8] if small else vol.pts[:2000]),
               lambda r: len(r["tsdf"]), "hash_retrieve")
    assert len(got["tsdf"]) == 2000 > 1024 and np.all(got["block_idx"] >= 0)  # (above the scratch's floor)


def test_rgbd_half(vol):
    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 256, (72, 96, 3), dtype=np.uint8)
    depth = rng.integers(0, 20000, (72, 96), dtype=np.uint16)
    mask = (rng.random((72, 96)) < 0.2).astype(np.uint8)

    def call(e, small):
        s = (slice(0, 24), slice(0, 32)) if small else (slice(None), slice(None))
        r, d = e.rgbd_half(np.ascontiguousarray(rgb[s]), np.ascontiguousarray(depth[s]),
                           np.ascontiguousarray(mask[s]), 5000.0)
        return dict(rgb=r, depth=d)
    grow(vol, call, lambda r: r["depth"].size, "rgbd_half")


def test_render_bands(vol):
    c = vol.cam

    def call(e, small):
        rows = [0, H] if small else [0, 9, 18, 27, H]
        counts, recs = e.render_bands(c.K, c.width, c.height, vol.pose, MAX_DEPTH, rows)
        return dict(counts=counts, records=recs)
    small, large = call(vol.a, True), call(vol.a, False)
    assert len(large["counts"]) == 4 and len(small["counts"]) == 1 and small["counts"][0] > 0
    assert len(large["records"]) >= len(small["records"])  # (a block may lie in several bands)
    same(large, call(vol.b, False), "render_bands")


def test_pack_blocks(vol):
    got = grow(vol, lambda e, small: e.pack_blocks(vol.cube if small else None), len, "pack_blocks")
    assert len(got) == vol.a.stats()["active_blocks"]
