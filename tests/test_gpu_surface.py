"""tsdf_raycast_surface against a numpy float32 restatement of its contract (_track_ref.surface), bit
for bit on every pixel, and against the shaded images of tsdf_raycast.

The scene is test_gpu_mesh_indexed's camera and volume (96x72, 1 cm voxels, 4 cm truncation, 2^13
blocks) with frames 40-43 integrated at their true poses."""
import ctypes as C

import numpy as np
import pytest

import _track_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
MAPS = ("point", "normal", "depth", "prob", "rgbw")


class Scene:
    def __init__(self):
        from tsdf_amd import synth
        self.eng = ref.make_engine()
        self.cam = ref.integrate_frames(self.eng, range(40, 44))
        assert self.eng.stats()["status"] == 0
        self.dump = self.eng.dump()
        # the view of frame 43, and a 50 x 38 view (partial 16 x 16 tiles and waves) from a pose 16
        # frames back along the orbit: part of it looks past what frames 40-43 integrated
        self.views = {"frame43": (self.cam.K, 96, 72, ref.true_pose(43)),
                      "shifted": (synth.camera(50, 38, synth.TUM_FR1).K, 50, 38, ref.true_pose(27))}
        self._ref = {}

    def reference(self, name):
        """(restatement, engine maps, shaded rgba before any surface call ... of this view), once."""
        if name not in self._ref:
            K, w, h, pose = self.views[name]
            rgba, normal = self.eng.raycast(K, w, h, pose, ref.MAX_DEPTH)
            want = ref.surface(self.dump, K, w, h, pose)
            got = self.eng.raycast_surface(K, w, h, pose, ref.MAX_DEPTH)
            self._ref[name] = (want, got, rgba, normal)
        return self._ref[name]


@pytest.fixture(scope="module")
def _holder():
    holder = []
    yield holder
    for s in holder:
        s.eng.close()


@pytest.fixture
def scene(_holder):
    if not _holder:
        _holder.append(Scene())
    return _holder[0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("view", ["frame43", "shifted"])
def test_surface_matches_restatement(scene, view):
    """Every map equals the numpy restatement bit for bit on every pixel; the hit mask is that of
    tsdf_raycast's alpha except pixels with a zero gradient, fewer than 1 % of the hits; the shaded
    images of the view are unchanged by the surface call."""
    want, got, rgba, normal = scene.reference(view)
    K, w, h, pose = scene.views[view]
    alpha = rgba[..., 3] == 255
    hits = int(alpha.sum())
    # the restatement first: its march hits where the shaded image has alpha 255
    assert np.array_equal(want["hit_march"], alpha)
    surf_ref = (want["normal"] != 0).any(axis=-1)
    dropped_ref = int((alpha & ~surf_ref).sum())
    print(f"{view}: {w}x{h}, {want['max_step']} steps, hits {hits} of {w * h}, zero-gradient hits {dropped_ref}")
    assert hits > 0 and not (surf_ref & ~alpha).any()
    assert dropped_ref < 0.01 * hits
    if view == "shifted":
        assert hits < w * h, "every ray of the shifted view hit: it does not look past the volume"
    for k in MAPS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        diff = int((got[k].view(np.uint8) != want[k].view(np.uint8)).reshape(h, w, -1).any(axis=-1).sum())
        assert diff == 0, f"{k}: {diff} pixels differ"
    surf = (got["normal"] != 0).any(axis=-1)
    assert np.array_equal(surf, alpha & surf_ref)
    assert int((alpha & ~surf).sum()) < 0.01 * hits
    # a pixel without a surface holds zeros everywhere; one with a surface a unit normal, a depth in range
    for k in MAPS:
        assert not got[k][~surf].any(), k
    ln = np.linalg.norm(got["normal"][surf].astype(np.float64), axis=-1)
    assert np.abs(ln - 1).max() < 1e-6
    assert (got["depth"][surf] > 0).all() and (got["depth"][surf] <= ref.MAX_DEPTH).all()
    assert got["rgbw"][surf][:, 3].any() and got["prob"][surf].max() > 0
    # the normals face the camera: toward increasing tsdf is toward free space
    P = ref.Camera(K, pose)
    view_dir = got["point"][surf].astype(np.float64) - np.array([float(v) for v in P.wt])
    assert ((got["normal"][surf] * view_dir).sum(axis=-1) < 0).mean() > 0.9
    # the existing images are what they were
    rgba2, normal2 = scene.eng.raycast(K, w, h, pose, ref.MAX_DEPTH)
    assert np.array_equal(rgba2, rgba) and np.array_equal(normal2, normal)


def test_surface_depth_is_the_frame(scene):
    """The surface of frame 43's view lies where frame 43's depth image put it: the median error of
    the raycast depth against the noisy input depth is below one voxel (nearest-voxel sampling moves a
    sample by at most half a voxel diagonal, 8.7 mm)."""
    from tsdf_amd import synth
    _, got, _, _ = scene.reference("frame43")
    d = synth.render(scene.cam, 43)["depth"]
    both = (got["depth"] > 0) & (d > 0)
    err = np.abs(got["depth"][both] - d[both])
    print(f"raycast depth vs frame depth: median {np.median(err) * 1e3:.2f} mm over {both.sum()} pixels")
    assert both.sum() > 0 and np.median(err) < ref.VOXEL


def test_device_maps_equal_host_maps(scene):
    """TSDF_MEM_DEVICE writes the bytes TSDF_MEM_HOST returns, for both views."""
    for view, (K, w, h, pose) in scene.views.items():
        host = scene.reference(view)[1]
        dev = scene.eng.raycast_surface(K, w, h, pose, ref.MAX_DEPTH, device=True)
        assert all(v.is_cuda for v in dev.values())
        for k in MAPS:
            assert same_bits(dev[k].cpu().numpy(), host[k]), (view, k)


def test_null_optional_maps_are_skipped(scene):
    """With depth, prob and rgbw NULL only point and normal are written (host and device forms);
    point or normal NULL is an invalid argument."""
    import torch
    import tsdf_amd
    from tsdf_amd import _lib
    L = tsdf_amd.load_library()
    K, w, h, pose = scene.views["shifted"]
    host = scene.reference("shifted")[1]
    got = scene.eng.raycast_surface(K, w, h, pose, ref.MAX_DEPTH, maps=())
    assert sorted(got) == ["normal", "point"]
    assert same_bits(got["point"], host["point"]) and same_bits(got["normal"], host["normal"])
    got = scene.eng.raycast_surface(K, w, h, pose, ref.MAX_DEPTH, maps=("prob",))
    assert sorted(got) == ["normal", "point", "prob"] and same_bits(got["prob"], host["prob"])
    # device form, through the C ABI: sentinel-filled optional maps that the call is not given stay put
    pt = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    nr = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    dp = torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")
    Kc, Pc = _lib.Intrinsics(*[float(v) for v in K]), pose._c()
    out = _lib.SurfaceOut(C.c_void_p(pt.data_ptr()), C.c_void_p(nr.data_ptr()), None, None, None,
                          tsdf_amd.TSDF_MEM_DEVICE)
    scene.eng._wait_torch(pt, nr, dp)
    assert L.tsdf_raycast_surface(scene.eng._h, C.byref(Kc), w, h, C.byref(Pc), ref.MAX_DEPTH, C.byref(out)) == 0
    scene.eng._signal_torch(pt, nr, dp)
    assert same_bits(pt.cpu().numpy(), host["point"]) and same_bits(nr.cpu().numpy(), host["normal"])
    assert (dp.cpu().numpy() == -7.0).all()
    out.normal = None
    assert L.tsdf_raycast_surface(scene.eng._h, C.byref(Kc), w, h, C.byref(Pc), ref.MAX_DEPTH, C.byref(out)) == 1
    assert L.tsdf_raycast_surface(scene.eng._h, C.byref(Kc), w, h, C.byref(Pc), ref.MAX_DEPTH, None) == 1


def test_shard_engine_is_refused():
    import tsdf_amd
    eng = tsdf_amd.Engine(ref.VOXEL, ref.TRUNC, max_width=64, max_height=64, num_block_bits=10, shard_index=0,
                          shard_count=2)
    try:
        K = np.array([50, 50, 32, 32], f32)
        with pytest.raises(tsdf_amd.TSDFError, match="shard"):
            eng.raycast_surface(K, 64, 64, tsdf_amd.SE3(), 4.0)
    finally:
        eng.close()
