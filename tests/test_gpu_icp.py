"""tsdf_icp_linearize and tsdf_track against numpy restatements (_track_ref), ground truth, and the
C++ facade.

The scene is test_gpu_surface's: test_gpu_mesh_indexed's camera and volume (96x72, 1 cm voxels, 4 cm
truncation, 2^13 blocks) with frames 40-43 integrated at their true poses; frame 44 is tracked."""
import math
import os
import subprocess

import numpy as np
import pytest

import _track_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "track_main")
MAX_DIST = 0.1


class Scene:
    def __init__(self):
        from tsdf_amd import synth
        self.eng = ref.make_engine()
        self.cam = ref.integrate_frames(self.eng, range(40, 44))
        assert self.eng.stats()["status"] == 0
        self.K = self.cam.K
        self.depth44 = synth.render(self.cam, 44)["depth"]  # noisy, quantised, 2 % holes
        # the model of both estimates: the surface seen from frame 43's pose
        self.model_pose = ref.true_pose(43)
        self.model = self.eng.raycast_surface(self.K, 96, 72, self.model_pose, ref.MAX_DEPTH, maps=())
        # a depth frame with zeros (the holes, and a block of them), a NaN and values above max_depth
        d = self.depth44.copy()
        d[10:14, 20:30] = 0.0
        d[30, 40] = np.nan
        d[31, 41] = np.inf
        d[50:52, 60:64] = f32(ref.MAX_DEPTH) + f32(0.5)
        d[52, 60] = np.nextafter(f32(ref.MAX_DEPTH), f32(np.inf))
        self.depth_bad = d
        self._track = {}

    def linearize(self, depth, est, stride):
        return self.eng.icp_linearize(depth, self.K, est, self.model, self.K, self.model_pose, stride, MAX_DIST,
                                      ref.MAX_DEPTH)

    def track(self, guess_frame):
        """(engine result, numpy driver result) of frame 44 from the pose of `guess_frame`, once."""
        if guess_frame not in self._track:
            g = ref.true_pose(guess_frame)
            self._track[guess_frame] = (self.eng.track(self.depth44, self.K, g, ref.MAX_DEPTH),
                                        ref.track(self.eng, self.depth44, self.K, g))
        return self._track[guess_frame]


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


def sums29(res):
    A, b, r2, count = res
    return np.concatenate([A[np.triu_indices(6)], b, [r2, float(count)]])


@pytest.mark.parametrize("stride", [1, 3, 4])
@pytest.mark.parametrize("est_frame", [44, 40])
def test_linearize_matches_restatement(scene, stride, est_frame):
    """count is the restatement's; each other sum is within count * 2^-53 * sum |term| of math.fsum
    over the exact double terms (at most count - 1 additions of non-zero terms, each rounding a
    partial sum that sum |term| bounds). Strides 1 (27 workgroups), 3 (rows that do not fill waves)
    and 4 (a partial second workgroup); a depth frame with zeros, a NaN, an infinity and values above
    max_depth; the estimates are frame 44's true pose and frame 40's."""
    est = ref.true_pose(est_frame)
    got = sums29(scene.linearize(scene.depth_bad, est, stride))
    J, r = ref.icp_terms(scene.depth_bad, scene.K, est, scene.model, scene.K, scene.model_pose, stride, MAX_DIST)
    want, mag = ref.icp_sums_exact(J, r)
    count = int(want[28])
    sampled = len(range(0, 96, stride)) * len(range(0, 72, stride))
    print(f"stride {stride} estimate {est_frame}: {sampled} sampled, {count} kept, rmse "
          f"{math.sqrt(want[27] / max(count, 1)) * 1e3:.2f} mm")
    assert 0 < count <= sampled
    assert int(got[28]) == count and got[28] == float(count)
    bound = count * 2.0 ** -53 * mag[:28]
    err = np.abs(got[:28] - want[:28])
    print(f"  largest error / bound: {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all(), np.flatnonzero(err > bound)
    # the gated pixels are really gated: the clean frame keeps more
    if stride == 1:
        assert sums29(scene.linearize(scene.depth44, est, stride))[28] > count


def test_linearize_is_deterministic_and_device_equals_host(scene):
    """Two calls give the same 29 doubles bit for bit, from host arrays and from device tensors."""
    import torch
    est = ref.true_pose(40)
    for stride in (1, 3):
        a = sums29(scene.linearize(scene.depth_bad, est, stride))
        b = sums29(scene.linearize(scene.depth_bad, est, stride))
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        dev = {k: torch.from_numpy(v).cuda() for k, v in scene.model.items()}
        c = sums29(scene.eng.icp_linearize(torch.from_numpy(scene.depth_bad).cuda(), scene.K, est, dev, scene.K,
                                           scene.model_pose, stride, MAX_DIST, ref.MAX_DEPTH))
        assert np.array_equal(a.view(np.uint64), c.view(np.uint64))


def test_linearize_empty_depth(scene):
    """An all-zero depth frame gives 29 zeros; so does a model without a surface."""
    z = np.zeros((72, 96), f32)
    assert not sums29(scene.linearize(z, ref.true_pose(44), 1)).any()
    empty = {k: np.zeros_like(v) for k, v in scene.model.items()}
    got = scene.eng.icp_linearize(scene.depth44, scene.K, ref.true_pose(44), empty, scene.K, scene.model_pose, 2,
                                  MAX_DIST, ref.MAX_DEPTH)
    assert not sums29(got).any()


def test_linearize_other_model_size(scene):
    """A model map of another size and camera than the depth frame (50 x 38): the restatement's count
    and sums."""
    from tsdf_amd import synth
    Km = synth.camera(50, 38, synth.TUM_FR1).K
    model = scene.eng.raycast_surface(Km, 50, 38, scene.model_pose, ref.MAX_DEPTH, maps=())
    est = ref.true_pose(44)
    got = sums29(scene.eng.icp_linearize(scene.depth44, scene.K, est, model, Km, scene.model_pose, 2, MAX_DIST,
                                         ref.MAX_DEPTH))
    J, r = ref.icp_terms(scene.depth44, scene.K, est, model, Km, scene.model_pose, 2, MAX_DIST)
    want, mag = ref.icp_sums_exact(J, r)
    assert got[28] == want[28] and want[28] > 0
    assert (np.abs(got[:28] - want[:28]) <= want[28] * 2.0 ** -53 * mag[:28]).all()


@pytest.mark.parametrize("guess_frame", [43, 40])
def test_track_matches_restated_loop(scene, guess_frame):
    """tsdf_track against the numpy float64 driver (the same model normals from the surface points, the
    same per-pixel rules and float rounding of the estimate between iterations,
    numpy.linalg.cholesky): within 1e-4 m and 1e-4 rad. While the inlier sets agree the two differ by
    the float rounding of the pose, about 1e-7; one correspondence that flips moves xi by at most about
    max_dist / count."""
    (pose, info), (rpose, rstatus, riters, rinl, rrmse) = scene.track(guess_frame)
    dt, dr = ref.pose_error(pose, rpose)
    print(f"guess {guess_frame}: engine vs numpy loop {dt:.3g} m, {dr:.3g} rad; iterations {info['iterations']}, "
          f"inliers {info['inliers']} / {rinl}, rmse {info['rmse'] * 1e3:.3f} / {rrmse * 1e3:.3f} mm")
    assert info["status"] == 0 and rstatus == 0
    assert info["iterations"] == 19 and riters == 19
    assert dt <= 1e-4 and dr <= 1e-4


def test_track_against_ground_truth(scene):
    """Frame 44 (noisy depth) from pose 43 (10 mm, 0.5 deg off) and from pose 40 (40 mm, 2 deg off):
    within 10 mm (one voxel) and 0.5 deg of synth.pose(44); from pose 40 also within a quarter of the
    guess's error."""
    truth = ref.true_pose(44)
    for guess_frame in (43, 40):
        pose, info = scene.track(guess_frame)[0]
        gt, gr = ref.pose_error(ref.true_pose(guess_frame), truth)
        dt, dr = ref.pose_error(pose, truth)
        print(f"guess {guess_frame}: off {gt * 1e3:.2f} mm {math.degrees(gr):.3f} deg -> "
              f"{dt * 1e3:.3f} mm {math.degrees(dr):.4f} deg ({info})")
        assert info["status"] == 0
        assert dt <= 0.010 and dr <= math.radians(0.5)
        if guess_frame == 40:
            assert dt <= gt / 4 and dr <= gr / 4


def test_track_and_integrate():
    """Frame 40 integrated at its true pose, then frames 41-48 tracked from the previous result and
    integrated at the tracked pose: the last pose is within 10 mm and 0.5 deg of truth.

    Measured: 8.63 mm and 0.287 deg after frame 48 (0.2, 3.4, 5.1, 5.3, 6.8, 7.6, 8.4, 8.6 mm after
    frames 41 .. 48). With the surface maps' own normals instead of tsdf_track's point-map normals the
    same sequence ended 54.4 mm and 2.76 deg off (DESIGN.md "Pose tracking")."""
    from tsdf_amd import synth
    eng = ref.make_engine()
    try:
        cam = ref.integrate_frames(eng, [40])
        pose = ref.true_pose(40)
        for f in range(41, 49):
            fr = synth.render(cam, f)
            pose, info = eng.track(fr["depth"], cam.K, pose, ref.MAX_DEPTH)
            assert info["status"] == 0, (f, info)
            eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, pose, ref.MAX_DEPTH)
            dt, dr = ref.pose_error(pose, ref.true_pose(f))
            print(f"frame {f}: {dt * 1e3:.3f} mm {math.degrees(dr):.4f} deg, inliers {info['inliers']}, "
                  f"rmse {info['rmse'] * 1e3:.2f} mm")
        assert eng.stats()["status"] == 0
        assert dt <= 0.010 and dr <= math.radians(0.5)
    finally:
        eng.close()


def test_track_degenerate(scene):
    """An all-zero depth frame: TSDF_TRACK_DEGENERATE with the guess as the pose. A 48 x 36 frame at
    stride 4 with one level (108 samples of one view): degenerate or ok, never a non-finite pose. An
    empty volume: degenerate. min_inliers above the pixel count: degenerate."""
    import tsdf_amd
    from tsdf_amd import synth
    g = ref.true_pose(43)
    pose, info = scene.eng.track(np.zeros((72, 96), f32), scene.K, g, ref.MAX_DEPTH)
    assert info == dict(status=1, iterations=0, inliers=0, rmse=0.0)
    assert np.array_equal(pose.q, g.q) and np.array_equal(pose.t, g.t)
    small = synth.camera(48, 36, synth.TUM_FR1)
    pose, info = scene.eng.track(synth.render(small, 44)["depth"], small.K, g, ref.MAX_DEPTH, levels=1, stride=[4],
                                 iterations=[4])
    print(f"48x36 stride 4: {info}")
    assert info["status"] in (0, 1)
    assert np.isfinite(pose.q).all() and np.isfinite(pose.t).all()
    assert abs(float(np.linalg.norm(pose.q.astype(np.float64))) - 1) < 1e-6
    pose, info = scene.eng.track(scene.depth44, scene.K, g, ref.MAX_DEPTH, min_inliers=96 * 72 + 1)
    assert info["status"] == 1 and info["iterations"] == 0 and info["inliers"] > 0
    assert np.array_equal(pose.q, g.q) and np.array_equal(pose.t, g.t)
    eng = ref.make_engine()
    try:
        pose, info = eng.track(scene.depth44, scene.K, g, ref.MAX_DEPTH)
        assert info["status"] == 1 and info["inliers"] == 0 and np.array_equal(pose.t, g.t)
        with pytest.raises(tsdf_amd.TSDFError):
            eng.track(scene.depth44, scene.K, g, ref.MAX_DEPTH, levels=4)
    finally:
        eng.close()


def test_track_shard_engine_is_refused(scene):
    import tsdf_amd
    eng = tsdf_amd.Engine(ref.VOXEL, ref.TRUNC, max_width=96, max_height=72, num_block_bits=10, shard_index=0,
                          shard_count=2)
    try:
        with pytest.raises(tsdf_amd.TSDFError, match="shard"):
            eng.track(scene.depth44, scene.K, ref.true_pose(43), ref.MAX_DEPTH)
        with pytest.raises(tsdf_amd.TSDFError, match="shard"):
            eng.icp_linearize(scene.depth44, scene.K, ref.true_pose(43), scene.model, scene.K, scene.model_pose, 1,
                              MAX_DIST, ref.MAX_DEPTH)
    finally:
        eng.close()


def test_facade_track_main(tmp_path):
    """DISINFSystem::track_rgbd_frame through track_main over raw 192 x 144 frames 40-44 == the same
    stream through Engine.rgbd_half / track / integrate: the registered poses are equal as floats."""
    from tsdf_amd import synth
    full = synth.camera(192, 144, synth.TUM_FR1)
    half = synth.camera(96, 72, synth.TUM_FR1)
    frames = range(40, 45)
    raw = []
    for i, f in enumerate(frames):
        fr = synth.render(full, f)
        d16 = np.round(fr["depth"].astype(np.float64) * synth.DEPTH_FACTOR).astype(np.uint16)
        fr["rgb"].tofile(tmp_path / f"rgb_{i}.bin")
        d16.tofile(tmp_path / f"depth_{i}.bin")
        raw.append((fr["rgb"], d16))
    p0 = ref.true_pose(40)
    (tmp_path / "meta.txt").write_text(
        f"{ref.VOXEL} {ref.TRUNC} {ref.NB_BITS} {ref.MAX_DEPTH} {synth.DEPTH_FACTOR} "
        + " ".join(repr(float(v)) for v in half.K) + f" 192 144 {len(frames)}\n"
        + " ".join(repr(float(v)) for v in (*p0.q, *p0.t)) + "\n")
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(tmp_path / "out_poses.bin", f32).reshape(-1, 7)
    info = np.loadtxt(tmp_path / "out_info.txt").reshape(-1, 4)
    eng = ref.make_engine()
    try:
        pose, want, status = p0, [], []
        for rgb, d16 in raw:
            rgb_h, depth_h = eng.rgbd_half(rgb, d16, None, synth.DEPTH_FACTOR)
            pose, inf = eng.track(depth_h, half.K, pose, ref.MAX_DEPTH)
            eng.integrate(rgb_h, depth_h, None, None, half.K, pose, ref.MAX_DEPTH)
            want.append(np.concatenate([pose.q, pose.t]))
            status.append(inf["status"])
    finally:
        eng.close()
    want = np.array(want, f32)
    assert got.shape == want.shape == (len(frames), 7)
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert list(info[:, 0].astype(int)) == status == [1, 0, 0, 0, 0]  # the first frame meets an empty volume
    assert np.array_equal(got[0], np.concatenate([p0.q, p0.t]))
    dt, dr = ref.pose_error(__import__("tsdf_amd").SE3(got[-1, :4], got[-1, 4:]), ref.true_pose(44))
    print(f"facade stream: last pose {dt * 1e3:.3f} mm {math.degrees(dr):.4f} deg from truth")
