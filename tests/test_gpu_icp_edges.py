"""tsdf_icp_linearize per pixel, on its gates and through its whole sum tree, tsdf_point_map_normals
element by element, and tsdf_track's early stop: the kernels against the numpy restatement
(tests/_track_ref.py) on the hand-built inputs of tests/_icp_cases.py, which tests/test_icp_cases_cpu.py
shows to stand where they claim. Comparisons are exact unless stated.

The engine of the synthetic tests is empty (640 x 480 frames at most, 2^10 blocks): the model maps are
the caller's. The early stop and one normals test use the scene of tests/test_gpu_icp.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import _icp_cases as ic
import _track_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32


def make_engine(**kw):
    import tsdf_amd
    return tsdf_amd.Engine(ref.VOXEL, ref.TRUNC, max_width=640, max_height=480, num_block_bits=10, **kw)


@pytest.fixture(scope="module")
def _holder():
    """What the module's tests share, made by the first test that asks (the function-scoped fixtures
    below run after conftest's _torch_hip_first; a module-scoped engine would be created before it)."""
    holder = {}
    yield holder
    for v in holder.values():
        (v.eng if isinstance(v, Scene) else v).close()


@pytest.fixture
def eng(_holder):
    if "eng" not in _holder:
        _holder["eng"] = make_engine()
    return _holder["eng"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def sums29(res):
    A, b, r2, count = res
    return np.concatenate([A[np.triu_indices(6)], b, [r2, float(count)]])


def on_device(c):
    """The depth frame and the model maps of a case as device tensors."""
    import torch
    return torch.from_numpy(c["depth"]).cuda(), {k: torch.from_numpy(v).cuda() for k, v in c["model"].items()}


def linearize(e, c, depth, model, stride=1):
    return sums29(e.icp_linearize(depth, c["K"], c["pose"], model, c["model_K"], c["model_pose"], stride,
                                  c["max_dist"], c["max_depth"]))


# ---- one-hot frames ----
@pytest.mark.parametrize("stride", [1, 3, 5, 64])
def test_onehot_frames_return_their_pixel(eng, stride):
    """Each of the 23 x 17 frames with one pixel of depth and zeros elsewhere returns exactly the 29
    terms of that pixel by the restatement (J_i J_j, J_i r, r r and 1: x + 0.0 is exact at every level
    of the tree) when the pixel is on the stride lattice, and 29 zeros when it is not. Half of the
    model columns and rows are ties of the projection, rounding down and up; stride 5 ends at column
    20 < W - 1, stride 64 samples pixel (0, 0) alone."""
    import torch
    c = ic.onehot()
    t = ic.full_terms(c)
    assert t["keep"].all()
    terms = ref.icp_lane_terms(t["J"], t["r"], t["keep"])
    _, model = on_device(c)
    H, W = c["depth"].shape
    frames = torch.zeros((H * W, H, W), dtype=torch.float32)
    idx = torch.arange(H * W)
    frames[idx, idx // W, idx % W] = torch.from_numpy(c["depth"].reshape(-1))
    frames = frames.cuda()
    bad, on = [], 0
    for p in range(H * W):
        u, v = p % W, p // W
        lattice = u % stride == 0 and v % stride == 0
        on += lattice
        want = terms[p] if lattice else np.zeros(29)
        got = linearize(eng, c, frames[p], model, stride)
        if not np.array_equal(got, want):
            bad.append((u, v, int(t["um"][p]), int(t["vm"][p]), int(np.flatnonzero(got != want)[0])))
    assert on == len(range(0, W, stride)) * len(range(0, H, stride))
    assert not bad, (len(bad), bad[:8])


# ---- the gates at equality ----
@functools.lru_cache(maxsize=None)
def _gates():
    return ic.gate_cases()


GATE_NAMES = ["plain", "d_eq_max", "d_above_max", "d_negzero", "d_tiny_positive", "d_negative", "d_positive_far",
              "d_subnormal", "d_subnormal_negative", "d_nan", "pmz_half",
              "pmz_zero", "pmz_negative", "proj_finite", "proj_inf", "n_zero", "n_tiny", "point_nan", "dist_eq",
              "dist_above", "dist_zero_gate", "dist_zero_gate_off"] + [
    ax + k for ax in "uv" for k in ("m_minus_half", "m_below_minus_half", "m_minus_0.3", "m_minus_0.6", "m_eq_size",
                                    "m_last", "m_even_tie_out", "m_even_below_tie", "m_odd_tie_in", "m_odd_above_tie")]


def test_gate_names_are_all_the_cases():
    assert sorted(GATE_NAMES) == sorted(_gates())


@pytest.mark.parametrize("name", GATE_NAMES)
def test_gate_at_equality(eng, name):
    """A one-hot frame that stands on a gate: count 1 and the pixel's exact terms where the contract
    keeps it (d == max_depth, a subnormal d, um rounding to -0, a tie that stays inside, e . e ==
    max_dist^2, max_dist == 0 with e == 0, a tiny normal), 29 zeros where it drops it (the neighbouring
    float above max_depth; -0, a negative and a negative subnormal d on inputs where d > 0 alone
    decides; a NaN; pm.z < 0, and pm.z == 0, which the projection drops whatever the comparison; um ==
    W_m with and without a tie, a projection that overflows to inf, n == 0, a NaN point, one ulp beyond
    the distance gate)."""
    c, kept, _, _ = _gates()[name]
    t = ic.full_terms(c)
    assert int(t["keep"].sum()) == int(kept)
    want = ref.icp_lane_terms(t["J"], t["r"], t["keep"]).sum(axis=0)  # one non-zero row at most
    depth, model = on_device(c)
    got = linearize(eng, c, depth, model)
    assert got[28] == float(kept)
    assert np.array_equal(got, want), (got, want)
    host = sums29(eng.icp_linearize(c["depth"], c["K"], c["pose"], c["model"], c["model_K"], c["model_pose"], 1,
                                    c["max_dist"], c["max_depth"]))
    assert np.array_equal(bits(host), bits(got))


# ---- the sum tree ----
@functools.lru_cache(maxsize=None)
def _tree(W, H, stride):
    c = ic.tree_case(W, H, stride)
    t = ic.full_terms(c, stride)
    return c, t, ref.icp_tree(t["J"], t["r"], t["keep"], t["keep"].size)


TREE_SHAPES = [(256, n, 1) for n in ic.TREE_NWG] + list(ic.TREE_RAGGED)


@pytest.mark.parametrize("shape", TREE_SHAPES, ids=lambda s: "%dx%d_s%d" % s)
def test_sum_tree(eng, shape):
    """Workgroup counts 1 .. 1200 (a workgroup is a row of 256 at stride 1; k_icp_final's runs have
    lengths 1 .. 38, its 8-wide loop runs from 225 workgroups on, runs end short and stay empty) and two
    ragged lattices. In this order: the count is the restatement's; each sum is within count * 2^-53 *
    sum |term| of math.fsum of the exact terms; the 29 doubles are bit-equal to the documented tree
    (ref.icp_tree); a second call is bit-equal to the first."""
    W, H, stride = shape
    c, t, tree = _tree(W, H, stride)
    keep = t["keep"]
    nwg = (keep.size + 255) // 256
    if stride == 1 and W == 256:
        assert nwg == H
    depth, model = on_device(c)
    got = linearize(eng, c, depth, model, stride)
    want, mag = ref.icp_sums_exact(t["J"][keep], t["r"][keep])
    print(f"{W}x{H} stride {stride}: {nwg} workgroups, runs of {(nwg + 31) // 32}, {int(want[28])} of {keep.size} kept")
    assert got[28] == want[28] == keep.sum() and 0 < want[28] < keep.size
    bound = want[28] * 2.0 ** -53 * mag[:28]
    err = np.abs(got[:28] - want[:28])
    print(f"  largest error / bound: {np.max(err / np.maximum(bound, 1e-300)):.3g}; "
          f"sums that differ from the tree: {int((bits(got) != bits(tree)).sum())}")
    assert (err <= bound).all(), np.flatnonzero(err > bound)
    assert np.array_equal(bits(got), bits(tree)), np.flatnonzero(bits(got) != bits(tree))
    again = linearize(eng, c, depth, model, stride)
    assert np.array_equal(bits(again), bits(got))


def test_sum_tree_ignores_stale_scratch(eng):
    """The partials' buffer only grows and the total sits at its end: 33 workgroups after 1200 on one
    engine give the doubles of 33 workgroups on a fresh engine."""
    big, small = _tree(256, 1200, 1)[0], _tree(256, 33, 1)[0]
    linearize(eng, big, *on_device(big))
    after = linearize(eng, small, *on_device(small))
    fresh_eng = make_engine()
    try:
        fresh = linearize(fresh_eng, small, *on_device(small))
    finally:
        fresh_eng.close()
    assert np.array_equal(bits(after), bits(fresh))
    assert np.array_equal(bits(after), bits(_tree(256, 33, 1)[2]))


# ---- the point-map normals ----
def _smooth_map(W, H, seed=3):
    """A W x H point map of a wavy surface about 2 m away, a surface everywhere."""
    rng = np.random.default_rng(seed)
    K = (30.0, 30.0, W / 2, H / 2)
    v, u = np.mgrid[0:H, 0:W]
    F = ref.Camera(K, ic.se3())
    ray = F.pixel_ray(u.reshape(-1), v.reshape(-1))
    d = 2 + 0.03 * np.sin(0.7 * u) + 0.02 * np.cos(0.9 * v) + rng.uniform(-0.004, 0.004, u.shape)
    d = d.astype(f32).reshape(-1)
    point = np.stack([ray[0] * d, ray[1] * d, d], -1).reshape(H, W, 3)
    return dict(point=point, normal=np.ones_like(point)), K, ic.se3()


def _check_normals(e, model, K, pose):
    import torch
    want = ref.point_map_normals(model, K, pose)["normal"]
    got = e.point_map_normals(model, K, pose)
    assert got.dtype == f32 and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), np.argwhere((bits(got) != bits(want)).any(-1))[:8]
    dev = e.point_map_normals({k: torch.from_numpy(v).cuda() for k, v in model.items()}, K, pose)
    assert dev.is_cuda and np.array_equal(bits(dev.cpu().numpy()), bits(got))
    return want


def test_point_map_normals_on_every_rule(eng):
    """The 37 x 21 map of _icp_cases.normals_case (partial 16 x 16 tiles; the angle gate swept through
    0.3 on a cylinder, holes, a depth edge, a patch that needs the flip, duplicate neighbours, points
    1e19 apart, a NaN point), seen from the origin and, for the flip's other sign, from behind the
    surface: every component of every pixel is the restatement's, from host maps and from device maps."""
    model, K, pose = ic.normals_case()
    want = _check_normals(eng, model, K, pose)
    assert (want != 0).any(-1).sum() >= 20
    behind = ic.se3(t=(0.0, 0.0, -6.0))  # camera centre at z = +6: every c is turned the other way
    other = _check_normals(eng, model, K, behind)
    assert ((other != 0).any(-1) & (want != 0).any(-1)).sum() >= 20


@pytest.mark.parametrize("size", [(1, 1), (3, 2), (2, 5), (16, 16), (17, 17)])
def test_point_map_normals_sizes(eng, size):
    """Maps that are all border (1 x 1, 3 x 2, 2 x 5: zeros), one full tile and one pixel more."""
    model, K, pose = _smooth_map(*size)
    want = _check_normals(eng, model, K, pose)
    assert (want != 0).any(-1).sum() == ((size[0] - 2) * (size[1] - 2) if min(size) > 2 else 0)


def test_point_map_normals_arguments(eng):
    """NULL arguments, more pixels than max_pixels and a bad mem_kind are TSDF_ERR_INVALID_ARG (1); a
    shard engine is refused with the "shard" message; maps of unequal shape, and device tensors that are
    not float32, are a ValueError before anything is launched."""
    import tsdf_amd
    from tsdf_amd import _lib
    L = _lib.load()
    model, K, pose = _smooth_map(8, 6)
    out = np.zeros_like(model["point"])
    Kc, Pc = eng._Kc(K), pose._c()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = [eng._h, C.byref(Kc), 8, 6, C.byref(Pc), p(model["point"]), p(model["normal"]), p(out), _lib.TSDF_MEM_HOST]
    assert L.tsdf_point_map_normals(*good) == 0 and out.any()
    for i in (0, 1, 4, 5, 6, 7):
        bad = list(good)
        bad[i] = None
        assert L.tsdf_point_map_normals(*bad) == 1, i
        assert b"tsdf_point_map_normals" in L.tsdf_last_error()
    for i, v in ((2, 0), (3, -1), (2, 641 * 480), (8, 7)):
        bad = list(good)
        bad[i] = v  # (the size is refused before a map is touched)
        assert L.tsdf_point_map_normals(*bad) == 1, (i, v)
    with pytest.raises(ValueError):
        eng.point_map_normals(dict(point=model["point"], normal=model["normal"][:-1]), K, pose)
    import torch
    half = {k: torch.from_numpy(v).cuda().half() for k, v in model.items()}
    with pytest.raises(ValueError, match="float32"):  # (empty_like would give an out of half the size)
        eng.point_map_normals(half, K, pose)
    with pytest.raises(ValueError, match="float32"):
        eng.icp_linearize(half["point"][..., 0], K, pose, half, K, pose, 1, 0.1, ref.MAX_DEPTH)
    shard = tsdf_amd.Engine(ref.VOXEL, ref.TRUNC, max_width=96, max_height=72, num_block_bits=10, shard_index=0,
                            shard_count=2)
    try:
        with pytest.raises(tsdf_amd.TSDFError, match="shard"):
            shard.point_map_normals(model, K, pose)
    finally:
        shard.close()


# ---- the scene of test_gpu_icp.py ----
class Scene:
    def __init__(self):
        from tsdf_amd import synth
        self.eng = ref.make_engine()
        self.cam = ref.integrate_frames(self.eng, range(40, 44))
        assert self.eng.stats()["status"] == 0
        self.K = self.cam.K
        self.depth44 = synth.render(self.cam, 44)["depth"]
        self.guess = ref.true_pose(40)
        self.norms = []
        self.base = self.eng.track(self.depth44, self.K, self.guess, ref.MAX_DEPTH)
        self.ref_base = ref.track(self.eng, self.depth44, self.K, self.guess, norms=self.norms)


@pytest.fixture
def scene(_holder):
    if "scene" not in _holder:
        _holder["scene"] = Scene()
    return _holder["scene"]


def test_point_map_normals_of_a_raycast(scene):
    """point_map_normals(raycast_surface(...)) on the 96 x 72 scene is the restatement bit for bit."""
    pose = ref.true_pose(43)
    model = scene.eng.raycast_surface(scene.K, 96, 72, pose, ref.MAX_DEPTH, maps=())
    want = _check_normals(scene.eng, model, scene.K, pose)
    assert (want != 0).any(-1).sum() > 3000


def _same_pose(a, b):
    return np.array_equal(a.q, b.q) and np.array_equal(a.t, b.t)


def test_early_stop_after_one_iteration_per_level(scene):
    """eps_rot = eps_trans = 1e9: every level ends after its first update; status 0, three iterations,
    and the pose of the numpy loop under the same eps within 1e-4 m and 1e-4 rad."""
    pose, info = scene.eng.track(scene.depth44, scene.K, scene.guess, ref.MAX_DEPTH, eps_rot=1e9, eps_trans=1e9)
    rpose, rstatus, riters, _, _ = ref.track(scene.eng, scene.depth44, scene.K, scene.guess, eps_rot=1e9,
                                             eps_trans=1e9)
    assert info["status"] == 0 and rstatus == 0
    assert info["iterations"] == 3 and riters == 3
    dt, dr = ref.pose_error(pose, rpose)
    assert dt <= 1e-4 and dr <= 1e-4
    assert not _same_pose(pose, scene.base[0])


@pytest.mark.parametrize("which", ["eps_rot", "eps_trans"])
def test_early_stop_needs_both_norms(scene, which):
    """Only one eps positive: the other norm is never within 0, so all 19 iterations run and the pose
    is the default call's bit for bit."""
    pose, info = scene.eng.track(scene.depth44, scene.K, scene.guess, ref.MAX_DEPTH, **{which: 1e9})
    assert scene.base[1]["status"] == 0 and scene.base[1]["iterations"] == 19
    assert info == scene.base[1]
    assert _same_pose(pose, scene.base[0])


def pick_stop(norms, iterations=(4, 5, 10)):
    """From the recorded (level, |omega|, |t|) of a loop without early stop: the first iteration k >= 2
    of the last level at which both norms are at least 4 times smaller than at k - 1, or smaller than
    the largest of all earlier iterations of that level; and the eps pair at the geometric means of the
    norms at k - 1 and k, as floats. None if there is no such k. The second clause holds for any
    decrease, so it guards nothing: what keeps solver rounding from deciding a stop is the clearance
    that test_early_stop_mid_value asserts for every decision of the loop under the pair."""
    first = sum(iterations[:-1])
    last = norms[first:]
    for k in range(2, len(last)):
        (_, w0, t0), (_, w1, t1) = last[k - 1], last[k]
        if (4 * w1 <= w0 and 4 * t1 <= t0) or (w1 < max(n[1] for n in last[:k]) and t1 < max(n[2] for n in last[:k])):
            return k, float(f32((w0 * w1) ** 0.5)), float(f32((t0 * t1) ** 0.5))
    return None


def test_early_stop_mid_value(scene):
    """eps between two iterations of the last level. From the numpy loop's recorded norms (pick_stop) an
    iteration k >= 2 of the last level and eps_rot, eps_trans at the geometric means of the norms at
    k - 1 and k: the engine and the numpy loop under that pair run the same number of iterations, fewer
    than 19, and their poses agree within 1e-4 m and 1e-4 rad. Every stop decision of the numpy loop is
    asserted to be clear of its eps by a factor 1.1, far more than the two Cholesky solves can differ:
    that assertion, not pick_stop's rule, is the guard.

    Recorded on an MI355X (guess pose 40; the maps are the GPU's, the loop is numpy's), |omega| [rad] /
    |t| [m] per iteration without early stop:
      stride 4: 1.70e-2 / 7.64e-2, 3.25e-2 / 1.75e-1, 2.40e-3 / 1.04e-2, 2.50e-4 / 1.24e-3
      stride 2: 1.12e-3 / 6.46e-3, 2.86e-4 / 8.52e-4, 2.32e-5 / 8.42e-5, 1.88e-7 / 1.34e-6, 5.29e-8 / 3.87e-7
      stride 1: 3.72e-4 / 3.41e-4, 2.99e-5 / 1.11e-4, 1.13e-5 / 4.25e-5, 9.25e-6 / 1.72e-5, 9.35e-6 / 1.76e-5,
                9.46e-6 / 1.81e-5, 9.45e-6 / 3.20e-5, 9.36e-6 / 3.16e-5, 9.21e-6 / 3.10e-5, 9.19e-6 / 3.06e-5
    The last level falls by 2.7 and 2.6 from its iteration 1 to 2 (not by 4) and then stays at about
    9e-6 rad, so k = 2 is taken by the second clause: eps_rot = 1.83e-5, eps_trans = 6.87e-5. Under that
    pair the stride-2 level also ends early, after its fourth iteration, and the last level after its
    third: 4 + 4 + 3 = 11 iterations in both loops."""
    norms = scene.norms
    assert len(norms) == 19 and scene.ref_base[1] == 0
    for l, w, t in norms:
        print(f"level {l}: |omega| {w:.3e} |t| {t:.3e}")
    pick = pick_stop(norms)
    assert pick is not None, norms
    k, er, et = pick
    under = []
    rpose, rstatus, riters, _, _ = ref.track(scene.eng, scene.depth44, scene.K, scene.guess, eps_rot=er, eps_trans=et,
                                             norms=under)
    pose, info = scene.eng.track(scene.depth44, scene.K, scene.guess, ref.MAX_DEPTH, eps_rot=er, eps_trans=et)
    print(f"k = {k}: eps_rot {er:.3e} eps_trans {et:.3e}; iterations {info['iterations']} / {riters}")
    for l, w, t in under:
        print(f"  level {l}: |omega| / eps {w / er:.3g} |t| / eps {t / et:.3g}")
        stop = w <= er and t <= et
        assert (w * 1.1 <= er and t * 1.1 <= et) if stop else (w >= 1.1 * er or t >= 1.1 * et)
    assert info["status"] == 0 and rstatus == 0
    assert info["iterations"] == riters == len(under) and 3 < riters < 19
    assert under[-1][0] == 2 and under[-1][1] <= er and under[-1][2] <= et  # the last level did stop early
    dt, dr = ref.pose_error(pose, rpose)
    print(f"  engine vs numpy loop {dt:.3g} m, {dr:.3g} rad")
    assert dt <= 1e-4 and dr <= 1e-4
