"""tsdf_view_gain on the GPU against its numpy restatement (_view_ref.py): every predicted depth image and every
gain bit for bit, host and device memory, with the skip path and the plain march. The figures of the worked
example are computed in tests/test_view_cpu.py from the restatement alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _free_ref as fref
import _view_ref as vr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "view_main")
VOXEL, TRUNC = 0.01, 0.03
TSDF_ERR_INVALID_ARG = 1
f32 = np.float32
# the worked example (the issue's; test_view_cpu.WORKED)
W_ORIGIN, W_DIMS, W_K, W_W, W_H, W_FAR, W_STEP = (-20, -10, -3), (70, 21, 40), (20.0, 20.0, 7.5, 5.5), 16, 12, 0.6, 0.005
IDENT = ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
AWAY = ((0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0))       # turned 180 degrees about y
OUTSIDE = ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.2))    # 20 cm behind the box, looking in along z


def worked_state():
    st = np.zeros(W_DIMS[::-1], np.uint8)
    st[:30, :, :20] = 1
    st[30:34] = 2
    return st


def make_engine(voxel=VOXEL, trunc=TRUNC, w=64, h=64, env=None, nb_bits=13, **kw):
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
    assert e.stats()["status"] == 0
    e.close()


@pytest.fixture(scope="module")
def plain():
    e = make_engine(env={"TSDF_VIEW_SKIP": "0"})
    yield e
    e.close()


def host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else a


def se3(view):
    import tsdf_amd
    return tsdf_amd.SE3(np.asarray(view[0], f32), np.asarray(view[1], f32))


def layer_of(mask, origin, junk_padding=False):
    """A host layer holding a bool mask; junk_padding sets the padding bits of every row's last word."""
    nz, ny, nx = mask.shape
    bits = fref.pack(mask)
    if junk_padding and nx % 32:
        bits[..., -1] |= np.uint32((0xFFFFFFFF << (nx % 32)) & 0xFFFFFFFF)
    return dict(bits=np.ascontiguousarray(bits), origin=tuple(origin), dims=(nx, ny, nz))


def check(engines, state, origin, views, K, W, H, far, step, margin, miss, seen=None, voxel=VOXEL, tag="",
          junk_padding=False, want=None):
    """Every engine, both memory kinds, against the restatement; returns (gain, pred, vis) of the restatement."""
    import torch
    if want is None:
        want = vr.view_gain(state, origin, voxel, K, W, H, views, far, step, margin, miss, seen)
    gain, pred, _ = want
    poses = [se3(v) for v in views]
    field = dict(state=state, origin=tuple(origin), dims=state.shape[::-1])
    layer = None if seen is None else layer_of(seen, origin, junk_padding)
    for e in engines if isinstance(engines, (list, tuple)) else [engines]:
        for device in (False, True):
            f, l = field, layer
            if device:
                f = dict(field, state=torch.as_tensor(state, device=f"cuda:{e.device}"))
                if layer is not None:
                    l = dict(layer, bits=torch.as_tensor(layer["bits"].view(np.int32), device=f"cuda:{e.device}"))
            got = e.view_gain(f, poses, K, W, H, far, step=step, margin=margin, miss_depth=miss, seen=l, depth=True,
                              device=device)
            d = host(got["depth"])
            print(f"{tag} device={device}: gains {got['gain'].tolist()[:6]} want {gain.tolist()[:6]}, depth differs at "
                  f"{int((d.view(np.uint32) != pred.view(np.uint32)).sum())} of {pred.size} pixels")
            assert bool(hasattr(got["depth"], "is_cuda")) == device
            assert d.dtype == np.float32 and d.shape == (len(views), H, W)
            assert np.array_equal(d.view(np.uint32), pred.view(np.uint32))
            assert got["gain"].dtype == np.int64 and np.array_equal(got["gain"], gain)
            assert got["origin"] == tuple(origin) and got["dims"] == state.shape[::-1]
            again = e.view_gain(f, poses, K, W, H, far, step=step, margin=margin, miss_depth=miss, seen=l, device=device)
            assert again["depth"] is None and np.array_equal(again["gain"], gain)
    return want


@pytest.mark.parametrize("miss", [W_FAR, 0.0])
def test_worked_example(eng, plain, miss):
    """Facing the wall, facing away, and standing outside the box looking in; the skip path and the plain march."""
    st = worked_state()
    gain, pred, vis = check([eng, plain], st, W_ORIGIN, [IDENT, AWAY, OUTSIDE], W_K, W_W, W_H, W_FAR, W_STEP, TRUNC, miss,
                            tag=f"worked miss {miss}")
    assert (pred[0] == f32(0.265)).all() and int(vis[0].sum()) == 2035 and gain[0] == 1100 and not vis[0][30:].any()
    assert (pred[1] == f32(miss)).all() and (gain[1] == 0) == (miss == 0.0)
    assert f32(0.4) < pred[2, 6, 8] < f32(0.5) and (pred[2, 0] == f32(miss)).all() and gain[2] > gain[0]


def many_views(n, seed):
    """n different poses around a small box: unit quaternions at random, camera centres within 10 cm."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q = rng.normal(size=4)
        q = (q / np.linalg.norm(q)).astype(f32)
        out.append((tuple(float(v) for v in q), tuple(float(v) for v in rng.uniform(-0.1, 0.1, 3).astype(f32))))
    return out


@pytest.mark.parametrize("over", [1, 65, 129])
def test_batching(eng, plain, over):
    """V = 1, batch + 1 and 2 batch + 1 at 8 x 6 on a 33 x 9 x 9 box, every view different; V = 0."""
    import tsdf_amd
    assert tsdf_amd.VIEW_BATCH == 64
    rng = np.random.default_rng(2)
    st = rng.choice(np.array([0, 1, 2], np.uint8), size=(9, 9, 33), p=[0.6, 0.3, 0.1])
    views = many_views(over, 5)
    assert len({v for v in views}) == over
    gain, _, _ = check([eng, plain], st, (-16, -4, -4), views, (6.0, 6.0, 3.5, 2.5), 8, 6, 0.4, 0.004, 0.0, 0.4,
                       tag=f"batch V={over}")
    assert over == 1 or (gain > 0).sum() > over // 2
    for device in (False, True):
        got = eng.view_gain(dict(state=st, origin=(-16, -4, -4), dims=(33, 9, 9)), [], (6.0, 6.0, 3.5, 2.5), 8, 6, 0.4,
                            depth=True, device=device)
        assert got["gain"].shape == (0,) and tuple(got["depth"].shape) == (0, 6, 8)


def test_ties_and_signs(eng, plain):
    """An axis-aligned camera at an exact voxel centre with step = voxel / 2 (every second sample a tie) over a
    box with a negative origin; a camera inside a state-2 voxel (a hit at j = 1); a camera in the box's last
    voxel; margin 0; miss_depth 0 against far."""
    v = f32(0.0078125)  # 2^-7: voxel centres and the half steps are exact
    e2, p2 = make_engine(voxel=float(v), trunc=0.03), make_engine(voxel=float(v), trunc=0.03, env={"TSDF_VIEW_SKIP": "0"})
    try:
        origin, dims = (-9, -7, -5), (40, 15, 17)
        rng = np.random.default_rng(3)
        st = rng.choice(np.array([0, 1, 2], np.uint8), size=dims[::-1], p=[0.7, 0.27, 0.03])
        K, W, H = (12.0, 12.0, 7.5, 5.5), 16, 12
        centre = (-3, 0, -2)  # a voxel of the box: the camera sits exactly on it
        t0 = tuple(-float(f32(c) * v) for c in centre)
        axis = [((0.0, 0.0, 0.0, 1.0), t0), ((0.0, 1.0, 0.0, 0.0), (-t0[0], t0[1], -t0[2]))]
        half = float(v / f32(2))
        want = check([e2, p2], st, origin, axis, K, W, H, 0.25, half, 0.0, 0.25, voxel=float(v), tag="ties, margin 0")
        # the centre pixel's samples are ties in z at every odd j: the restatement sees them on k + 1/2
        z = np.arange(1, 64, 2, dtype=f32) * f32(half)
        assert (((z - f32(t0[2])) / v) % 1 == 0.5).all()
        check([e2, p2], st, origin, axis, K, W, H, 0.25, half, 0.03, 0.0, voxel=float(v), tag="ties, miss 0")
        assert not np.array_equal(want[0], check(e2, st, origin, axis, K, W, H, 0.25, half, 0.03, 0.25, voxel=float(v))[0])
        # inside a state-2 voxel: the first sample of every ray near the axis lies in it
        st2 = st.copy()
        c = np.array(centre) - np.array(origin)
        st2[c[2], c[1], c[0]] = 2
        g, p, _ = check([e2, p2], st2, origin, axis[:1], K, W, H, 0.25, float(v) / 4, 0.0, 0.25, voxel=float(v),
                        tag="inside a wall voxel")
        assert p[0, 5, 7] == f32(float(v) / 4) or p[0, 6, 8] == f32(float(v) / 4)
        # the camera centre in the box's last voxel, looking back along the diagonal
        from tsdf_amd import esdf
        last = (np.array(origin) + np.array(dims) - 1).astype(np.float64) * float(v)
        pose = esdf.look_at(last, np.array(origin, np.float64) * float(v))
        corner = [(tuple(float(x) for x in pose.q), tuple(float(x) for x in pose.t))]
        g, _, _ = check([e2, p2], st, origin, corner, K, W, H, 0.25, float(v), 0.0, 0.25, voxel=float(v), tag="last voxel")
        assert g[0] > 0
    finally:
        e2.close()
        p2.close()


def test_frustum_borders_tilted(eng, plain):
    """A tilted, non-axis pose over a box wider than its frustum: unobserved voxels whose quotient lands within
    one pixel of each image border, on either side of it."""
    origin, dims = (-30, -30, -10), (67, 61, 50)
    st = np.zeros(dims[::-1], np.uint8)
    st[44:] = 2  # a wall at the far end
    st[:, :, 60:] = 1
    q = np.array([0.08, -0.05, 0.12, 1.0])
    q = (q / np.linalg.norm(q)).astype(f32)
    view = (tuple(float(c) for c in q), (0.013, -0.021, 0.05))
    K, W, H = (14.0, 15.0, 7.3, 5.6), 16, 12
    want = check([eng, plain], st, origin, [view], K, W, H, 0.6, 0.01, 0.02, 0.6, tag="tilted")
    tm = fref.terms(fref.box_points(origin, dims), fref.frame(want[1][0], K, view[0], view[1], np.inf), VOXEL, 0.02)
    front = (tm["hz"] > 0) & (st == 0)
    for q_, n in ((tm["uq"], W), (tm["vq"], H)):
        for lo, hi in ((-1.5, -0.5), (-0.5, 0.5), (n - 1.5, n - 0.5), (n - 0.5, n + 0.5)):
            assert int((front & (q_ >= lo) & (q_ < hi)).sum()) > 10, (n, lo)
    assert 0 < want[0][0] < int(front.sum())


def test_pose_and_state_edges(eng, plain):
    """A pose scaled by 1 + 2^-8 is no rotation (no cull): it still equals the restatement. State bytes other
    than 0, 1 and 2 are neither unknown nor opaque."""
    st = worked_state()
    s = f32(1) + f32(2.0 ** -8)
    q = np.array([0.05, 0.02, -0.03, 1.0])
    q = (q / np.linalg.norm(q)).astype(f32) * s
    n2 = float((q.astype(np.float64) ** 2).sum())
    assert abs(n2 - 1) > 2.0 ** -10
    scaled = (tuple(float(c) for c in q), (0.01, 0.0, -0.02))
    g, _, _ = check([eng, plain], st, W_ORIGIN, [scaled, IDENT], W_K, W_W, W_H, W_FAR, W_STEP, TRUNC, W_FAR, tag="scaled pose")
    assert g[0] > 0 and g[1] == 1100
    odd = st.copy()
    odd[30:34, :, :20] = 3     # half the wall becomes a byte that is not opaque
    odd[20:25, :, 20:] = 255   # and part of the unknown a byte that is not unknown
    g2, p2, _ = check([eng, plain], odd, W_ORIGIN, [IDENT], W_K, W_W, W_H, W_FAR, W_STEP, TRUNC, W_FAR, tag="odd bytes")
    assert (p2[0] == f32(W_FAR)).any() and (p2[0] == f32(0.265)).any() and g2[0] != 1100


def test_seen_and_identity(eng, plain):
    """`seen` with a partly set last word, and padding bits set by the caller; determinism over repeated calls;
    gain == the new bits of Engine.free_observe(pred) on state 0 (margin == truncation, max_depth 2 far)."""
    from tsdf_amd import esdf
    st = worked_state()
    rng = np.random.default_rng(9)
    seen = rng.random(st.shape) < 0.4
    seen[:, :, 64:] = False
    seen[:, :, 66] = True  # the last word (6 bits) partly set
    views = [IDENT, OUTSIDE, AWAY]
    none = check(eng, st, W_ORIGIN, views, W_K, W_W, W_H, W_FAR, W_STEP, TRUNC, W_FAR, tag="no seen")
    with_seen = check([eng, plain], st, W_ORIGIN, views, W_K, W_W, W_H, W_FAR, W_STEP, TRUNC, W_FAR, seen=seen,
                      junk_padding=True, tag="seen, junk padding")
    assert np.array_equal(with_seen[0], [int(((st == 0) & ~seen & m).sum()) for m in none[2]])
    assert (with_seen[0][:2] < none[0][:2]).all() and (with_seen[0][:2] > 0).all()
    for _ in range(3):
        check(eng, st, W_ORIGIN, views, W_K, W_W, W_H, W_FAR, W_STEP, TRUNC, W_FAR, seen=seen, want=with_seen, tag="again")
    # the identity, through the GPU's own free_observe
    for i, view in enumerate(views):
        layer = layer_of(seen, W_ORIGIN)
        eng.free_observe(layer, none[1][i], W_K, se3(view), 2 * W_FAR)
        new = esdf.free_mask(layer) & ~seen
        assert int((new & (st == 0)).sum()) == with_seen[0][i]


def raw(e, V=2, device=False, h=0, cfgp=True, statep=True, viewsp=True, gainp=True, depthp=True, kind=None, **cfg):
    """tsdf_view_gain through ctypes on the worked example: (rc, untouched)."""
    import torch
    import tsdf_amd
    lib = tsdf_amd._lib
    L = lib.load()
    c = lib.ViewConfig()
    L.tsdf_view_config_default(e._h, C.byref(c))
    vals = dict(origin=W_ORIGIN, dims=W_DIMS, width=W_W, height=W_H, far=W_FAR, step=W_STEP, margin=TRUNC, miss_depth=W_FAR)
    vals.update(cfg)
    c.origin, c.dims = (C.c_int32 * 3)(*vals["origin"]), (C.c_int32 * 3)(*vals["dims"])
    c.width, c.height, c.K = vals["width"], vals["height"], lib.Intrinsics(*W_K)
    c.far, c.step, c.margin, c.miss_depth = vals["far"], vals["step"], vals["margin"], vals["miss_depth"]
    st = worked_state()
    n = max(V, 1)
    poses = (lib.Pose * n)(*[se3(IDENT)._c() for _ in range(n)])
    gain = np.full(n, -7, np.int64)
    depth = np.full((n, W_H, W_W), -7.0, f32)
    if device:
        ds, dd = torch.as_tensor(st, device=f"cuda:{e.device}"), torch.as_tensor(depth, device=f"cuda:{e.device}")
        torch.cuda.synchronize()
        ps, pd = ds.data_ptr(), dd.data_ptr()
    else:
        ps, pd = st.ctypes.data, depth.ctypes.data
    rc = L.tsdf_view_gain(e._h if h == 0 else h, C.byref(c) if cfgp else None, ps if statep else None, None,
                          C.cast(poses, C.c_void_p) if viewsp else None, V, gain.ctypes.data if gainp else None,
                          pd if depthp else None, int(device) if kind is None else kind)
    if device:
        depth = dd.cpu().numpy()
    return rc, bool((gain == -7).all() and (depth == -7.0).all())


def test_arguments(eng):
    import tsdf_amd
    lib = tsdf_amd._lib
    L = lib.load()
    c = lib.ViewConfig()
    L.tsdf_view_config_default(eng._h, C.byref(c))
    assert (c.far, c.step, c.margin, c.miss_depth) == (3.0, f32(VOXEL), f32(TRUNC), 3.0)
    assert list(c.origin) + list(c.dims) + [c.width, c.height] == [0] * 8 and (c.K.fx, c.K.fy, c.K.cx, c.K.cy) == (0, 0, 0, 0)
    for device in (False, True):
        assert raw(eng, device=device) == (0, False)
        assert raw(eng, device=device, depthp=False)[0] == 0
        assert raw(eng, V=0, device=device) == (0, True)
        assert raw(eng, V=0, device=device, viewsp=False, gainp=False, depthp=False) == (0, True)
    inf, nan = float("inf"), float("nan")
    bad = [dict(dims=(0, 21, 40)), dict(dims=(70, 2049, 40)), dict(dims=(70, 21, -1)), dict(dims=(2048, 2048, 65)),
           dict(origin=(-262145, 0, 0)), dict(origin=(0, 262144 - 20, 0)), dict(width=0), dict(width=65), dict(height=0),
           dict(height=65), dict(V=-1), dict(V=4097), dict(far=0.0), dict(far=-1.0), dict(far=inf), dict(far=nan),
           dict(step=0.0), dict(step=-0.005), dict(step=inf), dict(step=nan), dict(step=0.7), dict(far=3.0, step=0.00004),
           dict(margin=-0.01), dict(margin=inf), dict(margin=nan), dict(miss_depth=-0.1), dict(miss_depth=0.61),
           dict(miss_depth=nan), dict(miss_depth=inf), dict(kind=2), dict(kind=-1), dict(h=None), dict(cfgp=False),
           dict(statep=False), dict(viewsp=False), dict(gainp=False)]
    for kw in bad:
        for device in (False, True):
            assert raw(eng, device=device, **kw) == (TSDF_ERR_INVALID_ARG, True), kw
    # V * W * H above 2^26 (an engine that admits the image)
    big = make_engine(w=1024, h=1024)
    try:
        assert raw(big, V=65, width=1024, height=1024) == (TSDF_ERR_INVALID_ARG, True)
    finally:
        big.close()
    st = worked_state()
    with pytest.raises(lib.TSDFError, match="invalid argument"):
        eng.view_gain((st, W_ORIGIN, W_DIMS), [se3(IDENT)], W_K, W_W, W_H, -1.0)
    with pytest.raises(ValueError):
        eng.view_gain((st, W_ORIGIN, (70, 21, 41)), [se3(IDENT)], W_K, W_W, W_H, W_FAR)
    with pytest.raises(ValueError):
        eng.view_gain(dict(state=None, origin=W_ORIGIN, dims=W_DIMS), [se3(IDENT)], W_K, W_W, W_H, W_FAR)
    with pytest.raises(ValueError):
        eng.view_gain((st, W_ORIGIN, W_DIMS), [se3(IDENT)], W_K, W_W, W_H, W_FAR,
                      seen=layer_of(np.zeros(st.shape, bool), (0, 0, 0)))
    assert eng.stats()["status"] == 0


def test_scratch_growth_and_shard():
    """Small, larger, small again on a fresh engine (its scratch starts empty); a shard engine serves."""
    rng = np.random.default_rng(4)
    small = rng.choice(np.array([0, 1, 2], np.uint8), size=(9, 9, 33), p=[0.6, 0.3, 0.1])
    args = ((-16, -4, -4), many_views(3, 8), (6.0, 6.0, 3.5, 2.5), 8, 6, 0.4, 0.004, 0.0, 0.4)
    e = make_engine()
    shard = make_engine(shard_index=1, shard_count=2)
    try:
        a = check(e, small, *args, tag="small")
        check(e, worked_state(), W_ORIGIN, [IDENT, OUTSIDE] * 4, W_K, W_W, W_H, W_FAR, W_STEP, TRUNC, W_FAR, tag="larger")
        check(e, small, *args, want=a, tag="small again")
        check(shard, small, *args, want=a, tag="shard")
        assert e.stats()["status"] == 0
    finally:
        e.close()
        shard.close()


def test_pending_frames_stay_as_they_were():
    """Frames integrated back to back, view_gain between them: the volume ends bit-identical to that of an engine
    that never made the call, with the same number of pipelined launches."""
    import tsdf_amd
    from tsdf_amd import synth
    cam = synth.camera(80, 60)
    st = worked_state()
    want = vr.view_gain(st, W_ORIGIN, 0.005, W_K, W_W, W_H, [IDENT, OUTSIDE], 0.3, 0.005, 0.03, 0.3)
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
                    check(e, st, W_ORIGIN, [IDENT, OUTSIDE], W_K, W_W, W_H, 0.3, 0.005, 0.03, 0.3, voxel=0.005, want=want,
                          tag="between frames")
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


S_VOXEL, S_TRUNC, S_DIMS, S_W, S_H, S_FAR, S_YAWS, S_MIN = 0.02, 0.08, (100, 100, 60), 40, 30, 1.5, 4, 40


def scene_setup(e, device):
    """The frontier scene test's stream: three synthetic frames, the free layer, the distance field, free_apply,
    the travel field and the frontiers; (field, frontiers, views, owner, K)."""
    import tsdf_amd
    from tsdf_amd import esdf, synth
    cam = synth.camera(80, 60)
    frames = [synth.render(cam, k) for k in (0, 10, 20)]
    last = tsdf_amd.SE3(frames[-1]["q"], frames[-1]["t"])

    def in_front(z):
        p = last.Inverse().Apply(np.array([0.0, 0.0, z], np.float32))
        return np.round(p.astype(np.float64) / S_VOXEL).astype(np.int64)

    origin = tuple(int(v) for v in in_front(1.0) - np.array(S_DIMS) // 2)
    layer = esdf.free_layer(origin, S_DIMS, device=device)
    for f in frames:
        pose = tsdf_amd.SE3(f["q"], f["t"])
        e.integrate(f["rgb"], f["depth"], f["ht"], f["lt"], cam.K, pose, 4.0)
        e.free_observe(layer, f["depth"], cam.K, pose, 4.0)
    field = e.free_apply(layer, e.distance_field(origin, S_DIMS, device=device))
    travel = e.travel_field(field, [in_front(0.3)], clearance2=4, unknown_free=False, device=device)
    fr = e.frontiers(field, travel, min_size=S_MIN, device=device)
    views, owner = esdf.view_candidates(fr, S_VOXEL, yaws=S_YAWS)
    small = synth.camera(S_W, S_H)
    return field, fr, views, owner, small.K, last


@pytest.mark.parametrize("device", [False, True])
def test_scene_next_views(device):
    """Frames -> free layer -> distance field -> free_apply -> travel field -> frontiers -> view_candidates ->
    next_views(k = 3): chosen views and gains equal the restatement's greedy loop on the same arrays."""
    from tsdf_amd import esdf
    e = make_engine(voxel=S_VOXEL, trunc=S_TRUNC, w=80, h=60)
    try:
        field, fr, views, owner, K, last = scene_setup(e, device)
        assert len(views) == S_YAWS * fr["count"] > 0 and owner.tolist() == sorted(owner.tolist())
        views, owner = views[:6 * S_YAWS], owner[:6 * S_YAWS]  # (the restatement's time: six clusters at most)
        # one more candidate: the last frame's own pose, turned towards the wall that is already mapped
        views = views + [last]
        chosen, gains, seen = esdf.next_views(e, field, views, K, S_W, S_H, 3, far=S_FAR, device=device)
        state = host(field["state"])
        vt = [(tuple(float(c) for c in v.q), tuple(float(c) for c in v.t)) for v in views]
        wc, wg, wseen = vr.next_views(state, field["origin"], S_VOXEL, S_TRUNC, K, S_W, S_H, vt, 3, S_FAR, S_VOXEL, S_FAR)
        print(f"scene device={device}: {len(views)} candidates, chosen {chosen} gains {gains}; restatement {wc} {wg}")
        assert chosen == wc and gains == wg and len(chosen) >= 1 and gains[0] > 0
        assert gains == sorted(gains, reverse=True)
        assert np.array_equal(esdf.free_mask(seen), wseen)
        assert sum(gains) == int((wseen & (state == 0)).sum())
        first = e.view_gain(field, views, K, S_W, S_H, S_FAR, device=device)["gain"]
        assert first[-1] < gains[0] and int(first.max()) == gains[0] and int(np.argmax(first)) == chosen[0]
        assert e.stats()["status"] == 0
    finally:
        e.close()


def test_facade(tmp_path):
    """DISINFSystem::query_next_views (view_main) on the scene's frames: candidates, chosen views, gains and the
    seen layer equal Python's."""
    import tsdf_amd
    from tsdf_amd import esdf, synth
    cam = synth.camera(80, 60)
    small = synth.camera(S_W, S_H)
    frames = [synth.render(cam, k) for k in (0, 10, 20)]
    last = tsdf_amd.SE3(frames[-1]["q"], frames[-1]["t"])

    def in_front(z):
        p = last.Inverse().Apply(np.array([0.0, 0.0, z], np.float32))
        return np.round(p.astype(np.float64) / S_VOXEL).astype(np.int64)

    origin = tuple(int(v) for v in in_front(1.0) - np.array(S_DIMS) // 2)
    seed = in_front(0.3)
    rgb = np.zeros((60, 80, 3), np.uint8)
    e = make_engine(voxel=S_VOXEL, trunc=S_TRUNC, w=80, h=60)
    try:
        layer = esdf.free_layer(origin, S_DIMS)
        for f in frames:
            pose = tsdf_amd.SE3(f["q"], f["t"])
            e.integrate(rgb, f["depth"], None, None, cam.K, pose, 4.0)
            e.free_observe(layer, f["depth"], cam.K, pose, 4.0)
        field = e.free_apply(layer, e.distance_field(origin, S_DIMS))
        travel = e.travel_field(field, [seed], clearance2=4, unknown_free=False)
        fr = e.frontiers(field, travel, min_size=S_MIN)
        views, owner = esdf.view_candidates(fr, S_VOXEL, yaws=S_YAWS)
        chosen, gains, seen = esdf.next_views(e, field, views, small.K, S_W, S_H, 3, far=S_FAR)
    finally:
        e.close()
    lo = [(origin[a] - 0.3) * S_VOXEL for a in range(3)]
    hi = [(origin[a] + S_DIMS[a] - 1 + 0.3) * S_VOXEL for a in range(3)]
    cube = " ".join(f"{lo[a]:.6f} {hi[a]:.6f}" for a in range(3))
    frm = " ".join(f"{seed[a] * S_VOXEL:.6f}" for a in range(3))
    meta = [f"{S_VOXEL} {S_TRUNC} 13 4.0 80 60 {' '.join(repr(float(v)) for v in cam.K)} {len(frames)} {cube} 255 0.0399 {frm} "
            f"{S_MIN} {S_YAWS} 0 {S_W} {S_H} {' '.join(repr(float(v)) for v in small.K)} {S_FAR} 3"]
    for i, f in enumerate(frames):
        meta.append(" ".join(repr(float(v)) for v in list(np.asarray(f["q"], f32)) + list(np.asarray(f["t"], f32))))
        np.ascontiguousarray(f["depth"], f32).tofile(tmp_path / f"depth_{i}.bin")
    (tmp_path / "meta.txt").write_text("\n".join(meta) + "\n")
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    print("view_main:", r.stdout.strip(), "python:", len(views), chosen, gains)
    out = [int(x) for x in r.stdout.split()]
    assert len(chosen) >= 1 and out == [len(views), len(chosen)] + [x for pair in zip(chosen, gains) for x in pair]
    want = np.array([np.concatenate([v.q, v.t]) for v in views], f32)
    assert np.array_equal(np.fromfile(tmp_path / "out_views.bin", f32).reshape(-1, 7), want)
    assert np.array_equal(np.fromfile(tmp_path / "out_cluster.bin", np.int32), owner)
    assert np.array_equal(np.fromfile(tmp_path / "out_seen.bin", np.uint32).reshape(seen["bits"].shape), seen["bits"])
