"""The voxel update pair by pair (csrc/tsdf_fuse.hip update_finish, the Pairs form of k_frame / k_frame_g): a
lane's two voxel pairs go through the tsdf / colour / weight update and the semantic update one after the
other, the second pair's semantic chain reading what its own first pass still holds, both inside the
pair's "one of the two voxels is updated" region. What can go wrong is a pair reading the other pair's
values, a voxel of a half-updated pair getting or losing a result, an exact recomputation
(sem_update_exact) fed the wrong pair's operands, and a fresh block's state leaking into a listed one.

48x36 frames (the size of tests/golden/integrate_48x36*.npz), 2 cm voxels, compared voxel for voxel as
uint32 -- tsdf, probability, rgbw -- with the hash table, the heap and the counts against the CPU oracle,
through the pipelined frame kernel, the two-launch frames (TSDF_PIPELINE=0), the captured graph and a
2-shard volume (selected as in tests/test_gpu_update_stores.py). No tolerance: equality of bits.

Streams:
  u16z   four frames of the uint16 touch stream with exact zeros in ht and lt: voxels of either pair go to
         sem_update_exact and to NaN (asserted on the oracle: p == 0, p == 1 and NaN all occur).
  masks  four frames (the second one twice, so that the blocks it carves are allocated again by its
         repetition) whose depth is cut up so that a lane's four voxels are updated in every one of the 16
         combinations: a checkerboard of single-pixel holes, a block of holes, a region beyond max_depth, and
         a per-pixel depth offset of up to +-3 cm (more than a voxel, less than the truncation distance), so
         that next to the back of the truncation band neighbouring voxels fall in and out of the update with
         the pixel they project to. The fixture asserts on the oracle's per-voxel update set, on the CPU, that
         all 16 values of the lane mask occur -- "first pair only" (0b0011 and its parts) and "second pair
         only" (0b1100 and its parts) among them -- on blocks a frame lists and on blocks it creates, and that
         some block is carved by one frame and allocated again by the next, so a fresh record follows listed
         ones in one workgroup's work.

The update set is read from the weights: every valid depth of these frames is at most 3 m of max_depth =
4 m (asserted), so every update adds w_new = 4 (1 - d / 4) >= 1 to a weight far below its cap, and the
rounded weight grows with each update. A voxel of a listed block was updated by a frame exactly when its
weight byte changed in it, a voxel of a block the frame created exactly when its weight is not 0.
"""
import numpy as np
import pytest

from _shards import assert_union_equals, live_blocks
from test_gpu_pipeline import _engine

pytestmark = pytest.mark.gpu

W, H = 48, 36
VOXEL, TRUNC, BITS = 0.02, 0.08, 13
MAXD = 4.0
NFRAMES = 4
MASK_FRAMES = (0, 1, 1, 2)  # (frame 1 twice: what it carves, its repetition allocates again)
COUNTERS = ("last_num_visible", "last_num_updated", "last_num_deleted", "active_blocks")


def _frame(cam, f, stream):
    from tsdf_amd import synth
    if stream == "u16z":
        return synth.render(cam, f, touch="u16z")
    fr = synth.render(cam, f, touch="u16z")
    depth = fr["depth"].copy()
    v, u = np.mgrid[0:H, 0:W]
    k = (u * 73856093 ^ v * 19349663 ^ (f + 1) * 83492791).astype(np.uint32)
    off = ((k >> 3) % 61).astype(np.float32) * np.float32(0.001) - np.float32(0.03)  # -3 .. +3 cm, per pixel
    depth = np.where(depth > 0, depth + off, depth).astype(np.float32)
    depth[4:32, 4:30][((u + v) % 2 == 0)[4:32, 4:30]] = 0.0   # checkerboard of single-pixel holes
    depth[(k % 7 == 0) & (u >= 30)] = 0.0                      # scattered holes in the rest
    depth[12:18, 34:44] = 0.0                                  # a hole several blocks wide
    depth[0:4, 36:48] = np.float32(1.5 * MAXD)                 # beyond max_depth
    return dict(fr, depth=depth)


def _by_key(d):
    """{block position: pool index} of a dump's live blocks."""
    live = np.flatnonzero(d["entry_idx"] >= 0)
    return {tuple(int(x) for x in d["entry_pos"][i, :3]): int(d["entry_idx"][i]) for i in live}


def _lane_masks(upd):
    """upd: (..., 512) bool per voxel -> the 4-bit update mask of each of a block's 128 lanes."""
    b = upd.reshape(-1, 128, 4).astype(np.uint8)
    return (b[..., 0] | (b[..., 1] << 1) | (b[..., 2] << 2) | (b[..., 3] << 3)).reshape(-1)


def _build_case(stream):
    from tsdf_amd import synth
    from _oracle import OracleGrid
    cam = synth.camera(W, H)
    frames = [_frame(cam, f, stream) for f in (MASK_FRAMES if stream == "masks" else range(NFRAMES))]
    for fr in frames if stream == "masks" else ():  # (the weights tell the update set: see the module docstring)
        d = fr["depth"]
        valid = (d > 0) & (d <= MAXD)
        assert valid.any() and d[valid].max() <= 3.0, d[valid].max()
    ora = OracleGrid(VOXEL, TRUNC, BITS)
    stats, snaps = [], []
    try:
        for fr in frames:
            ora.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], MAXD, cam.K, fr["q"], fr["t"])
            stats.append(ora.stats())
            snaps.append(ora.dump())
    finally:
        ora.close()
    assert all(s["last_num_updated"] > 0 for s in stats)
    # the lane masks of listed and of fresh blocks, and the blocks carved by one frame and created again by the next
    listed = np.zeros(16, np.int64)
    fresh = np.zeros(16, np.int64)
    recreated = 0
    prev, prev_keys, carved_last = None, {}, set()
    for d in snaps:
        keys = _by_key(d)
        w = d["rgbw"].reshape(-1, 512, 4)[..., 3]
        old = [k for k in keys if k in prev_keys]
        new = [k for k in keys if k not in prev_keys]
        if old:
            upd = w[[keys[k] for k in old]] != prev["rgbw"].reshape(-1, 512, 4)[[prev_keys[k] for k in old], :, 3]
            listed += np.bincount(_lane_masks(upd), minlength=16)
        if new:
            fresh += np.bincount(_lane_masks(w[[keys[k] for k in new]] != 0), minlength=16)
        recreated += len(carved_last.intersection(new))
        carved_last = set(prev_keys) - set(keys) if prev is not None else set()
        prev, prev_keys = d, keys
    end = snaps[-1]
    live = end["entry_idx"][end["entry_idx"] >= 0]
    seen = end["prob"].reshape(-1, 512)[live][end["rgbw"].reshape(-1, 512, 4)[live, :, 3] > 0]
    return dict(cam=cam, frames=frames, stats=stats, expect=end, listed=listed, fresh=fresh, recreated=recreated,
                seen=seen)


@pytest.fixture(scope="module", params=["u16z", "masks"])
def case(request):
    c = _build_case(request.param)
    print(request.param, "lane masks, listed:", c["listed"].tolist(), "fresh:", c["fresh"].tolist(),
          "carved and created again:", c["recreated"])
    if request.param == "u16z":
        s = c["seen"]
        assert (s == 0).sum() > 0 and (s == 1).sum() > 0 and np.isnan(s).sum() > 0, \
            ((s == 0).sum(), (s == 1).sum(), np.isnan(s).sum())
    else:
        assert (c["listed"] > 0).all(), c["listed"].tolist()
        assert (c["fresh"] > 0).all(), c["fresh"].tolist()
        assert c["recreated"] > 0
    return c


def _pose(fr):
    import tsdf_amd
    return tsdf_amd.SE3(fr["q"], fr["t"])


def _check(eng, case, tag, frame=-1):
    s, so = eng.stats(), case["stats"][frame]
    assert s["status"] == 0, (tag, s)
    for x in COUNTERS:
        assert s[x] == so[x], (tag, x, s[x], so[x])
    if frame not in (-1, NFRAMES - 1):
        return
    a, b = eng.dump(), case["expect"]
    for x in ("entry_pos", "entry_idx", "heap"):
        assert np.array_equal(a[x], b[x]), f"{tag}: {x}"
    assert a["free"] == b["free"], tag
    live = b["entry_idx"][b["entry_idx"] >= 0]
    for x in ("tsdf", "prob", "rgbw"):
        ua = a[x].view(np.uint32).reshape(-1, 512)[live]
        ub = b[x].view(np.uint32).reshape(-1, 512)[live]
        bad = np.argwhere(ua != ub)
        assert bad.size == 0, f"{tag}: {x} differs in {bad.shape[0]} voxels, first (block, voxel) {bad[:4].tolist()}"


def _device_frames(case):
    import torch
    return {x: torch.from_numpy(np.stack([fr[x] for fr in case["frames"]])).cuda() for x in ("rgb", "depth", "ht", "lt")}


def test_two_launch_frames(case):
    """TSDF_PIPELINE=0 (k_integrate), host frames, the counts after every frame."""
    eng = _engine(False, VOXEL, TRUNC, max_width=W, max_height=H, num_block_bits=BITS)
    try:
        for f, fr in enumerate(case["frames"]):
            eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], case["cam"].K, _pose(fr), MAXD)
            _check(eng, case, f"two launches, frame {f}", f)
    finally:
        eng.close()


def test_pipelined_frames(case):
    """Device frames back to back: k_frame, every frame's update beside the next frame's ingest."""
    import torch
    eng = _engine(True, VOXEL, TRUNC, max_width=W, max_height=H, num_block_bits=BITS)
    d = _device_frames(case)
    try:
        eng.profile_begin()
        for f, fr in enumerate(case["frames"]):
            eng.integrate(d["rgb"][f], d["depth"][f], d["ht"][f], d["lt"][f], case["cam"].K, _pose(fr), MAXD)
        eng.flush()
        torch.cuda.synchronize()
        assert eng.profile_end()["pipelined"] >= 1
        _check(eng, case, "pipelined")
    finally:
        eng.close()


def test_graph_frames(case):
    """The captured frame (k_frame_g), one launch per frame."""
    import torch
    eng = _engine(True, VOXEL, TRUNC, max_width=W, max_height=H, num_block_bits=BITS)
    d = _device_frames(case)
    try:
        g = eng.frame_graph(W, H, batch=1)
        try:
            for f, fr in enumerate(case["frames"]):
                g.frame(d["rgb"][f], d["depth"][f], d["ht"][f], d["lt"][f], case["cam"].K, _pose(fr), MAXD)
            eng.synchronize()
            torch.cuda.synchronize()
            _check(eng, case, "graph")
        finally:
            g.close()
    finally:
        eng.close()


def test_shard_frames(case):
    """Two shards of the volume, three-phase frames (the Raw update): the union of the shards is the oracle's
    volume, block for block, the probability as bits."""
    import tsdf_amd
    cam = case["cam"]
    group = tsdf_amd.ShardGroup(2, VOXEL, TRUNC, max_width=W, max_height=H, num_block_bits=BITS, split=True)
    try:
        for fr in case["frames"]:
            group.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, _pose(fr), MAXD)
        st, so = group.stats(), case["stats"][-1]
        assert all(s["status"] == 0 for s in st), st
        for x in ("last_num_visible", "last_num_updated", "active_blocks"):
            assert sum(s[x] for s in st) == so[x], (x, st, so)
        dumps = [e.dump() for e in group.engines]
        assert assert_union_equals(dumps, case["expect"], tag="shards") == so["active_blocks"]
        want = live_blocks(case["expect"])
        for i, dmp in enumerate(dumps):  # (the probability as bits too: assert_union_equals takes NaN == NaN)
            for key, (_, _, p) in live_blocks(dmp).items():
                assert np.array_equal(p.view(np.uint32), want[key][2].view(np.uint32)), (i, key)
    finally:
        group.close()
