"""The voxel update's write-back (csrc/tsdf_fuse.hip update_finish): a lane stores its whole 16-B tsdf /
probability / rgbw vectors whenever one of its four voxels was updated, so the voxels it did NOT update
are written back from the registers they were loaded into. They must come back bit for bit.

The volume is seeded through tsdf_import_blocks so that every voxel the frames leave alone holds bits no
update produces: a NaN of its own payload in tsdf (positive and negative), 0, 1, -0 and a NaN payload in
the probability, arbitrary rgb and weight bytes. Three 48x36 frames follow whose depth has a rectangular
hole and scattered single-pixel holes (d = 0), a region beyond max_depth, and the truncation band's edge
behind every surface: lanes with no updated voxel, with some and with all four, and whole waves with none
(the fixture asserts each class from the oracle).

Which voxels the frames touch is read from the oracle alone: before the three frames every voxel of every
block is given weight 0 and a colour below 64 (ora_hash_assign), and the frames' colours are 128 and up;
an update with w_old = 0 sets the colour to the pixel's, and averages of colours >= 128 stay there, so a
voxel was touched exactly when its red byte ends >= 128. The expected volume is the oracle's with the
seeds laid over the untouched voxels of the blocks that existed when they were seeded (a block the frames
carve and allocate again is reset as a whole: its untouched voxels no longer hold the colours given, and
it gets no seed in the expected volume). NaN seeds go only where the oracle's |tsdf| >= 0.9 and never into
a block's first voxel: a block's carve minimum (fminf drops NaN, and some voxel stays a number) then
crosses 0.9 in the engine exactly when it does in the oracle.

Every comparison is on bits (uint32), no tolerance: tsdf, probability and rgbw of every voxel of every
live block, the hash table, the heap and the counts, through the pipelined frame kernel, the two-launch
frames (TSDF_PIPELINE=0) and the captured graph. The 2-shard volume (the Raw update) is compared as the
union of its shards, block for block by position (a union has no one table or heap), with the summed
counts after the last frame.
"""
import numpy as np
import pytest

from _shards import assert_union_equals, live_blocks
from test_gpu_pipeline import _engine

pytestmark = pytest.mark.gpu

W, H = 48, 36
VOXEL, TRUNC, BITS = 0.01, 0.04, 13
MAXD = 3.0
PRELUDE, FRAMES = (0, 1), (2, 3, 4)
COUNTERS = ("last_num_visible", "last_num_updated", "last_num_deleted", "active_blocks")


def _frame(cam, f, test):
    from tsdf_amd import synth
    fr = synth.render(cam, f)
    if test:
        depth = fr["depth"].copy()
        depth[8:20, 10:24] = 0.0                    # a hole several blocks wide
        depth[24:34:3, 2:46:5] = 0.0                # single-pixel holes
        depth[0:7, 30:48] = np.float32(1.5 * MAXD)  # beyond max_depth
        fr = dict(fr, depth=depth, rgb=np.maximum(fr["rgb"], 128).astype(np.uint8))
    return fr


def _records(dump, tsdf, prob, rgbw):
    """Block records (tsdf_import_blocks) of every live block of `dump` with the given pool contents."""
    live = np.flatnonzero(dump["entry_idx"] >= 0)
    recs = np.zeros((live.size, 16 + 6144), np.uint8)
    recs[:, :8].view(np.int16)[:, :3] = dump["entry_pos"][live, :3]
    pidx = dump["entry_idx"][live]
    recs[:, 16:16 + 2048] = tsdf.reshape(-1, 512)[pidx].view(np.uint8)
    recs[:, 16 + 2048:16 + 4096] = prob.reshape(-1, 512)[pidx].view(np.uint8)
    recs[:, 16 + 4096:] = rgbw.reshape(-1, 2048)[pidx]
    return recs


def _build_case():
    """The oracle's run: dict(cam, prelude, frames, seed (pool arrays at the seeding point), s0 (the oracle's
    dump there), expect (dump after the last frame, seeds laid over), stats (per frame), lanes)."""
    from tsdf_amd import synth
    from _oracle import OracleGrid
    cam = synth.camera(W, H)
    prelude = [_frame(cam, f, False) for f in PRELUDE]
    frames = [_frame(cam, f, True) for f in FRAMES]
    ora = OracleGrid(VOXEL, TRUNC, BITS)
    try:
        for fr in prelude:
            ora.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], MAXD, cam.K, fr["q"], fr["t"])
        d = ora.dump()
        live = np.flatnonzero(d["entry_idx"] >= 0)
        pidx = d["entry_idx"][live]
        # weight 0 and a colour below 64 (distinct-ish bytes) in every voxel of every block
        loc = np.arange(512)
        pts = (d["entry_pos"][live, None, :3].astype(np.int32) * 8 +
               np.stack([loc & 7, (loc >> 3) & 7, loc >> 6], -1)[None]).astype(np.int16).reshape(-1, 3)
        n = pts.shape[0]
        i = np.arange(n, dtype=np.uint32)
        low = np.stack([1 + (i * 7) % 63, (i * 13 + 5) % 64, (i * 29 + 11) % 64, np.zeros_like(i)], -1).astype(np.uint8)
        assert ora.hash_assign(pts, low) == 0
        s0 = ora.dump()
        stats, snaps = [], [s0]
        for fr in frames:
            ora.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], MAXD, cam.K, fr["q"], fr["t"])
            stats.append(ora.stats())
            snaps.append(ora.dump())
        end = snaps[-1]
    finally:
        ora.close()
    assert all(s["last_num_updated"] > 0 for s in stats)
    assert np.array_equal(s0["entry_idx"][live], pidx)
    seeded = np.zeros(s0["tsdf"].size // 512, bool)
    seeded[pidx] = True
    touched = end["rgbw"][:, 0] >= 128
    same = np.ones(touched.size, bool)
    for x in ("tsdf", "prob", "rgbw"):
        same &= s0[x].view(np.uint32).reshape(-1) == end[x].view(np.uint32).reshape(-1)
    free_vox = np.repeat(seeded, 512) & ~touched & same  # voxels of the seeded blocks the frames leave alone
    k = np.arange(free_vox.size, dtype=np.uint32)
    tsdf, prob, rgbw = (s0[x].copy() for x in ("tsdf", "prob", "rgbw"))
    far = free_vox & (np.abs(s0["tsdf"]) >= np.float32(0.9)) & (k % 512 != 0)
    tsdf.view(np.uint32)[far] = (0x7FC00000 | ((k & 1) << 31) | ((k * 2654435761) & 0x3FFFFF))[far]
    pbits = np.array([0x00000000, 0x3F800000, 0x80000000, 0x7FC12345], np.uint32)[k % 4] ^ ((k >> 2 & 0xFF) * (k % 4 == 3))
    prob.view(np.uint32)[free_vox] = pbits[free_vox]
    rgbw.view(np.uint32).reshape(-1)[free_vox] = ((k * 2246822519 + 374761393) & 0xFFFFFFFF)[free_vox]
    expect = dict(end)
    for name, arr in (("tsdf", tsdf), ("prob", prob), ("rgbw", rgbw)):
        e = end[name].copy()
        e[free_vox] = arr[free_vox]
        expect[name] = e
    # the classes of lanes the frames produce (a voxel whose bits changed in a frame was updated in it)
    lanes = {"none": 0, "some": 0, "all": 0, "idle_waves": 0}
    for a, b in zip(snaps[:-1], snaps[1:]):
        ch = ((a["tsdf"].view(np.uint32) != b["tsdf"].view(np.uint32)) | (a["rgbw"].view(np.uint32).reshape(-1) != b["rgbw"].view(np.uint32).reshape(-1)))
        ch = ch.reshape(-1, 2, 64, 4)[seeded]      # block, wave (z half), lane, voxel
        fv = free_vox.reshape(-1, 2, 64, 4)[seeded]
        listed = ch.any(axis=(1, 2, 3))            # blocks the frame surely updated
        c, f_ = ch[listed], fv[listed]
        lanes["all"] += int(c.all(-1).sum())
        lanes["some"] += int((c.any(-1) & f_.any(-1)).sum())
        lanes["none"] += int(f_.all(-1).sum())
        lanes["idle_waves"] += int(f_.all(axis=(2, 3)).sum())
    assert all(v > 0 for v in lanes.values()), lanes
    assert far.sum() > 1000 and (free_vox & ~far).sum() > 0, (far.sum(), free_vox.sum())
    return dict(cam=cam, prelude=prelude, frames=frames, seed=(tsdf, prob, rgbw), s0=s0, expect=expect, stats=stats,
                lanes=lanes)


@pytest.fixture(scope="module")
def case():
    return _build_case()


def _pose(fr):
    import tsdf_amd
    return tsdf_amd.SE3(fr["q"], fr["t"])


def _seed(eng, case):
    """The prelude through the engine itself (its table and heap are then the oracle's), the seeds over it."""
    cam = case["cam"]
    for fr in case["prelude"]:
        eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, _pose(fr), MAXD)
    before = eng.dump(pool=False)
    for x in ("entry_pos", "entry_idx", "heap"):
        assert np.array_equal(before[x], case["s0"][x]), x
    eng.import_blocks(_records(case["s0"], *case["seed"]))
    after = eng.dump()
    for x in ("entry_pos", "entry_idx", "heap"):
        assert np.array_equal(after[x], case["s0"][x]), f"{x} after the import"
    _pool_equal(after, dict(zip(("tsdf", "prob", "rgbw"), case["seed"])), case["s0"], "seeded")


def _pool_equal(a, b, table, tag):
    live = table["entry_idx"][table["entry_idx"] >= 0]
    for x in ("tsdf", "prob", "rgbw"):
        ua = a[x].view(np.uint32).reshape(-1, 512)[live]
        ub = b[x].view(np.uint32).reshape(-1, 512)[live]
        bad = np.argwhere(ua != ub)
        assert bad.size == 0, f"{tag}: {x} differs in {bad.shape[0]} voxels, first (block, voxel) {bad[:4].tolist()}"


def _check(eng, case, tag, frame=-1):
    s, so = eng.stats(), case["stats"][frame]
    assert s["status"] == 0, (tag, s)
    for x in COUNTERS:
        assert s[x] == so[x], (tag, x, s[x], so[x])
    if frame not in (-1, len(case["frames"]) - 1):
        return
    a, b = eng.dump(), case["expect"]
    for x in ("entry_pos", "entry_idx", "heap"):
        assert np.array_equal(a[x], b[x]), f"{tag}: {x}"
    assert a["free"] == b["free"], tag
    _pool_equal(a, b, b, tag)


def _device_frames(case):
    import torch
    return {x: torch.from_numpy(np.stack([fr[x] for fr in case["frames"]])).cuda() for x in ("rgb", "depth", "ht", "lt")}


def test_two_launch_frames(case):
    """TSDF_PIPELINE=0 (k_integrate), host frames, the counts after every frame."""
    eng = _engine(False, VOXEL, TRUNC, max_width=W, max_height=H, num_block_bits=BITS)
    try:
        _seed(eng, case)
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
        _seed(eng, case)
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
        _seed(eng, case)
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
    """Two shards of the volume, three-phase frames (the Raw update): every shard re-imports the seeds of the
    blocks it holds; the union of the shards is the expected volume, block for block."""
    import tsdf_amd
    cam = case["cam"]
    group = tsdf_amd.ShardGroup(2, VOXEL, TRUNC, max_width=W, max_height=H, num_block_bits=BITS, split=True)
    try:
        for fr in case["prelude"]:
            group.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, _pose(fr), MAXD)
        all_recs = _records(case["s0"], *case["seed"])
        by_key = {tuple(int(v) for v in r[:8].view(np.int16)[:3]): r for r in all_recs}
        held = 0
        for e in group.engines:
            mine = np.stack([by_key[k] for k in live_blocks(e.dump())])
            held += mine.shape[0]
            e.import_blocks(mine)
        assert held == all_recs.shape[0]
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
