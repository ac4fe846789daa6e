"""Tile pairs (csrc/tsdf_ingest.h ingest_tile): an ingest workgroup covers two horizontally adjacent
16x16 pixel tiles of a tile row, two pixels per thread, one LDS key set whose slots hold the key and a
pair-local candidate order. The oracle decides, bit for bit, at the smallest shapes where pairing can
go wrong: odd and partial tile columns, a pair with more distinct keys than one tile's set held, the
larger set of maxs > 3, and a sharded frame's tile-row slices with an odd column count. The pool
indices (entry_idx) pin the candidate orders, so the rebuilt global order is covered. 1280x720, which
the pairs brought inside the pipelined frame's size gate, is compared with the two-launch engine."""
import numpy as np
import pytest

from test_gpu_parity import compare
from test_gpu_pipeline import _engine

pytestmark = pytest.mark.gpu

MAXD = 4.0


def _check_frame(eng, ora, tag):
    s, so = eng.stats(), ora.stats()
    assert s["status"] == 0, (tag, s)
    for k in ("last_num_visible", "last_num_updated", "last_num_deleted", "active_blocks"):
        assert s[k] == so[k], (tag, k, s[k], so[k])
    compare(eng, ora, tag=tag)


# 48x36: 3x3 tiles, a pair plus a single tile per row, partial bottom row; 40x24: the right tile of the
# second pair half outside the image; 16x16 / 17x17: no right tile / a one-column right tile; 33x17
@pytest.mark.parametrize("pipeline", [True, False])
@pytest.mark.parametrize("W,H", [(48, 36), (40, 24), (16, 16), (17, 17), (33, 17)])
def test_odd_and_partial_tile_columns(W, H, pipeline):
    """6 frames of the synth stream, the whole state against the oracle after every frame."""
    import tsdf_amd
    from tsdf_amd import synth
    from _oracle import OracleGrid
    cam = synth.camera(W, H)
    eng = _engine(pipeline, 0.01, 0.04, max_width=W, max_height=H, num_block_bits=13)
    ora = OracleGrid(0.01, 0.04, 13)
    try:
        for f in range(6):
            fr = synth.render(cam, f)
            eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, tsdf_amd.SE3(fr["q"], fr["t"]), MAXD)
            ora.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], MAXD, cam.K, fr["q"], fr["t"])
            _check_frame(eng, ora, f"{W}x{H} pipeline={pipeline} frame {f}")
        assert ora.stats()["active_blocks"] > 0
    finally:
        eng.close()
        ora.close()


@pytest.mark.parametrize("W,H", [(48, 36), (40, 24)])
def test_odd_columns_back_to_back(W, H):
    """The same shapes with the frames back to back (2 cm voxels: carvings every frame), so that the
    pipelined launch's chained tiles tag found keys with their rebuilt orders and the carving
    re-inserts them; the state after the last frame against the oracle."""
    import tsdf_amd
    from tsdf_amd import synth
    from _oracle import OracleGrid
    cam = synth.camera(W, H)
    eng = _engine(True, 0.02, 0.08, max_width=W, max_height=H, num_block_bits=12)
    ora = OracleGrid(0.02, 0.08, 12)
    try:
        eng.profile_begin()
        deleted = 0
        for f in range(10):
            fr = synth.render(cam, 3 * f)
            eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, tsdf_amd.SE3(fr["q"], fr["t"]), MAXD)
            ora.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], MAXD, cam.K, fr["q"], fr["t"])
            deleted += ora.stats()["last_num_deleted"]
        compare(eng, ora, tag=f"{W}x{H} back to back")
        s = eng.stats()
        assert s["status"] == 0 and s["active_blocks"] == ora.stats()["active_blocks"], s
        assert eng.profile_end()["pipelined"] == 9
        assert deleted > 0
    finally:
        eng.close()
        ora.close()


def _random_frame(seed, W=64, H=48):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.3, MAXD, size=(H, W)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return rgb, depth


def _max_pair_keys(voxel, trunc, depth, K, q, t):
    """The largest count of distinct block keys in one tile pair (32x16 pixels), from below: the
    oracle's key listing of the pair's pixels alone on an empty volume (the fully visible keys of the
    pair's DDA, each once)."""
    from _oracle import OracleGrid
    H, W = depth.shape
    best = 0
    for y0 in range(0, H, 16):
        for x0 in range(0, W, 32):
            ora = OracleGrid(voxel, trunc, 15)
            try:
                d = np.zeros_like(depth)
                d[y0:y0 + 16, x0:x0 + 32] = depth[y0:y0 + 16, x0:x0 + 32]
                keys, _ = ora.shard_keys(d, K, q, t, MAXD, y0, y0 + 16)
            finally:
                ora.close()
            assert len({tuple(k) for k in keys.tolist()}) == len(keys)
            best = max(best, len(keys))
    return best


# 5 mm voxels: 3 cm truncation gives maxs = 3 (the pipelined frame's key set), 6 cm gives maxs = 5 (the
# larger set; such frames take the two launches either way)
@pytest.mark.parametrize("trunc,pipeline", [(0.03, True), (0.03, False), (0.06, True)])
def test_key_set_holds_a_pairs_worst_case(trunc, pipeline):
    """A 64x48 frame of independent uniform depths in [0.3 m, max depth]: nearly every DDA sample of a
    pair is a key of its own. First shown from the oracle: some pair holds more than 1,024 distinct
    keys, more than one tile's set had slots. Then two such frames against the oracle."""
    import tsdf_amd
    from tsdf_amd import synth
    from _oracle import OracleGrid
    voxel = 0.005
    cam = synth.camera(64, 48)
    frames = []
    for f in range(2):
        rgb, depth = _random_frame(1234 + f)
        _, (q, t) = synth.pose(f)
        frames.append((rgb, depth, q, t))
    n = _max_pair_keys(voxel, trunc, frames[0][1], cam.K, frames[0][2], frames[0][3])
    print(f"trunc {trunc}: most distinct keys in a tile pair >= {n}")
    assert n > 1024, n
    eng = _engine(pipeline, voxel, trunc, max_width=64, max_height=48, num_block_bits=15)
    ora = OracleGrid(voxel, trunc, 15)
    try:
        for f, (rgb, depth, q, t) in enumerate(frames):
            eng.integrate(rgb, depth, None, None, cam.K, tsdf_amd.SE3(q, t), MAXD)
            ora.integrate(rgb, depth, None, None, MAXD, cam.K, q, t)
            _check_frame(eng, ora, f"trunc {trunc} pipeline={pipeline} frame {f}")
        assert eng.stats()["status"] == 0
    finally:
        eng.close()
        ora.close()


@pytest.mark.parametrize("G", [2, 3])
def test_shard_slices_with_odd_tile_columns(G):
    """48x36 (3 tiles per row), the DDA split by tile rows over G shards of one volume on one device:
    the union of the shards equals the unsharded oracle, every shard its oracle shard."""
    from test_gpu_sharded import _run
    nblk, _, group = _run(G, 48, 36, 0.01, 0.04, 6, nb_bits=13, shard_bits=13, split=True)
    try:
        assert nblk > 100, nblk
    finally:
        group.close()


def test_1280x720_pipelined_equals_two_launches():
    """1280x720 (80 x 45 tiles: 40 pairs per row, a partial bottom row) is within the pipelined frame's
    size gate since the tile pairs: 8 frames back to back, pipelined against the two-launch engine the
    other tests pin to the oracle, the whole state bit for bit."""
    import torch

    import tsdf_amd
    from tsdf_amd import synth
    from test_gpu_pipeline import _same
    cam = synth.camera(1280, 720, synth.L515_FULL)
    K = tsdf_amd.CameraIntrinsics(*[float(v) for v in cam.K])
    n = 8
    fr = synth.render_torch(cam, list(range(n)), device="cuda")
    engs = [_engine(p, 0.005, 0.03, max_width=1280, max_height=720, num_block_bits=17) for p in (True, False)]
    try:
        for e in engs:
            e.profile_begin()
            for i in range(n):
                e.integrate(fr["rgb"][i], fr["depth"][i], fr["ht"][i], fr["lt"][i], K,
                            tsdf_amd.SE3(fr["q"][i], fr["t"][i]), MAXD)
            e.flush()
            torch.cuda.synchronize()
        p0, p1 = engs[0].profile_end(), engs[1].profile_end()
        assert p0["pipelined"] == n - 1 and p1["pipelined"] == 0, (p0, p1)
        _same(engs[0], engs[1], "1280x720")
    finally:
        for e in engs:
            e.close()
