"""The voxel update and the allocation against the oracle ON their geometric gates (csrc/tsdf_fuse.hip:
update_issue_pix / update_finish; csrc/tsdf_device.h: voxel_visible, round_quot_*, quot_for_cmp,
weight_round_cap), through every copy of the update.

The stream (tests/_geo_edges.py; tests/test_geo_edges_cpu.py shows on the oracle that it stands on every
gate) is dyadic, so its ties are real: voxels whose projection is exactly k + 0.5, -0.5, W - 0.5 and
H - 0.5; voxels behind the camera plane that are updated (no z > 0 test) and the 0 / 0 voxel at the
camera centre, updated from pixel (0, 0); block corners that project exactly onto column 0 / W - 1 and
row 0 / H - 1; sdf == -trunc (not updated) and sdf == trunc; wc and the colour average on k + 0.5, wc
above the cap; partially visible blocks whose lanes fall off the image. A wrong operator or rounding
mode at any of them changes some voxel, a counter or the hash table. Every comparison is bit for bit
(NaN == NaN), no tolerance: hash table, pool indices and free stack, tsdf, colour, weight, probability,
the counters, status 0, and the raycast images from both poses (rays that start inside allocated
blocks). The oracle runs the stream once per module; the tests only read its kept states.

The shard engines run the stream WITHOUT the seed blocks, against a second, unseeded oracle run: the
hash-level hook (tsdf_hash_allocate) resolves its keys with default frame parameters, whose shard
count is 0, so on a shard engine it would give every key voxels on every shard. Unseeded, the origin
blocks are missing, and with them the voxels with ph.z < 0, the 0 / 0 voxel and the quotients of exactly
-0.5 (all three counts are 0), and 1 297 of the 3 712 partially visible blocks; every other gate keeps
at least 65 % of its voxels (measured with _geo_edges.gates). The four single-engine tests hold them all.

What the stream guards: five one-token changes of the arithmetic, each built and run against this file
alone on an MI355X.
* sdf > neg_trunc -> >= (update_finish): all six tests fail, the eager one at frame 0 (last_num_updated
  102 192 against 102 183: the nine voxels with sdf == -trunc under the centre pixel).
* <= (W - 1) -> < (voxel_visible): all six fail; the eager one at frame 3 (last_num_visible 378 against
  382), the others on the hash table (blocks with a corner on column W - 1 are not allocated).
* half away -> rintf in round_quot_i2's fallback: all six fail, the eager one at frame 0
  (last_num_updated 102 414 against 102 183: a quotient of -0.5 lands on pixel 0, inside the image).
* ph.z >= 0 -> > 0 (voxel_visible): all six pass, and no input can tell the two apart: at ph.z == +-0
  both quotients are +-inf or NaN, so the u and v tests have already failed. The voxels with ph.z == 0
  that the stream holds (pose B's plane Z = 0, the 0 / 0 voxel among them) show just that.
* pred(1/2) -> 0.5f in the weight rounding (update_finish): all six pass. floor(RN(wc + 0.5)) and
  roundf(wc) differ at wc == pred(1/2) only, and no update reaches it: w_old is an integer and
  w_new = RN((1 - RN(d / max_depth)) * 4), where 1 - x for a float x in [1/2, 1) is a multiple of
  2^-24, so w_new below 1/2 is a multiple of 2^-22. On every reachable wc -- the ties k + 1/2, 0.5 and
  even k among them, which this stream holds by the hundred thousand -- both forms are exact; the
  constant matters only to weight_round_cap's stated domain, which tests/test_cpu_lib.py checks
  exhaustively.
"""
import numpy as np
import pytest

import _geo_edges as ge
from _shards import assert_union_equals
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

N = ge.FRAMES
MAXD = float(ge.MAX_DEPTH)
COUNTERS = ("last_num_visible", "last_num_updated", "last_num_deleted", "active_blocks")


@pytest.fixture(scope="module")
def oracle():
    """{frame: Snapshot of the oracle after it} for every frame; "raycast_A" / "raycast_B": its images."""
    return ge.run_oracle(N, raycast=True)


@pytest.fixture(scope="module")
def oracle_unseeded():
    return ge.run_oracle(N, keep=(N - 1,), seeds=False)


@pytest.fixture(scope="module")
def stream():
    return list(ge.frames(N))


@pytest.fixture(scope="module")
def device_stream(stream):
    """The frames as stacked device tensors (they stay alive while pipelined frames read them)."""
    import torch
    return {k: torch.from_numpy(np.stack([fr[k] for fr in stream])).cuda() for k in ("rgb", "depth")}


def _engine(seeds=True):
    import tsdf_amd
    eng = tsdf_amd.Engine(ge.VOXEL, ge.TRUNC, max_width=ge.W, max_height=ge.H, num_block_bits=ge.BLOCK_BITS)
    if seeds:
        eng.hash_allocate(ge.seed_keys())
    return eng


def _pose(fr):
    import tsdf_amd
    return tsdf_amd.SE3(fr["q"], fr["t"])


def _check(eng, snap, tag):
    s, so = eng.stats(), snap.stats()
    assert s["status"] == 0, (tag, s)
    for k in COUNTERS:
        assert s[k] == so[k], (tag, k, s[k], so[k])
    compare(eng, snap, tag=tag)


def test_eager_host_frames_every_frame(oracle, stream):
    """tsdf_integrate on host frames, the whole state and the counters compared after every frame (each
    read completes the frame: the two-launch update); then a raycast from each pose, whose rays start
    inside allocated blocks (pose B's at the camera-centre voxel of the origin blocks)."""
    import tsdf_amd
    eng = _engine()
    try:
        for f, fr in enumerate(stream):
            eng.integrate(fr["rgb"], fr["depth"], None, None, ge.K, _pose(fr), MAXD)
            _check(eng, oracle[f], f"frame {f}")
        for name in "AB":
            rgba, nrm = eng.raycast(ge.K, ge.W, ge.H, tsdf_amd.SE3(*ge.pose(name)), ge.RAY_DEPTH)
            rgba_o, nrm_o = oracle["raycast_" + name]
            assert (rgba_o[..., 3] == 255).mean() > 0.2, name
            np.testing.assert_array_equal(rgba, rgba_o, err_msg=f"pose {name}")
            np.testing.assert_array_equal(nrm, nrm_o, err_msg=f"pose {name}")
    finally:
        eng.close()


def test_eager_device_frames_back_to_back(oracle, stream, device_stream):
    """Device frames integrated back to back: pipelined k_frame launches, frame n's update beside frame
    n + 1's ingest under the other pose. Compared at frames 11 and 35 only (a read completes the pending
    frames)."""
    import torch
    eng = _engine()
    d = device_stream
    try:
        eng.profile_begin()
        for f, fr in enumerate(stream):
            eng.integrate(d["rgb"][f], d["depth"][f], None, None, ge.K, _pose(fr), MAXD)
            if f in (11, N - 1):
                torch.cuda.synchronize()
                _check(eng, oracle[f], f"frame {f}")
        assert eng.profile_end()["pipelined"] >= N - 4  # all but the first and the one after the read
    finally:
        eng.close()


@pytest.mark.parametrize("batch", [1, 4])
def test_graph_frames(oracle, stream, device_stream, batch):
    """The graph kernels' copy of the update: one captured launch per frame, or per four frames."""
    import torch
    eng = _engine()
    g = eng.frame_graph(ge.W, ge.H, batch=batch)
    d = device_stream
    try:
        for f, fr in enumerate(stream):
            g.frame(d["rgb"][f], d["depth"][f], None, None, ge.K, _pose(fr), MAXD)
        eng.synchronize()
        torch.cuda.synchronize()
        _check(eng, oracle[N - 1], f"graph batch {batch}")
    finally:
        g.close()
        eng.close()


@pytest.mark.parametrize("pipe", [False, True])
def test_shard_engines(oracle_unseeded, stream, pipe):
    """Two shard engines of the volume (the Raw update: range and w_new are computed inside pass 2, not
    by the ingest), as three-phase frames with the DDA split and as pipelined ones, without the seed
    blocks (module docstring): their union is the unseeded, unsharded oracle volume."""
    import tsdf_amd
    group = tsdf_amd.ShardGroup(2, ge.VOXEL, ge.TRUNC, max_width=ge.W, max_height=ge.H,
                                num_block_bits=ge.BLOCK_BITS, split=not pipe, pipe=pipe)
    snap = oracle_unseeded[N - 1]
    try:
        for fr in stream:
            group.integrate(fr["rgb"], fr["depth"], None, None, ge.K, _pose(fr), MAXD)
        st, so = group.stats(), snap.stats()  # (flushes the pipelined frames)
        assert all(s["status"] == 0 for s in st), st
        for k in COUNTERS:
            assert sum(s[k] for s in st) == so[k], (k, st, so)
        nblk = assert_union_equals([e.dump() for e in group.engines], snap.dump(), tag=f"pipe={pipe}")
        assert nblk == so["active_blocks"]
    finally:
        group.close()
