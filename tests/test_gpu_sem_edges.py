"""The semantic update's fast path against the oracle ON its gates (csrc/tsdf_device.h: sem_pixel_fast,
sem_voxel_fast), through every copy of the update.

The stream (tests/_sem_edges.py; tests/test_sem_edges_cpu.py shows on the oracle that it stands on
every gate) holds pixels with ht, lt at 2^-39, one ulp below and one ulp above, depths one ulp around
max_depth * 0.9999f and at max_depth itself, voxels whose p lies below 2^-39, just below 1 and at
exactly 1, updates with w_old = 0 and wc down to 4e-4 (and 0: NaN), and voxels at the weight cap. A
gate that compares with the wrong operator or the wrong constant sends such a voxel down the other
path; wherever the fast chain is not exact there, some bit differs. Every comparison is bit for bit
(NaN == NaN), no tolerance: hash table, tsdf, colour, weight, probability, counters, raycast images.
The oracle runs the stream once per module; the tests only read its kept states. A second, three-frame
stream (unit_frames) puts p == 1 under updates with w_old = 0, which the long stream avoids because the
NaN they give would spread over it.

The d == max_depth band also holds blocks whose every voxel's tsdf is NaN (wc = 0): the reference's
carving keeps such a block (its fminf reduction gives NaN, and NaN >= 0.9 is false), and so must the
engine -- the counters and the hash table compared here caught it carving them.

What the gates' constants guard (one-token changes tried against these tests): p < 1 -> p <= 1 fails
test_unit_probability_under_weight_zero_updates (90 588 voxels finite where the reference gives NaN);
2^-39 -> 2^-60 in sem_pixel_fast and max_depth * 0.9999f -> * 1.0f pass everything, and are still
exact: the expansions equal the IEEE divide while every residual is a normal float, far below 2^-40.
"""
import numpy as np
import pytest

import _sem_edges as se
from _shards import assert_union_equals
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

N = se.FRAMES
MAXD = float(se.MAX_DEPTH)
COUNTERS = ("last_num_visible", "last_num_updated", "last_num_deleted", "active_blocks")


@pytest.fixture(scope="module")
def oracle():
    """{frame: Snapshot of the oracle after it} for every frame, and "raycast": its images at the end."""
    return se.run_oracle(N, raycast=True)


@pytest.fixture(scope="module")
def stream():
    return list(se.frames(N))


@pytest.fixture(scope="module")
def device_stream(stream):
    """The frames as stacked device tensors (they stay alive while pipelined frames read them)."""
    import torch
    return {k: torch.from_numpy(np.stack([fr[k] for fr in stream])).cuda() for k in ("rgb", "depth", "ht", "lt")}


def _engine():
    import tsdf_amd
    return tsdf_amd.Engine(se.VOXEL, se.TRUNC, max_width=se.W, max_height=se.H, num_block_bits=se.BLOCK_BITS)


def _pose_K():
    import tsdf_amd
    q, t = se.pose()
    return tsdf_amd.SE3(q, t), se.camera().K


def _check(eng, snap, tag):
    s, so = eng.stats(), snap.stats()
    assert s["status"] == 0, (tag, s)
    for k in COUNTERS:
        assert s[k] == so[k], (tag, k, s[k], so[k])
    compare(eng, snap, tag=tag)


def test_eager_host_frames_every_frame(oracle, stream):
    """tsdf_integrate on host frames, the whole state and the counters compared after every frame (each
    read completes the frame: the two-launch update); then a raycast from the stream's pose, whose
    colour blends with p."""
    pose, K = _pose_K()
    eng = _engine()
    try:
        for f, fr in enumerate(stream):
            eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], K, pose, MAXD)
            _check(eng, oracle[f], f"frame {f}")
        rgba, nrm = eng.raycast(K, se.W, se.H, pose, 4.0)
        rgba_o, nrm_o = oracle["raycast"]
        assert (rgba_o[..., 3] == 255).mean() > 0.2  # the two weighted bands are hit
        np.testing.assert_array_equal(rgba, rgba_o)
        np.testing.assert_array_equal(nrm, nrm_o)
    finally:
        eng.close()


def test_eager_device_frames_back_to_back(oracle, device_stream):
    """Device frames integrated back to back: pipelined k_frame launches, frame n's update beside frame
    n + 1's ingest, which writes the pixel gate into the range's sign. Compared at frames 19 and 44
    only (a read would complete the pending frames)."""
    import torch
    pose, K = _pose_K()
    eng = _engine()
    d = device_stream
    try:
        eng.profile_begin()
        for f in range(N):
            eng.integrate(d["rgb"][f], d["depth"][f], d["ht"][f], d["lt"][f], K, pose, MAXD)
            if f in (19, N - 1):
                torch.cuda.synchronize()
                _check(eng, oracle[f], f"frame {f}")
        assert eng.profile_end()["pipelined"] >= N - 4  # all but the first and the one after the read
    finally:
        eng.close()


@pytest.mark.parametrize("batch", [1, 4])
def test_graph_frames(oracle, device_stream, batch):
    """The graph kernels' copy of the update: one captured launch per frame, or per four frames (the
    last, partly filled batch is launched by the read)."""
    import torch
    pose, K = _pose_K()
    eng = _engine()
    g = eng.frame_graph(se.W, se.H, batch=batch)
    d = device_stream
    try:
        for f in range(N):
            g.frame(d["rgb"][f], d["depth"][f], d["ht"][f], d["lt"][f], K, pose, MAXD)
        eng.synchronize()
        torch.cuda.synchronize()
        _check(eng, oracle[N - 1], f"graph batch {batch}")
    finally:
        g.close()
        eng.close()


def test_unit_probability_under_weight_zero_updates():
    """_sem_edges.unit_frames: p == 1 met by an update with w_old = 0 (NaN in the reference's chain, a
    finite number on the fast chain: only sem_voxel_fast's p < 1 decides) and with w_old > 0 (p stays
    1): host frames compared after every frame, device frames back to back compared at the end."""
    import torch
    pose, K = _pose_K()
    frames = list(se.unit_frames())
    ora = se.run_oracle(source=frames)
    eng, dev = _engine(), _engine()
    try:
        d = {k: torch.from_numpy(np.stack([fr[k] for fr in frames])).cuda() for k in ("rgb", "depth", "ht", "lt")}
        for f, fr in enumerate(frames):
            eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], K, pose, MAXD)
            _check(eng, ora[f], f"unit frame {f}")
            dev.integrate(d["rgb"][f], d["depth"][f], d["ht"][f], d["lt"][f], K, pose, MAXD)
        torch.cuda.synchronize()
        _check(dev, ora[len(frames) - 1], "unit frames, pipelined")
    finally:
        eng.close(), dev.close()


@pytest.mark.parametrize("pipe", [False, True])
def test_shard_engines(oracle, stream, pipe):
    """Two shard engines of the volume (the Raw update: the pixel gate and the logs are computed inside
    pass 2, not by the ingest), as three-phase frames and as pipelined ones: their union is the
    unsharded oracle volume."""
    import tsdf_amd
    pose, K = _pose_K()
    group = tsdf_amd.ShardGroup(2, se.VOXEL, se.TRUNC, max_width=se.W, max_height=se.H,
                                num_block_bits=se.BLOCK_BITS, split=not pipe, pipe=pipe)
    try:
        for fr in stream:
            group.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], K, pose, MAXD)
        st, so = group.stats(), oracle[N - 1].stats()  # (flushes the pipelined frames)
        assert all(s["status"] == 0 for s in st), st
        for k in ("last_num_visible", "last_num_updated", "active_blocks"):
            assert sum(s[k] for s in st) == so[k], (k, st, so)
        nblk = assert_union_equals([e.dump() for e in group.engines], oracle[N - 1].dump(), tag=f"pipe={pipe}")
        assert nblk == so["active_blocks"]
    finally:
        group.close()
