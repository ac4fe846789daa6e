"""The gate-edge stream (tests/_sem_edges.py) really stands on every gate of the semantic update's
fast path, checked on the CPU oracle alone: otherwise the bit-for-bit GPU comparison on it
(tests/test_gpu_sem_edges.py) could pass vacuously. These are conditions on the test's input, not
tolerances; measured on the oracle: 19 093 - 25 405 voxels with 0 < p < 2^-39, 77 785 - 92 056 in
[2^-39, 1) other than 0.5, 3 117 at exactly 1, 13 241 NaN of 187 267 updates per frame, 21 383
voxels at the weight cap from frame 40 on, 509 blocks."""
import numpy as np

import _sem_edges as se


def test_stream_inputs_sit_on_the_pixel_gates():
    M, T, g = se.MAX_DEPTH, se.gate_depth(), se.GATE
    d = se.depth_bands()
    assert d.dtype == np.float32 and g == np.float32(2.0 ** -39)
    assert d[4] == T and d[7] == M and T < M
    assert np.nextafter(d[3], np.float32(np.inf)) == T and np.nextafter(T, np.float32(np.inf)) == d[5]
    assert np.nextafter(d[6], np.float32(np.inf)) == M
    w_new = (np.float32(1) - d / M) * np.float32(4)
    assert w_new[0] == 2 and w_new[1] == 1 and (w_new[2:] < 0.5).all() and w_new[7] == 0
    frames = list(se.frames(8))
    for fr in frames:
        assert fr["depth"].dtype == fr["ht"].dtype == fr["lt"].dtype == np.float32
        assert fr["depth"].shape == fr["ht"].shape == fr["lt"].shape == (se.H, se.W)
        assert np.array_equal(fr["depth"][::6, 0], d) and (fr["depth"] == fr["depth"][:, :1]).all()
    # every column band takes every class over eight frames; at, just below and just above the floor
    ht = np.stack([fr["ht"] for fr in frames])
    lt = np.stack([fr["lt"] for fr in frames])
    for c in range(0, se.W, 8):
        for r in (0, se.WEIGHT0_ROW):
            got = {(a, b) for a, b in zip(ht[:, r, c].tolist(), lt[:, r, c].tolist())}
            assert got == {(float(a), float(b)) for a, b in se.touch_classes(r >= se.WEIGHT0_ROW)}
    below, above = np.nextafter(g, np.float32(0)), np.nextafter(g, np.float32(1))
    assert (ht == g).any() and (ht == below).any() and (ht == above).any() and (lt == g).any()
    assert (lt[:, :se.WEIGHT0_ROW] == g).any() and not (lt[:, se.WEIGHT0_ROW:, :][ht[:, se.WEIGHT0_ROW:, :] == 1] == g).any()


def test_stream_stands_on_every_gate_on_the_oracle():
    g = se.GATE
    seen = []

    def each(f, ora):
        s = ora.stats()
        p, w = se.seen_prob(ora.dump())
        nan = np.isnan(p)
        q = np.where(nan, np.float32(0.5), p)
        tiny = int(((q > 0) & (q < g)).sum())
        fast = int(((q >= g) & (q < 1) & (q != 0.5)).sum())
        one = int((q == 1).sum())
        assert tiny >= 15000, (f, tiny)
        assert fast >= 60000, (f, fast)
        assert one >= 2000, (f, one)
        assert 0 < int(nan.sum()) <= 0.1 * s["last_num_updated"], (f, int(nan.sum()), s)
        seen.append((s["active_blocks"], int((w == 40).sum())))

    se.run_oracle(se.FRAMES, keep=(), each=each)
    assert len(seen) == se.FRAMES
    assert seen[-1][1] >= 15000, seen[-1]
    # the two weighted bands reach the cap at frames 20 and 40 (w_new 2 and 1), one after the other
    assert seen[18][1] == 0 and 0 < seen[19][1] < seen[39][1] and seen[38][1] == seen[19][1]
    assert seen[-1][0] == seen[0][0] > 400, seen[0]


def test_unit_frames_put_p_equal_one_under_weight_zero_updates():
    """unit_frames: after frame 0 p == 1 on weighted and on weight-0 voxels alike (measured: 21 383 and
    144 381); frame 1 turns exactly the weight-0 ones NaN (0 * logf(0)) and leaves the others at 1."""
    seen = []

    def each(f, ora):
        p, w = se.seen_prob(ora.dump())
        nan = np.isnan(p)
        one = np.where(nan, np.float32(0.5), p) == 1
        seen.append((int((one & (w > 0)).sum()), int((one & (w == 0)).sum()), int((nan & (w == 0)).sum()),
                     int((nan & (w > 0)).sum())))

    se.run_oracle(keep=(), each=each, source=se.unit_frames())
    (hot0, cold0, nan0, _), (hot1, cold1, nan1, _), last = seen
    assert hot0 >= 15000 and cold0 >= 100000 and nan0 > 0, seen
    assert hot1 == hot0 and cold1 == 0 and nan1 == nan0 + cold0, seen
    assert last == seen[1] and all(s[3] == 0 for s in seen), seen


def test_snapshots_reproduce_the_oracle_dumps():
    """The compact per-frame states the GPU tests compare against are the oracle's dumps, bit for bit."""
    from _oracle import OracleGrid
    cam = se.camera()
    snaps = se.run_oracle(3)
    ora = OracleGrid(se.VOXEL, se.TRUNC, se.BLOCK_BITS)
    try:
        for f, fr in enumerate(se.frames(3)):
            ora.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], float(se.MAX_DEPTH), cam.K, fr["q"], fr["t"])
            a, b = snaps[f].dump(), ora.dump()
            assert a.keys() == b.keys() and a["free"] == b["free"]
            for k in b:
                if k != "free":
                    assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
                    assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (f, k)
            assert snaps[f].stats() == ora.stats()
            assert "tsdf" not in snaps[f].dump(pool=False)
    finally:
        ora.close()
