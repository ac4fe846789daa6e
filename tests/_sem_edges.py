"""The semantic update's gate-edge stream (TEST INFRASTRUCTURE, numpy only).

The voxel update's fast semantic chain (csrc/tsdf_device.h: sem_pixel_fast / sem_voxel_fast) runs
where ht, lt lie in [2^-39, 1], d <= max_depth * 0.9999f and p lies in [2^-39, 1); every other voxel
takes sem_update_exact. This stream puts pixels and voxels ON those comparisons, frame after frame,
from one fixed pose (synth.pose(0)) of a 64 x 48 camera, 1 cm voxels, 4 cm truncation, max_depth =
float32(1.3), 2^12 blocks, constant grey rgb:

* depth -- eight bands of six rows, constant in time. With M = max_depth and T = RN(M * 0.9999f):
  0.5 M, 0.75 M (w_new 2 and 1: their voxels reach the weight cap of 40 at frames 20 and 40), then
  0.9 M, pred(T), T, succ(T), pred(M), M, whose w_new < 0.5 keeps the stored weight 0: every update
  there runs with w_old = 0 and a tiny wc (0 at d = M: the reference's own 0 / 0 = NaN);
* touch -- eight bands of eight columns; at frame f, column band c takes class (c + f) % 8 of
  (ht, lt), with g = 2^-39: (g, 1), (pred(g), 1), (1, g), (succ(g), pred(1)), (0.5, 0.5),
  (2^-20, 2^-19), (g, g), (1, 1). Class (1, g) drives p to exactly 1; in the weight-0 rows (12 and
  below) 0 * logf(0) would then turn every voxel NaN within eight frames, so there it is (1, 2^-23)
  (p just below 1, inside the fast range).

tests/test_sem_edges_cpu.py asserts on the oracle that the stream stands on every gate; the GPU
tests (tests/test_gpu_sem_edges.py) compare the engine with the oracle bit for bit on it.
"""
from __future__ import annotations

import numpy as np

W, H = 64, 48
VOXEL, TRUNC = 0.01, 0.04
BLOCK_BITS = 12
FRAMES = 45
MAX_DEPTH = np.float32(1.3)
GATE = np.float32(2.0 ** -39)  # the fast path's floor for ht, lt and p
WEIGHT0_ROW = 12               # first row of the six depth bands whose voxels keep weight 0

_F0, _F1, _INF = np.float32(0.0), np.float32(1.0), np.float32(np.inf)


def _pred(x):
    return np.nextafter(np.float32(x), -_INF)


def _succ(x):
    return np.nextafter(np.float32(x), _INF)


def gate_depth():
    """T = RN(max_depth * 0.9999f) in float, sem_pixel_fast's own product."""
    return np.float32(MAX_DEPTH * np.float32(0.9999))


def depth_bands():
    M, T = MAX_DEPTH, gate_depth()
    return np.array([np.float32(0.5) * M, np.float32(0.75) * M, np.float32(0.9) * M, _pred(T), T, _succ(T),
                     _pred(M), M], np.float32)


def touch_classes(weight0: bool):
    g = GATE
    third = (_F1, np.float32(2.0 ** -23)) if weight0 else (_F1, g)
    return np.array([(g, _F1), (_pred(g), _F1), third, (_succ(g), _pred(_F1)), (0.5, 0.5),
                     (2.0 ** -20, 2.0 ** -19), (g, g), (_F1, _F1)], np.float32)


def camera():
    from tsdf_amd import synth
    return synth.camera(W, H, synth.TUM_FR1)


def pose():
    """(q xyzw, t) float32: cam_T_world of every frame."""
    from tsdf_amd import synth
    return synth.pose(0)[1]


def frames(n: int = FRAMES):
    """Yields n dicts(rgb HxWx3 u8, depth / ht / lt HxW f32, q, t), as synth.render does."""
    q, t = pose()
    rgb = np.full((H, W, 3), 128, np.uint8)
    depth = np.ascontiguousarray(np.repeat(depth_bands(), H // 8)[:, None].repeat(W, 1), dtype=np.float32)
    rows = np.arange(H)[:, None]
    cband = (np.arange(W) // (W // 8))[None, :]
    tables = touch_classes(False), touch_classes(True)
    for f in range(n):
        cls = np.broadcast_to((cband + f) % 8, (H, W))
        ht = np.where(rows < WEIGHT0_ROW, tables[0][cls, 0], tables[1][cls, 0]).astype(np.float32)
        lt = np.where(rows < WEIGHT0_ROW, tables[0][cls, 1], tables[1][cls, 1]).astype(np.float32)
        yield dict(rgb=rgb, depth=depth, ht=np.ascontiguousarray(ht), lt=np.ascontiguousarray(lt), q=q, t=t)


def unit_frames():
    """Three frames on the same depth bands that put p == 1 under an update with w_old = 0, which the
    stream above avoids: every pixel (1, 2^-39), so p becomes exactly 1 everywhere; then (2^-39, 1),
    where the reference's chain gives 0 * logf(1 - 1) = 0 * -inf = NaN in the weight-0 rows and keeps
    p = 1 in the weighted ones; then (0.5, 0.5). Only sem_voxel_fast's p < 1 keeps those voxels off
    the fast chain, whose logarithm of 0 is a finite number."""
    base = next(iter(frames(1)))
    for h, l in ((_F1, GATE), (GATE, _F1), (np.float32(0.5), np.float32(0.5))):
        yield dict(base, ht=np.full((H, W), h, np.float32), lt=np.full((H, W), l, np.float32))


def seen_prob(dump):
    """(p, weight) of every voxel of the live blocks of a dump."""
    live = dump["entry_idx"][dump["entry_idx"] >= 0]
    return dump["prob"].reshape(-1, 512)[live], dump["rgbw"].reshape(-1, 512, 4)[live, :, 3]


class Snapshot:
    """An oracle state kept for later comparison, with OracleGrid's dump() / stats(): the dump is held
    as the blocks (and index arrays) that differ from the first kept dump, so 45 of them stay small."""

    _POOL = ("tsdf", "prob", "rgbw")

    def __init__(self, dump, stats, base=None):
        self._stats = dict(stats)
        self._base = base
        if base is None:
            self._full = dump
            return
        b = base._full
        self._index = {k: b[k] if np.array_equal(dump[k], b[k]) else dump[k] for k in ("entry_pos", "entry_idx", "heap")}
        self._free = dump["free"]
        rows = [dump[k].reshape(-1, 512 * (4 if k == "rgbw" else 1)) for k in self._POOL]
        brows = [b[k].reshape(r.shape) for k, r in zip(self._POOL, rows)]
        changed = np.zeros(rows[0].shape[0], bool)
        for r, br in zip(rows, brows):  # (as bits: NaN payloads and signed zeros count)
            changed |= (r.view(np.uint8) != br.view(np.uint8)).any(axis=1)
        self._blocks = np.flatnonzero(changed)
        self._rows = [r[self._blocks].copy() for r in rows]

    def stats(self):
        return dict(self._stats)

    def dump(self, pool: bool = True):
        if self._base is None:
            d = self._full
            return dict(d) if pool else {k: v for k, v in d.items() if k not in self._POOL}
        out = dict(self._index, free=self._free)
        if pool:
            for k, r in zip(self._POOL, self._rows):
                a = self._base._full[k].copy()
                a.reshape(-1, r.shape[1])[self._blocks] = r
                out[k] = a
        return out


def run_oracle(n: int = FRAMES, keep=None, each=None, raycast=False, source=None):
    """The stream (or the frames of `source`) on the CPU oracle. keep: the frames whose state is kept
    (None: all) -> {frame: Snapshot}; each(frame, oracle) is called after every frame; raycast: also
    the oracle's (rgba, normal) from the stream's pose after the last frame, under the key "raycast"."""
    from _oracle import OracleGrid
    cam = camera()
    ora = OracleGrid(VOXEL, TRUNC, BLOCK_BITS)
    out, base = {}, None
    try:
        for f, fr in enumerate(frames(n) if source is None else source):
            ora.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], float(MAX_DEPTH), cam.K, fr["q"], fr["t"])
            if each is not None:
                each(f, ora)
            if keep is None or f in keep:
                out[f] = Snapshot(ora.dump(), ora.stats(), base)
                base = base or out[f]
        if raycast:
            q, t = pose()
            out["raycast"] = ora.raycast(cam.K, W, H, q, t, 4.0)
    finally:
        ora.close()
    return out
