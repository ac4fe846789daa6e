"""The voxel update's and the allocation's geometric gate-edge stream (TEST INFRASTRUCTURE, numpy only).

The update (csrc/tsdf_fuse.hip: update_issue_pix / update_finish) and the visibility test
(csrc/tsdf_device.h: voxel_visible) compare and round: the projection rounds half away from zero, the
image test is on the rounded pixel, visibility is on the unrounded quotient against 0 and W - 1, the
sdf gate is a strict >, the weight and the colour round half away. Frames rendered from generic poses
never put a voxel ON one of those comparisons; this stream does, by making every quantity dyadic, so
that all float arithmetic on it is exact and a tie is a real tie:

* volume -- voxel 2^-7 m, truncation 2^-5 m (4 voxels), max_depth 1.0, 2^13 blocks;
* camera -- 64 x 48, K = (32, 32, 32, 24), rotation identity, two translations of cam_T_world: pose A
  t = 0 and pose B t = (0, 0, 4 voxels). With Z = gz (+ 4 under B) a voxel (gx, gy, gz) projects to
  u = 32 gx / Z + 32, v = 32 gy / Z + 24: a tie wherever 64 gx / Z is an odd integer. Under A the
  block corners at Z = 32 project exactly onto u = 0 / 63 and v = 0 / 47; under B the block row
  gz = -8..-1 straddles the camera plane (Z = -4..3, the camera centre at gz = -4);
* depth of frame f -- the plane PLAN[f % 12] (voxels) plus (((7u + 13v + f) % 9) - 4) / 2 voxels, the
  offset 0 at the pixels (u, v) = (32, 24), (8, 24), (56, 24), (32, 0), whose ray lengths are exactly
  1 and 1.25 (sdf is exact there); depth[5, 7] = 0, depth[40, 50] = max_depth, depth[41, 50] =
  succ(max_depth) (rows, columns). w_new = (1 - d) * 4 is 2, 3, 1, 0.5 at the planes 64, 32, 96, 112
  and 0 at 128 (or the pixel is beyond range);
* rgb -- seeded random per frame, so a wrong pixel or a wrong colour rounding changes bits; ht / lt
  None: the semantic chain keeps p = 0.5 (tests/_sem_edges.py is the stream for that half);
* seed blocks -- allocated through the hash-level hook before frame 0, blocks the DDA never creates
  (they are never fully visible): the eight blocks {-1, 0}^3 around the origin, and the ring around
  pose A's frustum at block z = 8 (x in {-9, 7} x y in -7..5, y in {-7, 5} x x in -8..6). Frame 0's
  64-voxel plane passes through the ring, so it survives carving.

gates() restates the projection and the update's conditions in float32 for exactly this setting and
counts the voxels on each gate; tests/test_geo_edges_cpu.py asserts with it, on the oracle alone, that
the stream stands on every gate. The GPU tests (tests/test_gpu_geo_edges.py) compare the engine with
the oracle bit for bit on the stream and never see the census.
"""
from __future__ import annotations

import types

import numpy as np

import _sem_edges as se

W, H = 64, 48
VOXEL, TRUNC = 2.0 ** -7, 2.0 ** -5
BLOCK_BITS = 13
FRAMES = 36
MAX_DEPTH = np.float32(1.0)
RAY_DEPTH = 2.0  # the raycasts' range
K = np.array([32, 32, 32, 24], np.float32)
Q = np.array([0, 0, 0, 1], np.float32)
T = {"A": np.zeros(3, np.float32), "B": np.array([0, 0, 4 * VOXEL], np.float32)}
PLAN = ((64, "A"), (6, "B"), (6, "A"), (32, "A"), (112, "A"), (96, "B"), (64, "A"), (112, "B"), (128, "A"),
        (32, "B"), (96, "A"), (64, "B"))
ZERO_OFFSET = ((32, 24), (8, 24), (56, 24), (32, 0))  # (u, v)

_F32 = np.float32


def camera():
    return types.SimpleNamespace(K=K, width=W, height=H)


def pose(name: str):
    """(q xyzw, t) float32: cam_T_world of pose "A" or "B"."""
    return Q, T[name]


def frames(n: int = FRAMES):
    """Yields n dicts(rgb HxWx3 u8, depth HxW f32, ht / lt None, q, t, pose "A" / "B")."""
    u, v = np.arange(W)[None, :], np.arange(H)[:, None]
    for f in range(n):
        plane, name = PLAN[f % len(PLAN)]
        off = ((7 * u + 13 * v + f) % 9) - 4
        for pu, pv in ZERO_OFFSET:
            off[pv, pu] = 0
        depth = ((plane + off / 2.0) * VOXEL).astype(_F32)  # dyadic: exact
        depth[5, 7] = 0
        depth[40, 50] = MAX_DEPTH
        depth[41, 50] = np.nextafter(MAX_DEPTH, _F32(np.inf))
        rgb = np.random.default_rng(7000 + f).integers(0, 256, (H, W, 3), dtype=np.uint8)
        yield dict(rgb=rgb, depth=np.ascontiguousarray(depth), ht=None, lt=None, q=Q, t=T[name], pose=name)


def origin_keys():
    return np.array([(x, y, z) for z in (-1, 0) for y in (-1, 0) for x in (-1, 0)], np.int16)


def ring_keys():
    side = [(x, y, 8) for x in (-9, 7) for y in range(-7, 6)]
    cap = [(x, y, 8) for y in (-7, 5) for x in range(-8, 7)]
    return np.array(side + cap, np.int16)


def seed_keys():
    """The seed blocks, in the order of the one hash-level Allocate launch that creates them."""
    return np.concatenate([origin_keys(), ring_keys()])


def live_keys(dump):
    """{(x, y, z)} of the blocks of a dump."""
    return set(map(tuple, dump["entry_pos"][dump["entry_idx"] >= 0, :3].tolist()))


class Snapshot(se.Snapshot):
    """_sem_edges.Snapshot for a stream whose hash table changes in every frame: the index arrays are
    kept as the entries that differ from the first kept dump (whole, they are 48 MB per frame)."""

    def __init__(self, dump, stats, base=None):
        super().__init__(dump, stats, base)
        if base is not None:
            self._sparse = {}
            for k, a in self._index.items():
                b = base._full[k]
                rows = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1)) if a is not b else np.zeros(0, np.int64)
                self._sparse[k] = (rows, a[rows].copy())
            self._index = None

    def dump(self, pool: bool = True):
        if self._base is None:
            return super().dump(pool)
        self._index = {}
        for k, (rows, vals) in self._sparse.items():
            a = self._base._full[k]
            if rows.size:
                a = a.copy()
                a[rows] = vals
            self._index[k] = a
        try:
            return super().dump(pool)
        finally:
            self._index = None


def run_oracle(n: int = FRAMES, keep=None, each=None, raycast=False, seeds=True):
    """The stream on the CPU oracle. seeds: the seed blocks first; keep: the frames whose state is kept
    (None: all) -> {frame: Snapshot}; each(frame index, frame, oracle) is called after every frame, and
    each(-1, None, oracle) before the first; raycast: also the oracle's (rgba, normal) from pose A and
    from pose B after the last frame, under "raycast_A" / "raycast_B"."""
    from _oracle import OracleGrid
    ora = OracleGrid(VOXEL, TRUNC, BLOCK_BITS)
    out, base = {}, None
    try:
        if seeds:
            ora.hash_allocate(seed_keys())
        if each is not None:
            each(-1, None, ora)
        for f, fr in enumerate(frames(n)):
            ora.integrate(fr["rgb"], fr["depth"], None, None, float(MAX_DEPTH), K, fr["q"], fr["t"])
            if each is not None:
                each(f, fr, ora)
            if keep is None or f in keep:
                out[f] = Snapshot(ora.dump(), ora.stats(), base)
                base = base or out[f]
        if raycast:
            for name in "AB":
                out["raycast_" + name] = ora.raycast(K, W, H, Q, T[name], RAY_DEPTH)
    finally:
        ora.close()
    return out


# ---------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------
def ray_lengths():
    """img_depth_to_range_ of every pixel (block_allocate_kernel): |Kinv (u, v, 1)| in float32, the
    3-vector norm as a0 + (a1 + a2)."""
    fx, fy = _F32(1) / K[0], _F32(1) / K[1]
    cx, cy = -K[2] * fx, -K[3] * fy
    x = fx * np.arange(W, dtype=_F32)[None, :] + cx * _F32(1)
    y = fy * np.arange(H, dtype=_F32)[:, None] + cy * _F32(1)
    return np.sqrt(x * x + (y * y + _F32(1)))


def _round_away(x):
    """f2i(roundf(x)) of a float32 array: half away from zero, NaN -> 0, saturating."""
    x = x.astype(np.float64)
    r = np.copysign(np.floor(np.abs(x) + 0.5), x)
    r = np.where(np.isnan(r), 0.0, np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1))
    return r.astype(np.int64)


def _on_half(x):
    """x is k + 0.5 exactly (float32; the subtraction is exact)."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & ((x - np.floor(x)) == _F32(0.5))


def _project(g, t):
    """(u, v) quotients and ph.z of grid points g (..., 3) under cam_T_world = (identity, t): with
    q = (0, 0, 0, 1) Eigen's _transformVector returns its argument unchanged, so pc = pw + t."""
    pc = g.astype(_F32) * _F32(VOXEL) + t
    hx = K[0] * pc[..., 0] + K[2] * pc[..., 2]
    hy = K[1] * pc[..., 1] + K[3] * pc[..., 2]
    hz = pc[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return hx / hz, hy / hz, hz, hx


def dda_ties(fr):
    """The number of DDA sample coordinates (block_allocate_kernel: start + i * step, in voxels) of one
    frame that sit exactly on k + 0.5 before roundf; counted, not a condition of the stream."""
    t = fr["t"].astype(_F32)
    fx, fy = _F32(1) / K[0], _F32(1) / K[1]
    pc = np.stack(np.broadcast_arrays(fx * np.arange(W, dtype=_F32)[None, :] + (-K[2] * fx) * _F32(1),
                                      fy * np.arange(H, dtype=_F32)[:, None] + (-K[3] * fy) * _F32(1), _F32(1)), -1)
    d = fr["depth"][..., None]
    live = (d[..., 0] != 0) & (d[..., 0] <= MAX_DEPTH)
    dw = pc / ray_lengths()[..., None]        # world_T_cam = (identity, -t): the direction is unchanged
    sw = (pc * d + (-t)) - dw * _F32(TRUNC)
    dg, pos = dw / _F32(VOXEL), sw / _F32(VOXEL)
    rg = _F32(2 * TRUNC) * dg
    steps = np.ceil(np.abs(rg).max(axis=-1) / _F32(8)).astype(np.int64)
    st = rg / np.maximum(steps.astype(_F32), _F32(1))[..., None]
    n = 0
    for i in range(int(steps.max()) + 1):
        n += int((_on_half(pos) & (live & (i <= steps))[..., None]).sum())
        pos = pos + st
    return n


_OFF = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1)  # [x, y, z]
_OFF = _OFF.transpose(2, 1, 0, 3).reshape(512, 3)  # index x + 8 y + 64 z
_CORNERS = np.array([((i & 1) * 7, ((i >> 1) & 1) * 7, ((i >> 2) & 1) * 7) for i in range(8)])


def gates(fr, before, after):
    """Counts, for one frame of the stream, the voxels on each geometric gate, from the oracle's dumps
    before and after it. The update list is restated as the partially visible blocks of before | after
    (a block born and carved within the frame is in neither dump: `new_blocks` then differs from the
    oracle's last_num_alloc, and `updated` from its last_num_updated); the state a voxel is updated from
    is the earlier dump's, or AquireBlock's for a block born in this frame.
    Of the updated voxels: u_tie / v_tie (quotient on k + 0.5), last_tie_updated (a tie that rounds onto
    the last column or row), behind (ph.z < 0), zero_over_zero, sdf_plus_trunc, wc_half (wc on k + 0.5;
    wc_half_even: k even), wc_is_half, wc_over_cap, colour_half (colour quotients on k + 0.5, per channel).
    Of all voxels of the listed blocks: minus_half / size_minus_half_in (a quotient of exactly -0.5 /
    W - 0.5 or H - 0.5, the other coordinate in the image), sdf_minus_trunc (valid depth, sdf == -trunc:
    not updated). Of the blocks: visible, partial (listed, not fully visible), corners_on_edge (visible
    corners exactly on column 0 / W - 1 or row 0 / H - 1), full_with_edge_corner."""
    t = fr["t"].astype(_F32)
    depth, rgb = fr["depth"].reshape(-1), fr["rgb"].reshape(-1, 3)
    eb = np.flatnonzero(before["entry_idx"] >= 0)
    ea = np.flatnonzero(after["entry_idx"] >= 0)
    pb, pa = before["entry_pos"][eb, :3].astype(np.int64), after["entry_pos"][ea, :3].astype(np.int64)
    code = lambda p: ((p[:, 0] + 32768) << 32) | ((p[:, 1] + 32768) << 16) | (p[:, 2] + 32768)
    new = ~np.isin(code(pa), code(pb))
    pos = np.concatenate([pb, pa[new]])
    old = np.zeros((pos.shape[0], 512, 4), np.uint8)  # AquireBlock: weight 0, colour defined as 0
    old[:pb.shape[0]] = before["rgbw"].reshape(-1, 512, 4)[before["entry_idx"][eb]]
    out = dict(new_blocks=int(new.sum()), blocks=int(pos.shape[0]))

    # ---- block visibility: the 8 corners against 0, W - 1, H - 1 and ph.z >= 0 (voxel_visible)
    cu, cv, cz, _ = _project(pos[:, None, :] * 8 + _CORNERS[None], t)
    with np.errstate(invalid="ignore"):
        cvis = (cu >= 0) & (cu <= _F32(W - 1)) & (cv >= 0) & (cv <= _F32(H - 1)) & (cz >= 0)
        cedge = cvis & ((cu == 0) | (cu == _F32(W - 1)) | (cv == 0) | (cv == _F32(H - 1)))
    part, full = cvis.any(axis=1), cvis.all(axis=1)
    out.update(visible=int(part.sum()), corners_on_edge=int(cedge.sum()),
               full_with_edge_corner=int((full & cedge.any(axis=1)).sum()), partial=int((part & ~full).sum()))

    # ---- the update of every voxel of the listed blocks (update_and_carve_test)
    pos, old = pos[part], old[part]
    uq, vq, hz, hx = _project(pos[:, None, :] * 8 + _OFF[None], t)
    u, v = _round_away(uq), _round_away(vq)
    u_in, v_in = (u >= 0) & (u < W), (v >= 0) & (v < H)
    inb = u_in & v_in
    img = np.where(inb, v * W + u, 0)
    d = depth[img]
    valid = inb & (d != 0) & (d <= MAX_DEPTH)
    with np.errstate(invalid="ignore"):
        sdf = ray_lengths().reshape(-1)[img] * (d - hz)
        upd = valid & (sdf > -_F32(TRUNC))
        w_old = old[..., 3].astype(_F32)
        w_new = (_F32(1) - d / MAX_DEPTH) * _F32(4)
        wc = w_old + w_new
        col = 0
        for ch in range(3):
            q = (old[..., ch].astype(_F32) * w_old + rgb[img, ch].astype(_F32) * w_new) / wc
            col += int((upd & _on_half(q)).sum())
        wc_half = upd & _on_half(wc)
        out.update(
            updated=int(upd.sum()),
            u_tie=int((upd & _on_half(uq)).sum()), v_tie=int((upd & _on_half(vq)).sum()),
            minus_half=int(((uq == _F32(-0.5)) & v_in).sum() + ((vq == _F32(-0.5)) & u_in).sum()),
            size_minus_half_in=int(((uq == _F32(W - 0.5)) & v_in).sum() + ((vq == _F32(H - 0.5)) & u_in).sum()),
            last_tie_updated=int((upd & ((uq == _F32(W - 1.5)) | (vq == _F32(H - 1.5)))).sum()),
            behind=int((upd & (hz < 0)).sum()),
            zero_over_zero=int((upd & (hx == 0) & (hz == 0)).sum()),
            sdf_minus_trunc=int((valid & (sdf == -_F32(TRUNC))).sum()),
            sdf_plus_trunc=int((upd & (sdf == _F32(TRUNC))).sum()),
            wc_half=int(wc_half.sum()), wc_half_even=int((wc_half & (np.floor(wc) % 2 == 0)).sum()),
            wc_is_half=int((upd & (wc == _F32(0.5))).sum()), wc_over_cap=int((upd & (wc > 40)).sum()),
            colour_half=col)
    return out
