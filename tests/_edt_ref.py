"""numpy restatement of the distance-field contract (include/disinfect_tsdf.h, DESIGN.md "Distance
field") for tests/test_edt_cpu.py and tests/test_gpu_edt.py: the voxels' classes and the site set from an
engine dump, with the neighbours read from the volume, and the exact squared Euclidean distance transform
as the plain separable min-plus -- along each axis the minimum over every offset of f[j] + (i - j)^2.
That is deliberately not the GPU's algorithm (bitmap scans, windowed passes with an early exit): it is the
definition of a separable squared distance, one line per axis. All integers."""
import numpy as np

from _track_ref import Blocks

INF = np.int64(1) << 40


def classes(dump, origin, dims, min_weight=1):
    """state (nz, ny, nx) uint8 of the box -- 0 unobserved, 1 free, 2 inside -- and the surface sites
    (bool): inside voxels with a free face neighbour, the neighbours looked up in the volume."""
    B = Blocks(dump)
    ox, oy, oz = (int(v) for v in origin)
    nx, ny, nz = (int(v) for v in dims)
    # the box grown by one voxel, (z, y, x) order
    z, y, x = np.meshgrid(np.arange(oz - 1, oz + nz + 1), np.arange(oy - 1, oy + ny + 1),
                          np.arange(ox - 1, ox + nx + 1), indexing="ij")
    ok, vi = B.voxel((x.astype(np.int64), y.astype(np.int64), z.astype(np.int64)))
    vi = np.where(ok, vi, 0)
    weight = B.rgbw.reshape(-1, 4)[vi, 3].astype(np.int64)
    tsdf = B.tsdf.reshape(-1)[vi]
    observed = ok & (weight >= min_weight)
    inside = observed & (tsdf <= 0)
    free = observed & ~inside
    c = (slice(1, -1),) * 3
    nfree = (free[1:-1, 1:-1, :-2] | free[1:-1, 1:-1, 2:] | free[1:-1, :-2, 1:-1] | free[1:-1, 2:, 1:-1] |
             free[:-2, 1:-1, 1:-1] | free[2:, 1:-1, 1:-1])
    state = np.where(inside[c], 2, np.where(free[c], 1, 0)).astype(np.uint8)
    return state, inside[c] & nfree


def min_plus(f, axis):
    """out[i] = min over j of f[j] + (i - j)^2 along `axis` (int64)."""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    out = f.copy()
    for d in range(1, n):
        dd = np.int64(d * d)
        np.minimum(out[d:], f[:-d] + dd, out=out[d:])
        np.minimum(out[:-d], f[d:] + dd, out=out[:-d])
    return np.moveaxis(out, 0, axis)


def transform(site, R):
    """min(R^2, squared distance to the nearest True of `site` (nz, ny, nx)) as uint16."""
    f = np.where(site, np.int64(0), INF)
    for axis in (2, 1, 0):
        f = min_plus(f, axis)
    return np.minimum(f, np.int64(R) * R).astype(np.uint16)


def distance_field(dump, origin, dims, max_dist=255, min_weight=1, unknown=False):
    """dict(d2, state, site) of the box by the contract."""
    state, site = classes(dump, origin, dims, min_weight)
    if unknown:
        site = site | (state == 0)
    return dict(d2=transform(site, max_dist), state=state, site=site)


# ---- volumes as block records (tsdf_import_blocks), and a dump of them without an engine ----
VOXEL, TRUNC, NB_BITS = 0.01, 0.04, 13
f32 = np.float32


def record(block, tsdf, weight, prob=0.5):
    """One block record: key, then tsdf / prob / rgbw of the 512 voxels given as (x, y, z)-indexed arrays."""
    rec = np.zeros(6160, np.uint8)
    rec[:8].view(np.int16)[:3] = block
    # voxel offset x + 8 y + 64 z: (z, y, x) order in memory
    rec[16:16 + 2048].view(f32)[:] = np.asarray(tsdf, f32).transpose(2, 1, 0).reshape(-1)
    rec[16 + 2048:16 + 4096].view(f32)[:] = np.broadcast_to(np.asarray(prob, f32), (8, 8, 8)).transpose(2, 1, 0).reshape(-1)
    rgbw = np.zeros((512, 4), np.uint8)
    rgbw[:, :3] = 128
    rgbw[:, 3] = np.asarray(weight).transpose(2, 1, 0).reshape(-1)
    rec[16 + 4096:].reshape(512, 4)[:] = rgbw
    return rec


def scene_records():
    """The analytic floor-and-box volume of the UV dose tests: 1 cm voxels, 4 cm truncation. The signed
    distance is the minimum of a floor whose zero crossing is at voxel z = -7.5 and a box x, y in
    [-4.5, 3.5], z in [-7.5, 8.5] (voxels), sampled in the voxel cube x, y in [-32, 32), z in [-16, 32):
    voxels with |sd| <= 4 cm hold clip(sd / 0.04, -1, 1) and weight 10, every other voxel of a block that
    holds such a voxel tsdf 1 and weight 0, and no other block exists."""
    lo, hi = np.array([-4.5, -4.5, -7.5]), np.array([3.5, 3.5, 8.5])
    x, y, z = np.meshgrid(np.arange(-32, 32), np.arange(-32, 32), np.arange(-16, 32), indexing="ij")
    g = np.stack([x, y, z], -1).astype(np.float64)
    q = np.abs(g - (lo + hi) / 2) - (hi - lo) / 2
    sb = np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(axis=-1), 0)
    sf = g[..., 2] + 7.5
    sd = np.minimum(sb, sf) * VOXEL
    near = np.abs(sd) <= TRUNC
    tsdf = np.where(near, np.clip(sd / TRUNC, -1, 1), 1.0).astype(f32)
    prob = np.where(sb <= sf, 0.9, 0.2).astype(f32)
    recs = []
    for bx in range(-4, 4):
        for by in range(-4, 4):
            for bz in range(-2, 4):
                sl = (slice(8 * bx + 32, 8 * bx + 40), slice(8 * by + 32, 8 * by + 40), slice(8 * bz + 16, 8 * bz + 24))
                if near[sl].any():
                    recs.append(record((bx, by, bz), tsdf[sl], np.where(near[sl], 10, 0), prob[sl]))
    return np.stack(recs)


def site_records(voxels):
    """One block per voxel of `voxels` (each in a block of its own, off the block's faces): the voxel
    inside (tsdf -0.5, weight 10), its six face neighbours free and observed (tsdf 1, weight 10), the
    block's other voxels unobserved (tsdf 1, weight 0)."""
    recs = []
    for v in voxels:
        v = np.asarray(v)
        l = v & 7
        assert ((l >= 1) & (l <= 6)).all()
        tsdf, w = np.ones((8, 8, 8), f32), np.zeros((8, 8, 8), np.int64)
        for a in range(3):
            for d in (-1, 1):
                n = l.copy()
                n[a] += d
                w[tuple(n)] = 10
        tsdf[tuple(l)], w[tuple(l)] = -0.5, 10
        recs.append(record(tuple(v >> 3), tsdf, w))
    return np.stack(recs)


def records_dump(recs):
    """What Engine.dump() holds for a volume of these records, as far as Blocks reads it (record i in pool
    block i)."""
    n = recs.shape[0]
    pos = np.zeros((n, 4), np.int16)
    pos[:, :3] = recs[:, :8].view(np.int16)[:, :3]
    return dict(entry_pos=pos, entry_idx=np.arange(n, dtype=np.int32),
                tsdf=np.ascontiguousarray(recs[:, 16:16 + 2048]).view(f32).reshape(-1),
                prob=np.ascontiguousarray(recs[:, 16 + 2048:16 + 4096]).view(f32).reshape(-1),
                rgbw=np.ascontiguousarray(recs[:, 16 + 4096:]).reshape(-1, 4))
