"""numpy restatement of the observed-free-space contract (include/disinfect_tsdf.h, DESIGN.md "Observed free
space") for tests/test_free_cpu.py and tests/test_gpu_free.py: free(points, frame), observe(layer, frame) and
apply. float32, one IEEE operation at a time: the projection in Eigen's order (_track_ref.se3_apply), the ray
lengths by the expression of _geo_edges.ray_lengths, f2i(roundf(.)) by _geo_edges._round_away (np.round is
half-to-even and wrong here). Not the GPU's algorithm: no culls, no pixel records, every voxel of the box.
A frame is dict(depth (H, W) f32, K (fx, fy, cx, cy), q xyzw, t, max_depth); a layer is what esdf.free_layer
makes (host words); masks are bool (nz, ny, nx)."""
import numpy as np

from _geo_edges import _round_away
from _track_ref import se3_apply

f32 = np.float32


def frame(depth, K, q, t, max_depth):
    return dict(depth=np.ascontiguousarray(depth, f32), K=np.asarray(K, f32), q=np.asarray(q, f32),
                t=np.asarray(t, f32), max_depth=f32(max_depth))


def ray_lengths(K, W, H):
    """img_depth_to_range_ of every pixel: |Kinv (u, v, 1)| in float32, the norm as a0 + (a1 + a2)."""
    K = np.asarray(K, f32)
    fx, fy = f32(1) / K[0], f32(1) / K[1]
    cx, cy = -K[2] * fx, -K[3] * fy
    x = fx * np.arange(W, dtype=f32)[None, :] + cx * f32(1)
    y = fy * np.arange(H, dtype=f32)[:, None] + cy * f32(1)
    return np.sqrt(x * x + (y * y + f32(1) * f32(1)))


def terms(points, fr, voxel, trunc):
    """Every quantity of the contract for global voxels `points` (..., 3) int: dict(uq, vq: the quotients, hx,
    hy, hz, u, v: the rounded pixel, inb: in image, d, valid, sdf, free)."""
    g = np.asarray(points, np.int64)
    K, depth = fr["K"], fr["depth"]
    H, W = depth.shape
    pw = tuple(g[..., a].astype(f32) * f32(voxel) for a in range(3))
    q, t = [f32(c) for c in fr["q"]], [f32(c) for c in fr["t"]]
    pc = se3_apply(q, t, pw)
    hx = K[0] * pc[0] + K[2] * pc[2]
    hy = K[1] * pc[1] + K[3] * pc[2]
    hz = pc[2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        uq, vq = hx / hz, hy / hz
        u, v = _round_away(uq), _round_away(vq)
        inb = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        img = np.where(inb, v * W + u, 0)
        d = depth.reshape(-1)[img]
        valid = inb & (d != 0) & (d <= fr["max_depth"])
        sdf = ray_lengths(K, W, H).reshape(-1)[img] * (d - hz)
        free = valid & (sdf >= f32(trunc)) & (hz > 0)
    return dict(uq=uq, vq=vq, hx=hx, hy=hy, hz=hz, u=u, v=v, inb=inb, d=d, valid=valid, sdf=sdf, free=free)


def free(points, fr, voxel, trunc):
    return terms(points, fr, voxel, trunc)["free"]


def box_points(origin, dims):
    """Global voxels (nz, ny, nx, 3) of a box."""
    nx, ny, nz = (int(v) for v in dims)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([x, y, z], -1).astype(np.int64) + np.asarray(origin, np.int64)


def frame_mask(origin, dims, fr, voxel, trunc):
    """free(., frame) over a box: bool (nz, ny, nx)."""
    return free(box_points(origin, dims), fr, voxel, trunc)


def pack(mask):
    """Layer words (nz, ny, ceil(nx / 32)) uint32 of a mask: voxel x is bit x & 31 of word x >> 5, padding 0."""
    nz, ny, nx = mask.shape
    wx = (nx + 31) // 32
    m = np.zeros((nz, ny, wx * 32), np.uint64)
    m[..., :nx] = mask
    return (m.reshape(nz, ny, wx, 32) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


def unpack(bits, nx):
    w = np.asarray(bits).view(np.uint32)
    m = (w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return m.reshape(w.shape[0], w.shape[1], -1)[..., :nx].astype(bool)


def padding(bits, nx):
    """The padding bits of every row's last word, ORed together."""
    w = np.asarray(bits).view(np.uint32)
    keep = nx - 32 * (w.shape[-1] - 1)
    return int(np.bitwise_or.reduce(w[..., -1].reshape(-1) >> np.uint32(keep))) if keep < 32 else 0


def observe(layer, fr, voxel, trunc):
    """bits |= free(., frame) on a host layer, in place; returns the frame's mask."""
    m = frame_mask(layer["origin"], layer["dims"], fr, voxel, trunc)
    layer["bits"] |= pack(m)
    return m


def apply(mask, layer_origin, state, origin):
    """(state with 0 -> 1 where the voxel lies in the layer's box and its bit is set, the number changed)."""
    state = np.asarray(state)
    nz, ny, nx = state.shape
    l = box_points(origin, (nx, ny, nz)) - np.asarray(layer_origin, np.int64)
    lz, ly, lx = mask.shape
    inside = ((l >= 0) & (l < np.array([lx, ly, lz]))).all(axis=-1)
    l = np.where(inside[..., None], l, 0)
    hit = inside & mask[l[..., 2], l[..., 1], l[..., 0]] & (state == 0)
    return np.where(hit, 1, state).astype(np.uint8), int(hit.sum())
