"""Helpers around Engine.distance_field (DESIGN.md "Distance field"), numpy only: the squared voxel
distances in metres, with a sign, a box around a set of points, and the clearance at world points.

A field is the dict Engine.distance_field returns (host arrays): d2 (nz, ny, nx) uint16, state (same shape,
0 unobserved / 1 free / 2 inside, or None), origin (x, y, z), dims (nx, ny, nz), max_dist, unknown.

With uv.tube_emitters a planner can reject a lamp pose before it irradiates from it: take the tube's
emitter positions, ask clearance() for them, and drop the pose when any distance is under the threshold
the arm needs or any state is 0 (the lamp would sit in space no frame has observed)."""
from __future__ import annotations

import numpy as np


def metres(field, voxel: float) -> np.ndarray:
    """sqrt(d2) * voxel as float32: the distance to the nearest site, saturated at max_dist * voxel."""
    return (np.sqrt(np.asarray(field["d2"]).astype(np.float32)) * np.float32(voxel)).astype(np.float32)


def signed(field, voxel: float) -> np.ndarray:
    """metres() with a sign: negative inside (state 2), and NaN at unobserved voxels (state 0) unless the
    field was built with unknown=True, where they are sites and read 0."""
    if field.get("state") is None:
        raise ValueError("signed: the field has no state (distance_field(..., state=True))")
    d, st = metres(field, voxel), np.asarray(field["state"])
    d = np.where(st == 2, -d, d).astype(np.float32)
    if not field.get("unknown", False):
        d[st == 0] = np.nan
    return d


def box_around(points, voxel: float, margin: float = 0.0):
    """(origin, dims) of the voxel box that covers the (n, 3) world points [m] and `margin` metres around
    them, as Engine.distance_field takes them. Pad by max_dist * voxel for distances that are the
    volume's own up to the cap."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if p.shape[0] == 0:
        raise ValueError("box_around: no points")
    lo = np.floor((p.min(axis=0) - margin) / voxel).astype(np.int64)
    hi = np.ceil((p.max(axis=0) + margin) / voxel).astype(np.int64)
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo + 1)


def voxel_of(points, voxel: float, sample_offset: float = 0.0) -> np.ndarray:
    """The library's nearest voxel of world points: round(p / voxel - sample_offset) per component in
    float32, half away from zero, as int64 (n, 3)."""
    f = np.asarray(points, np.float32).reshape(-1, 3) / np.float32(voxel) - np.float32(sample_offset)
    r = np.trunc(f + np.copysign(np.float32(0.5), f))
    r = np.where(np.abs(f) < np.float32(0.5), np.float32(0), r)
    return np.nan_to_num(r, nan=0.0).astype(np.int64)


def clearance(field, voxel: float, points, sample_offset: float = 0.0):
    """(distance [m] float32 (n,), state uint8 (n,)) at the voxel nearest to each world point (voxel_of);
    (0, 0) for a point outside the box: unknown, no clearance. Without a state array every point inside
    the box reads state 1."""
    v = voxel_of(points, voxel, sample_offset) - np.asarray(field["origin"], np.int64)
    nx, ny, nz = field["dims"]
    ok = np.all((v >= 0) & (v < np.array([nx, ny, nz])), axis=1)
    v = np.where(ok[:, None], v, 0)
    d2 = np.asarray(field["d2"])[v[:, 2], v[:, 1], v[:, 0]].astype(np.float32)
    dist = np.where(ok, np.sqrt(d2) * np.float32(voxel), np.float32(0)).astype(np.float32)
    if field.get("state") is None:
        st = np.ones(v.shape[0], np.uint8)
    else:
        st = np.asarray(field["state"])[v[:, 2], v[:, 1], v[:, 0]]
    return dist, np.where(ok, st, 0).astype(np.uint8)


def standoff_candidates(field, voxel: float, lo: float, hi: float, stride: int) -> np.ndarray:
    """Where a lamp may stand: the world positions [m] (k, 3) f32 of the free voxels (state 1) of a
    distance_field result whose clearance metres() lies in [lo, hi] and that lie on the lattice origin +
    stride * k of the box, in box order (z slowest, x fastest). Voxel v sits at v * voxel. With a field built
    with unknown=True unobserved space is a site, so the clearance is to it as well and no candidate
    stands in or next to it."""
    if field.get("state") is None:
        raise ValueError("standoff_candidates: the field has no state (distance_field(..., state=True))")
    if stride < 1:
        raise ValueError("standoff_candidates: stride >= 1")
    d = metres(field, voxel)
    ok = (np.asarray(field["state"]) == 1) & (d >= np.float32(lo)) & (d <= np.float32(hi))
    lat = np.zeros(ok.shape, bool)
    lat[::stride, ::stride, ::stride] = True
    z, y, x = np.nonzero(ok & lat)
    v = np.stack([x, y, z], -1).astype(np.int64) + np.asarray(field["origin"], np.int64)
    return (v.astype(np.float32) * np.float32(voxel)).astype(np.float32)


# ---- travel field (Engine.travel_field; DESIGN.md "Travel field") ----
# A travel is the dict Engine.travel_field returns (host arrays): cost (nz, ny, nx) uint32, 0xFFFFFFFF where
# unreached, origin, dims. These filter the output of standoff_candidates before tubes are built.
UNREACHED = 0xFFFFFFFF


def travel_metres(travel, voxel: float) -> np.ndarray:
    """cost / 3 * voxel as float32: the travel distance from the nearest seed, inf where unreached."""
    c = np.asarray(travel["cost"])
    m = (c.astype(np.float32) / np.float32(3)) * np.float32(voxel)
    return np.where(c == UNREACHED, np.float32(np.inf), m).astype(np.float32)


def reachable(travel, voxel: float, positions, max_travel=None, sample_offset: float = 0.0):
    """(mask bool (n,), travel [m] float32 (n,)) at the voxel nearest to each world position (voxel_of):
    whether it was reached, within max_travel metres when that is given, and how far it is from the nearest
    seed (inf where unreached). A position outside the box is unreachable."""
    v = voxel_of(positions, voxel, sample_offset) - np.asarray(travel["origin"], np.int64)
    nx, ny, nz = travel["dims"]
    ok = np.all((v >= 0) & (v < np.array([nx, ny, nz])), axis=1)
    v = np.where(ok[:, None], v, 0)
    c = np.asarray(travel["cost"])[v[:, 2], v[:, 1], v[:, 0]]
    ok = ok & (c != UNREACHED)
    m = np.where(ok, (c.astype(np.float32) / np.float32(3)) * np.float32(voxel), np.float32(np.inf)).astype(np.float32)
    if max_travel is not None:
        ok = ok & (m <= np.float32(max_travel))
    return ok, m


def path_points(travel, voxel: float, path) -> np.ndarray:
    """World positions [m] (k, 3) f32 of a path of Engine.travel_paths (box-local linear indices, target
    first), in travel order: the seed first, the target last. Voxel v sits at v * voxel."""
    p = np.asarray(path, np.int64).reshape(-1)[::-1]
    nx, ny, _ = travel["dims"]
    v = np.stack([p % nx, p // nx % ny, p // (nx * ny)], -1) + np.asarray(travel["origin"], np.int64)
    return (v.astype(np.float32) * np.float32(voxel)).astype(np.float32)


# ---- observed free space (Engine.free_observe / free_apply; DESIGN.md "Observed free space") ----
# A layer is a dict: bits (nz, ny, ceil(nx / 32)) -- numpy uint32 on the host, torch.int32 viewing the same bits
# on a device -- origin and dims of its box in global voxels. Voxel (x, y, z) of the box is bit x & 31 of
# bits[z, y, x >> 5].
def free_layer(origin, dims, device=False):
    """A cleared layer over the box origin (x, y, z), dims (nx, ny, nz): host words, or with device=True (or
    a torch device) a tensor on that GPU."""
    o, d = tuple(int(v) for v in origin), tuple(int(v) for v in dims)
    if len(o) != 3 or len(d) != 3 or min(d) < 1:
        raise ValueError("free_layer: origin and dims are three integers each, dims positive")
    shape = (d[2], d[1], (d[0] + 31) // 32)
    if device is False or device is None:
        bits = np.zeros(shape, np.uint32)
    else:
        import torch
        bits = torch.zeros(shape, dtype=torch.int32, device="cuda" if device is True else device)
    return dict(bits=bits, origin=o, dims=d)


def free_mask(layer) -> np.ndarray:
    """bool (nz, ny, nx): the voxels of the layer's box that were observed free."""
    b = layer["bits"]
    b = b.cpu().numpy() if hasattr(b, "is_cuda") else np.asarray(b)
    w = np.ascontiguousarray(b).view(np.uint32)
    nx = int(layer["dims"][0])
    m = (w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return m.reshape(w.shape[0], w.shape[1], -1)[..., :nx].astype(bool)


def free_fraction(layer) -> float:
    """The fraction of the box's voxels observed free."""
    m = free_mask(layer)
    return float(m.sum()) / float(m.size)


# ---- frontiers and components (Engine.frontiers / components; DESIGN.md "Frontiers and components") ----
def _host(a) -> np.ndarray:
    return a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)


def frontier_goals(fr, voxel: float):
    """World positions of the clusters of an Engine.frontiers result, voxel v at v * voxel: dict(goal (k, 3)
    float32: each cluster's cheapest voxel to travel to, centroid (k, 3) float32: float32(sum / size + origin)
    * voxel with the quotient in float64, metres (k,) float32: goal_key / 3 * voxel, the travel distance to
    the goal (0 without a travel field, inf for a key of 0xFFFFFFFF))."""
    c = fr["clusters"]
    nx, ny, _ = (int(v) for v in fr["dims"])
    o = np.asarray(fr["origin"], np.int64)
    g = c["goal"].astype(np.int64)
    v = np.stack([g % nx, g // nx % ny, g // (nx * ny)], -1).reshape(-1, 3) + o
    goal = (v.astype(np.float32) * np.float32(voxel)).astype(np.float32)
    mean = c["sum"].astype(np.float64).reshape(-1, 3) / np.maximum(c["size"], 1).astype(np.float64).reshape(-1, 1)
    centroid = ((mean + o.astype(np.float64)).astype(np.float32) * np.float32(voxel)).astype(np.float32)
    k = c["goal_key"]
    m = (k.astype(np.float32) / np.float32(3)) * np.float32(voxel)
    return dict(goal=goal, centroid=centroid, metres=np.where(k == UNREACHED, np.float32(np.inf), m).astype(np.float32))


def frontier_voxels(fr, k: int) -> np.ndarray:
    """The global voxels (m, 3) int64, x y z, of cluster k of an Engine.frontiers / components result (with
    `origin`; box-local without), in ascending linear index."""
    lab = _host(fr["label"])
    z, y, x = np.nonzero(lab == np.uint32(fr["clusters"]["label"][k]))
    return np.stack([x, y, z], -1).astype(np.int64) + np.asarray(fr.get("origin", (0, 0, 0)), np.int64)


# ---- view gain (Engine.view_gain; DESIGN.md "View gain") ----
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """cam_T_world (SE3) of a camera at `eye` looking at `target`: z forward, x right, y down, x horizontal with
    respect to `up`. An `up` (anti)parallel to the viewing direction is replaced by the world x axis, or the y
    axis when the camera looks along x. Float64 throughout, one operation at a time in the order of
    host/uv_dose.h look_at_pose, then rounded to float32: the two agree bit for bit."""
    import math
    from . import SE3
    e, t, u = ([float(np.float64(v)) for v in a] for a in (eye, target, up))
    f = [t[0] - e[0], t[1] - e[1], t[2] - e[2]]
    n = math.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])
    if not (n > 0.0 and math.isfinite(n)):
        raise ValueError("look_at: eye and target coincide (or are not finite)")
    f = [f[0] / n, f[1] / n, f[2] / n]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    r = cross(f, u)
    n = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if not n > 1e-9:
        r = cross(f, [1.0, 0.0, 0.0] if abs(f[0]) < 0.9 else [0.0, 1.0, 0.0])
        n = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    r = [r[0] / n, r[1] / n, r[2] / n]
    d = cross(f, r)
    # cam_R_world: rows right, down, forward; its quaternion by the largest of w, x, y, z (Shepperd)
    m = [r, d, f]
    tr = m[0][0] + m[1][1] + m[2][2]
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0
        q = [(m[2][1] - m[1][2]) / s, (m[0][2] - m[2][0]) / s, (m[1][0] - m[0][1]) / s, 0.25 * s]
    elif m[0][0] > m[1][1] and m[0][0] > m[2][2]:
        s = math.sqrt(1.0 + m[0][0] - m[1][1] - m[2][2]) * 2.0
        q = [0.25 * s, (m[0][1] + m[1][0]) / s, (m[0][2] + m[2][0]) / s, (m[2][1] - m[1][2]) / s]
    elif m[1][1] > m[2][2]:
        s = math.sqrt(1.0 + m[1][1] - m[0][0] - m[2][2]) * 2.0
        q = [(m[0][1] + m[1][0]) / s, 0.25 * s, (m[1][2] + m[2][1]) / s, (m[0][2] - m[2][0]) / s]
    else:
        s = math.sqrt(1.0 + m[2][2] - m[0][0] - m[1][1]) * 2.0
        q = [(m[0][2] + m[2][0]) / s, (m[1][2] + m[2][1]) / s, 0.25 * s, (m[1][0] - m[0][1]) / s]
    if q[3] < 0.0:
        q = [-q[0], -q[1], -q[2], -q[3]]
    tt = [-(m[a][0] * e[0] + m[a][1] * e[1] + m[a][2] * e[2]) for a in range(3)]
    return SE3(np.array(q, np.float64).astype(np.float32), np.array(tt, np.float64).astype(np.float32))


def view_candidates(fr, voxel: float, yaws: int = 8, pitch: float = 0.0):
    """Candidate camera poses for an Engine.frontiers result: at every cluster's goal (frontier_goals: its
    cheapest voxel to travel to), `yaws` poses turned about the world z axis, yaw 2 pi k / yaws from the world
    x axis, looking `pitch` radians above the horizon. Returns (views: list of SE3 cam_T_world, cluster (n,)
    int32: the index of the cluster each pose belongs to), cluster-major."""
    import math
    if yaws < 1:
        raise ValueError("view_candidates: yaws >= 1")
    goal = frontier_goals(fr, voxel)["goal"]
    pitch = float(np.float32(pitch))  # (a float, as host/uv_dose.h view_candidates takes it)
    views, owner = [], []
    for c in range(goal.shape[0]):
        e = [float(v) for v in goal[c]]
        for k in range(yaws):
            a = 2.0 * math.pi * float(k) / float(yaws)
            dirn = [math.cos(a) * math.cos(pitch), math.sin(a) * math.cos(pitch), math.sin(pitch)]
            views.append(look_at(e, [e[0] + dirn[0], e[1] + dirn[1], e[2] + dirn[2]]))
            owner.append(c)
    return views, np.asarray(owner, np.int32)


def next_views(engine, field, views, K, width: int, height: int, k: int, far: float = 3.0, step=None,
               miss_depth=None, seen=None, device: bool = False):
    """The greedy choice of up to k next views: each round Engine.view_gain scores every view against the
    layer `seen` (what the views chosen so far will observe; a cleared esdf.free_layer over the field's box
    when None), the largest gain wins (ties to the lowest index), and the winner's predicted depth image is
    committed into `seen` with Engine.free_observe (max_depth 2 far). Stops at gain 0. The margin is the
    engine's truncation, so each gain is exactly the number of unobserved voxels the commit adds. Returns
    (chosen: list of view indices, gains: list of int, seen)."""
    views = list(views)
    if seen is None:
        seen = free_layer(field["origin"], field["dims"], device=(f"cuda:{engine.device}" if device else False))
    chosen, gains, depth = [], [], None
    for _ in range(max(int(k), 0)):
        if not views:
            break
        r = engine.view_gain(field, views, K, width, height, far, step=step, miss_depth=miss_depth, seen=seen,
                             depth=depth is None, device=device)
        if depth is None:  # (the images depend on the state alone: one march serves every round)
            depth = r["depth"]
        g = r["gain"]
        i = int(np.argmax(g))  # (the first of the largest)
        if int(g[i]) <= 0:
            break
        engine.free_observe(seen, depth[i], K, views[i], 2.0 * float(far))
        chosen.append(i)
        gains.append(int(g[i]))
    return chosen, gains, seen
