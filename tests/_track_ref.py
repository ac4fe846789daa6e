"""numpy restatements of the pose-tracking contract (include/disinfect_tsdf.h, DESIGN.md "Pose
tracking") for tests/test_gpu_surface.py, tests/test_gpu_icp.py and tests/test_gpu_icp_edges.py: the
raycast's surface maps from an engine dump, the per-pixel rules of one ICP linearisation, and the
Gauss-Newton loop around them.
Per-pixel arithmetic is float32 one operation at a time, as the kernels' (no contraction, IEEE
division and square root); sums, solve and pose update are float64."""
import math

import numpy as np

f32 = np.float32
VOXEL, TRUNC, NB_BITS, MAX_DEPTH = 0.01, 0.04, 13, 4.0


# ---- float32 helpers on (N,) component arrays: the expressions of csrc/tsdf_device.h ----
def cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot3(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def qrot(q, v):
    qv = (q[0], q[1], q[2])
    uv = cross3(qv, v)
    uv = tuple(c + c for c in uv)
    c = cross3(qv, uv)
    return tuple((v[i] + q[3] * uv[i]) + c[i] for i in range(3))


def se3_apply(q, t, v):
    r = qrot(q, v)
    return tuple(r[i] + t[i] for i in range(3))


def round_s16(f):
    """round_s16: roundf (half away from zero) and the saturating conversion, as an int64 array."""
    r = np.trunc(f + np.copysign(f32(0.5), f))
    r = np.where(np.abs(f) < f32(0.5), f32(0), r)
    return np.clip(np.nan_to_num(r, nan=0.0), -32768, 32767).astype(np.int64)


class Camera:
    """FrameParams of (K, pose): intrinsics_inv and world_T_cam as the host computes them."""

    def __init__(self, K, pose):
        import tsdf_amd
        self.fx, self.fy, self.cx, self.cy = (f32(v) for v in K)
        self.ifx, self.ify = f32(1) / self.fx, f32(1) / self.fy
        self.icx, self.icy = -self.cx * self.ifx, -self.cy * self.ify
        self.cq, self.ct = [f32(v) for v in pose.q], [f32(v) for v in pose.t]
        inv = tsdf_amd.SE3(pose.q, pose.t).Inverse()
        self.wq, self.wt = [f32(v) for v in inv.q], [f32(v) for v in inv.t]

    def pixel_ray(self, x, y):
        return (self.ifx * x.astype(f32) + self.icx * f32(1), self.ify * y.astype(f32) + self.icy * f32(1),
                np.ones(x.shape, f32))


class Blocks:
    """Voxel lookups of an engine dump (Retrieve: a missing block reads tsdf +1, prob 0, rgbw 0)."""

    def __init__(self, dump):
        live = np.flatnonzero(dump["entry_idx"] >= 0)
        code = self._encode(dump["entry_pos"][live, :3].astype(np.int64))
        order = np.argsort(code)
        self.code, self.pool = code[order], dump["entry_idx"][live][order].astype(np.int64)
        assert np.unique(self.code).size == self.code.size
        self.tsdf, self.prob, self.rgbw = dump["tsdf"], dump["prob"], dump["rgbw"]

    @staticmethod
    def _encode(b):
        b = b + (1 << 19)
        return (b[..., 0] << 40) | (b[..., 1] << 20) | b[..., 2]

    def voxel(self, p):
        """(present, flat voxel index) of int64 voxel coordinates p = (x, y, z)."""
        p = np.stack(p, -1)
        code = self._encode(p >> 3)
        i = np.minimum(np.searchsorted(self.code, code), self.code.size - 1)
        ok = self.code[i] == code
        l = p & 7
        return ok, self.pool[i] * 512 + l[..., 0] + 8 * l[..., 1] + 64 * l[..., 2]

    def sample(self, p):
        ok, vi = self.voxel(p)
        return np.where(ok, self.tsdf[np.where(ok, vi, 0)], f32(1)).astype(f32)


def surface(dump, K, W, H, pose, max_depth=MAX_DEPTH, voxel=VOXEL, trunc=TRUNC):
    """The maps of tsdf_raycast_surface by the contract: dict of point, normal, depth, prob, rgbw, plus
    hit_march (the march's hit mask, before the gradient test) and the steps marched."""
    B = Blocks(dump)
    P = Camera(K, pose)
    voxel, step = f32(voxel), f32(trunc) / f32(2)
    y, x = np.divmod(np.arange(W * H), W)
    pc = P.pixel_ray(x, y)
    s = np.sqrt(dot3(pc, pc))
    dw = qrot(P.wq, tuple(c / s for c in pc))
    sg = tuple(c * step / voxel for c in dw)
    max_step = int(np.ceil(f32(max_depth) / step))
    pos = tuple(np.full(W * H, P.wt[i] / voxel, f32) for i in range(3))
    n = W * H
    live = np.full(n, 1 < max_step)
    prev = np.where(live, B.sample(tuple(round_s16(c) for c in pos)), f32(1)).astype(f32)
    pos = tuple(pos[i] + sg[i] for i in range(3))
    hp = [np.zeros(n, f32) for _ in range(3)]
    hprev, hcur = np.ones(n, f32), np.zeros(n, f32)
    for _ in range(1, max_step):
        if not live.any():
            break
        cur = B.sample(tuple(round_s16(c) for c in pos))
        hit = live & (prev > 0) & (cur <= 0) & ((prev - cur).astype(np.float64) <= 1.5)
        for i in range(3):
            hp[i] = np.where(hit, pos[i], hp[i])
        hprev, hcur = np.where(hit, prev, hprev), np.where(hit, cur, hcur)
        live &= ~hit
        prev = cur
        pos = tuple(pos[i] + sg[i] for i in range(3))
    hit = np.full(n, 1 < max_step) & ~live
    assert all(a.dtype == f32 for a in (*hp, *sg, hprev, hcur))
    # the zero crossing
    with np.errstate(all="ignore"):
        p1 = tuple(hp[i] - sg[i] for i in range(3))
        t = hprev / (hprev - hcur)
        pw = tuple((p1[i] + t * sg[i]) * voxel for i in range(3))
        depth = se3_apply(P.cq, P.ct, pw)[2]
        # ray_shade's binary search and its voxel
        a, b = list(p1), list(hp)
        mid = [(a[i] + b[i]) / f32(2) for i in range(3)]
        while True:
            dd = tuple(a[i] - b[i] for i in range(3))
            go = hit & (dot3(dd, dd).astype(np.float64) > .1)
            if not go.any():
                break
            neg = B.sample(tuple(round_s16(c) for c in mid)) < 0
            for i in range(3):
                b[i] = np.where(go & neg, mid[i], b[i])
                a[i] = np.where(go & ~neg, mid[i], a[i])
                mid[i] = np.where(go, (a[i] + b[i]) / f32(2), mid[i])
        g = tuple(round_s16(c) for c in mid)
        ok, vi = B.voxel(g)
        vi = np.where(ok, vi, 0)
        prob = np.where(ok, B.prob[vi], f32(0)).astype(f32)
        rgbw = np.where(ok[:, None], B.rgbw[vi], np.uint8(0)).astype(np.uint8)
        e = np.eye(3, dtype=np.int64)
        nr = tuple(B.sample(tuple(g[j] + e[i, j] for j in range(3))) - B.sample(tuple(g[j] - e[i, j] for j in range(3)))
                   for i in range(3))
        nn = dot3(nr, nr)
        good = hit & (nn > 0) & (nn < np.inf)
        ln = np.sqrt(nn)
        normal = np.stack([np.where(good, nr[i] / ln, f32(0)) for i in range(3)], -1).astype(f32)
    assert nn.dtype == f32 and t.dtype == f32 and depth.dtype == f32
    point = np.stack([np.where(good, pw[i], f32(0)) for i in range(3)], -1).astype(f32)
    return dict(point=point.reshape(H, W, 3), normal=normal.reshape(H, W, 3),
                depth=np.where(good, depth, f32(0)).astype(f32).reshape(H, W),
                prob=np.where(good, prob, f32(0)).astype(f32).reshape(H, W),
                rgbw=np.where(good[:, None], rgbw, np.uint8(0)).reshape(H, W, 4),
                hit_march=hit.reshape(H, W), max_step=max_step)


def point_map_normals(model, K, pose):
    """tsdf_track's model normals (k_surface_normals): at a pixel whose four neighbours and itself have
    a surface, c = (p[v+1, u] - p[v-1, u]) x (p[v, u+1] - p[v, u-1]), turned to face the camera
    (c . (p - camera centre) <= 0) and divided by its length; zero elsewhere, where the length is zero
    or not finite, and where c is more than acos(0.3) off the viewing ray (a grazing surface, or a
    difference that spans a depth edge): (c . to)^2 < 0.3^2 (c . c) (to . to). float32 op by op."""
    pt = model["point"]
    H, W = pt.shape[:2]
    P = Camera(K, pose)
    has = (model["normal"] != 0).any(axis=-1)
    ok = np.zeros((H, W), bool)
    ok[1:-1, 1:-1] = has[1:-1, 1:-1] & has[1:-1, 2:] & has[1:-1, :-2] & has[2:, 1:-1] & has[:-2, 1:-1]
    out = np.zeros((H, W, 3), f32)
    with np.errstate(all="ignore"):
        dx = tuple(pt[1:-1, 2:, i] - pt[1:-1, :-2, i] for i in range(3))
        dy = tuple(pt[2:, 1:-1, i] - pt[:-2, 1:-1, i] for i in range(3))
        c = cross3(dy, dx)
        to = tuple(pt[1:-1, 1:-1, i] - P.wt[i] for i in range(3))
        dv = dot3(c, to)
        c = tuple(np.where(dv > 0, -a, a) for a in c)
        nn = dot3(c, c)
        good = ok[1:-1, 1:-1] & (nn > 0) & (nn < np.inf) & (dv * dv >= (f32(0.3) * f32(0.3)) * (nn * dot3(to, to)))
        ln = np.sqrt(nn)
        for i in range(3):
            out[1:-1, 1:-1, i] = np.where(good, c[i] / ln, f32(0))
    assert nn.dtype == f32
    return dict(point=pt, normal=out)


def icp_terms_full(depth, K, pose, model, model_K, model_pose, stride, max_dist, max_depth=MAX_DEPTH,
                   d_positive=True):
    """Every sample of the stride lattice in sample order (sample s is pixel (stride * (s % nsx),
    stride * (s // nsx))) by the per-pixel rules of tsdf_icp_linearize, computed in float32: dict of keep
    (n,) bool, J (n, 6) float64 and r (n,) float64 (float32 values; whatever the arithmetic gives where
    keep is false), um, vm (n,) int64 the model pixel read (0 where the sample is dropped before the
    read), u, v (n,) the depth pixel, nsx. d_positive=False leaves the gate d > 0 out: only for
    tests/test_icp_cases_cpu.py, to show which cases that gate alone decides."""
    H, W = depth.shape
    F, M = Camera(K, pose), Camera(model_K, model_pose)
    pt, nm = model["point"], model["normal"]
    Hm, Wm = pt.shape[:2]
    v, u = [a.reshape(-1) for a in np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")]
    d = depth[v, u].astype(f32)
    with np.errstate(all="ignore"):
        keep = (d <= f32(max_depth)) & ((d > 0) if d_positive else True)
        ray = F.pixel_ray(u, v)
        pc = (ray[0] * d, ray[1] * d, d)
        pw = se3_apply(F.wq, F.wt, pc)
        pm = se3_apply(M.cq, M.ct, pw)
        keep &= pm[2] > 0
        fu = np.rint(M.fx * (pm[0] / pm[2]) + M.cx)
        fv = np.rint(M.fy * (pm[1] / pm[2]) + M.cy)
        assert fu.dtype == f32 and pw[0].dtype == f32
        keep &= (fu >= 0) & (fu < f32(Wm)) & (fv >= 0) & (fv < f32(Hm))
        um, vm = np.where(keep, fu, 0).astype(np.int64), np.where(keep, fv, 0).astype(np.int64)
        q = tuple(pt[vm, um, i] for i in range(3))
        n = tuple(nm[vm, um, i] for i in range(3))
        keep &= (n[0] != 0) | (n[1] != 0) | (n[2] != 0)
        e = tuple(pw[i] - q[i] for i in range(3))
        keep &= dot3(e, e) <= f32(max_dist) * f32(max_dist)
        r = dot3(n, e)
        c = cross3(pw, n)
    assert r.dtype == f32 and c[0].dtype == f32
    return dict(keep=keep, J=np.stack([*c, *n], -1).astype(np.float64), r=r.astype(np.float64), um=um, vm=vm,
                u=u, v=v, nsx=len(range(0, W, stride)))


def icp_terms(depth, K, pose, model, model_K, model_pose, stride, max_dist, max_depth=MAX_DEPTH):
    """(J (n, 6) float64, r (n,) float64) of the kept pixels by the per-pixel rules of tsdf_icp_linearize,
    computed in float32."""
    t = icp_terms_full(depth, K, pose, model, model_K, model_pose, stride, max_dist, max_depth)
    return t["J"][t["keep"]], t["r"][t["keep"]]


def icp_lane_terms(J, r, keep):
    """The 29 double terms of every sample, (n, 29): the products of J and r as the kernel forms them
    (exact), +0.0 where the sample is gated."""
    J = np.where(keep[:, None], J, 0.0)
    r = np.where(keep, r, 0.0)
    cols = [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [J[:, i] * r for i in range(6)] + [r * r]
    return np.stack(cols + [keep.astype(np.float64)], -1)


def icp_tree(J, r, keep, nsamples):
    """The 29 sums by the documented addition tree (csrc/tsdf_track.hip, DESIGN.md "Pose tracking"), in
    float64: per lane the 29 terms (+0.0 where gated or past nsamples); per wave of 64 the xor butterfly
    over 32, 16, 8, 4, 2, 1 (a = a + a[lane ^ o]), lane 0's value; per workgroup of 256
    ((w0 + w1) + w2) + w3; then 32 runs of ceil(nwg / 32) consecutive workgroups, each added from 0.0
    in index order; then the runs from 0.0 in index order."""
    assert J.shape[0] == r.shape[0] == keep.shape[0] == nsamples
    nwg = (nsamples + 255) // 256
    a = np.zeros((nwg * 256, 29))
    a[:nsamples] = icp_lane_terms(J, r, keep)
    a = a.reshape(nwg, 4, 64, 29)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, lane ^ o]
    w = a[:, :, 0]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    ln = (nwg + 31) // 32
    runs = np.zeros((32, 29))
    for k in range(ln):  # the k-th workgroup of every run that has one
        g = np.arange(32) * ln + k
        ok = g < np.minimum(nwg, (np.arange(32) + 1) * ln)
        runs[ok] = runs[ok] + part[g[ok]]
    out = np.zeros(29)
    for c in range(32):
        out = out + runs[c]
    return out


def icp_sums_exact(J, r):
    """The 29 sums as math.fsum of the exact double terms, and the sum of |term| of each."""
    cols = [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [J[:, i] * r for i in range(6)] + [r * r]
    return (np.array([math.fsum(c) for c in cols] + [float(r.size)]),
            np.array([math.fsum(np.abs(c)) for c in cols] + [float(r.size)]))


# ---- the pose update (csrc/tsdf_track_host.h restated) ----
def quat_to_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat(m):
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = 2 * math.sqrt(1 + tr)
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = 2 * math.sqrt(1 + m[0, 0] - m[1, 1] - m[2, 2])
        q = [0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
    elif m[1, 1] > m[2, 2]:
        s = 2 * math.sqrt(1 + m[1, 1] - m[0, 0] - m[2, 2])
        q = [(m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
    else:
        s = 2 * math.sqrt(1 + m[2, 2] - m[0, 0] - m[1, 1])
        q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s, (m[1, 0] - m[0, 1]) / s]
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def so3_exp(w):
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if t < 1e-4:
        a, b = 1 - t * t / 6 + t ** 4 / 120, 0.5 - t * t / 24 + t ** 4 / 720
    else:
        a, b = math.sin(t) / t, (1 - math.cos(t)) / (t * t)
    return np.eye(3) + a * K + b * K @ K


def pose_update(pose, xi):
    """One iteration's update of the float pose cam_T_world, rounded to floats again."""
    import tsdf_amd
    R_cw = quat_to_R(pose.q)
    R_wc, p_wc = R_cw.T, -R_cw.T @ pose.t.astype(np.float64)
    E = so3_exp(xi[:3])
    R_wc, p_wc = E @ R_wc, E @ p_wc + xi[3:]
    return tsdf_amd.SE3(R_to_quat(R_wc.T).astype(f32), (-R_wc.T @ p_wc).astype(f32))


def track(eng, depth, K, guess, max_depth=MAX_DEPTH, levels=3, stride=(4, 2, 1), iterations=(4, 5, 10),
          max_dist=0.1, min_inliers=6, eps_rot=0.0, eps_trans=0.0, norms=None):
    """tsdf_track's loop in numpy: the model maps from the engine, the per-pixel rules above, float64
    sums, numpy.linalg.cholesky; after an update a level ends when |omega| <= eps_rot and |t| <= eps_trans
    (eps as floats, as the engine holds them), if either eps is greater than 0. Returns (pose, status,
    iterations, inliers, rmse); `norms`, a list, receives (level, |omega|, |t|) of every iteration."""
    H, W = depth.shape
    model = point_map_normals(eng.raycast_surface(K, W, H, guess, max_depth, maps=()), K, guess)
    est, done, inl, rmse = guess, 0, 0, 0.0
    eps_rot, eps_trans = float(f32(eps_rot)), float(f32(eps_trans))
    early = eps_rot > 0 or eps_trans > 0
    for l in range(levels):
        for _ in range(iterations[l]):
            J, r = icp_terms(depth, K, est, model, K, guess, stride[l], max_dist, max_depth)
            inl = r.size
            rmse = math.sqrt(float(r @ r) / inl) if inl else 0.0
            if inl < min_inliers:
                return est, 1, done, inl, rmse
            try:
                L = np.linalg.cholesky(J.T @ J)
            except np.linalg.LinAlgError:
                return est, 1, done, inl, rmse
            xi = -np.linalg.solve(L.T, np.linalg.solve(L, J.T @ r))
            if not np.isfinite(xi).all():
                return est, 1, done, inl, rmse
            est = pose_update(est, xi)
            done += 1
            nw, nt = math.sqrt(float(xi[:3] @ xi[:3])), math.sqrt(float(xi[3:] @ xi[3:]))
            if norms is not None:
                norms.append((l, nw, nt))
            if early and nw <= eps_rot and nt <= eps_trans:
                break
    return est, 0, done, inl, rmse


def pose_error(a, b):
    """(translation [m], rotation [rad]) between two cam_T_world poses, compared as world_T_cam."""
    Ra, Rb = quat_to_R(a.q).T, quat_to_R(b.q).T
    pa, pb = -Ra @ a.t.astype(np.float64), -Rb @ b.t.astype(np.float64)
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.linalg.norm(pa - pb)), float(math.acos(min(1.0, max(-1.0, c))))


# ---- the scene of the tests: test_gpu_mesh_indexed's camera and volume, frames 40-43 ----
def make_engine(**kw):
    import tsdf_amd
    return tsdf_amd.Engine(VOXEL, TRUNC, max_width=96, max_height=72, num_block_bits=NB_BITS, **kw)


def true_pose(f):
    import tsdf_amd
    from tsdf_amd import synth
    q, t = synth.pose(f)[1]
    return tsdf_amd.SE3(q, t)


def integrate_frames(eng, frames, poses=None):
    from tsdf_amd import synth
    cam = synth.camera(96, 72, synth.TUM_FR1)
    for k, f in enumerate(frames):
        fr = synth.render(cam, f, touch="complement")
        eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, poses[k] if poses else true_pose(f), MAX_DEPTH)
    return cam
