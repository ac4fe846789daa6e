"""Hand-built inputs that put tsdf_icp_linearize and tsdf_point_map_normals on their gates (TEST
INFRASTRUCTURE, numpy only). tsdf_icp_linearize takes caller-owned model maps, so none of this needs a
volume: the engine of the tests stays empty.

* onehot() -- a 23 x 17 depth frame, K = (64, 64, 11, 8), and a 12 x 9 model, K_m = (32, 32, 5.5, 4),
  both at the identity: 1 / fx and the rays are exact, and the model column is um = (u - 11) / 2 + 5.5 =
  u / 2, a tie at every odd column (rounding down at u = 1, 5, 9, ... and up at 3, 7, 11, ...), and vm
  = v / 2 likewise. Every model pixel holds its own point and a random normal, so reading a neighbour
  changes every entry of J and r. A frame with one pixel of that depth and zeros elsewhere must
  return that pixel's 29 terms exactly (x + 0.0 is exact at every level of the tree).
* gate_cases() -- one-hot twins on a 5 x 4 frame, kept against dropped, that differ in the gated
  quantity alone; probe() restates the intermediate values so that tests/test_icp_cases_cpu.py can
  assert, on the restatement alone, that an equality case stands ON the comparison.
* tree_case() -- frames of width 256 at stride 1 with H = nwg (a workgroup is a row), and two ragged
  ones, whose terms vary in sign and over about six decades, about a tenth of them gated.
* normals_case() and normals_rules() -- a 37 x 21 point map that shows both outcomes of every rule of
  k_surface_normals, and the census of which rule decides which pixel.
"""
from __future__ import annotations

import numpy as np

import _track_ref as ref

f32 = np.float32
IDENT = ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))


def se3(q=IDENT[0], t=IDENT[1]):
    import tsdf_amd
    return tsdf_amd.SE3(np.asarray(q, f32), np.asarray(t, f32))


def succ(x, toward=np.inf):
    return np.nextafter(f32(x), f32(toward))


# ---- one-hot frames ----
ONEHOT_W, ONEHOT_H, ONEHOT_K = 23, 17, (64.0, 64.0, 11.0, 8.0)
ONEHOT_WM, ONEHOT_HM, ONEHOT_KM = 12, 9, (32.0, 32.0, 5.5, 4.0)
ONEHOT_MAX_DIST = 1.0
ONEHOT_DEPTHS = (1.0, 2.0, 1.3)


def onehot():
    """dict of the full depth frame (every pixel at the depth its one-hot frame gives it: 1.0, 2.0 or
    1.3 by (u + 2 v) % 3), the cameras and the model. The model point of pixel (um, vm) is
    (0.05 um - 0.2, 0.05 vm - 0.15, 1.5) plus a seeded offset below 0.02: it encodes its pixel, and is
    within ONEHOT_MAX_DIST of every depth point that lands on it."""
    rng = np.random.default_rng(20261)
    v, u = np.mgrid[0:ONEHOT_H, 0:ONEHOT_W]
    depth = np.array(ONEHOT_DEPTHS, f32)[(u + 2 * v) % 3]
    vm, um = np.mgrid[0:ONEHOT_HM, 0:ONEHOT_WM]
    point = np.stack([0.05 * um - 0.2, 0.05 * vm - 0.15, np.full(um.shape, 1.5)], -1)
    point = (point + rng.uniform(-0.02, 0.02, point.shape)).astype(f32)
    normal = rng.uniform(0.2, 1.0, point.shape) * rng.choice([-1.0, 1.0], point.shape)
    normal = (normal / np.linalg.norm(normal, axis=-1, keepdims=True)).astype(f32)
    return dict(depth=depth, K=ONEHOT_K, pose=se3(), model=dict(point=point, normal=normal), model_K=ONEHOT_KM,
                model_pose=se3(), max_dist=ONEHOT_MAX_DIST, max_depth=ref.MAX_DEPTH)


def full_terms(c, stride=1, **kw):
    """ref.icp_terms_full of a case dict."""
    return ref.icp_terms_full(c["depth"], c["K"], c["pose"], c["model"], c["model_K"], c["model_pose"], stride,
                              c["max_dist"], c["max_depth"], **kw)


# ---- the gates at equality ----
# the dropped cases that the lower depth gate alone decides: the restatement without `d > 0` keeps them
GATES_WITHOUT_D_POSITIVE = ("d_negzero", "d_negative", "d_subnormal_negative")
GATE_W, GATE_H, GATE_K = 5, 4, (64.0, 64.0, 2.0, 1.0)
GATE_E = (0.01, -0.02, 0.03)  # model point - depth point of the plain case: inside the 0.25 gate


def _gate_case(d=1.0, px=(2, 1), Wm=6, Hm=4, Km=(32.0, 32.0, 2.25, 1.25), model_q=IDENT[0], model_t=IDENT[1],
               max_dist=0.25, max_depth=ref.MAX_DEPTH, near=None, offset=GATE_E, normal=None, point_nan=False,
               encode=True):
    """A one-hot 5 x 4 frame: depth d at pixel px (the default (2, 1) has the ray (0, 0, 1), so the model
    pixel is (cx_m, cy_m) whatever pm.z is). Every model pixel holds the depth point of depth `near`
    (default d) minus `offset`, plus (`encode`) 2^-10 (um + 8 vm) in x so that the pixel read shows, and a
    seeded normal (`normal` overrides all of them)."""
    rng = np.random.default_rng(7)
    depth = np.zeros((GATE_H, GATE_W), f32)
    depth[px[1], px[0]] = d
    F = ref.Camera(GATE_K, se3())
    ray = F.pixel_ray(np.array([px[0]]), np.array([px[1]]))
    nd = f32(d if near is None else near)
    pw = np.array([ray[0][0] * nd, ray[1][0] * nd, nd], f32)
    vm, um = np.mgrid[0:Hm, 0:Wm]
    point = np.broadcast_to(pw - np.array(offset, f32), (Hm, Wm, 3)).copy()
    if encode:
        point[..., 0] += (um + 8 * vm).astype(f32) * f32(2.0 ** -10)
    if point_nan:
        point[..., 0] = np.nan
    nrm = rng.uniform(0.2, 1.0, (Hm, Wm, 3)) * rng.choice([-1.0, 1.0], (Hm, Wm, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(f32)
    if normal is not None:
        nrm[...] = np.array(normal, f32)
    return dict(depth=depth, K=GATE_K, pose=se3(), model=dict(point=point.astype(f32), normal=nrm), model_K=Km,
                model_pose=se3(model_q, model_t), max_dist=max_dist, max_depth=max_depth, px=px)


def probe(c):
    """The intermediate float32 values of a one-hot case's pixel by the rules of tsdf_icp_linearize: d,
    pm (3,), fu_raw / fv_raw (before rint), fu / fv, n (3,), e2 = e . e, max_dist2 (NaN where an
    earlier value makes a later one meaningless is kept as computed)."""
    u, v = np.array([c["px"][0]]), np.array([c["px"][1]])
    F, M = ref.Camera(c["K"], c["pose"]), ref.Camera(c["model_K"], c["model_pose"])
    d = c["depth"][v, u].astype(f32)
    with np.errstate(all="ignore"):
        ray = F.pixel_ray(u, v)
        pw = ref.se3_apply(F.wq, F.wt, (ray[0] * d, ray[1] * d, d))
        pm = ref.se3_apply(M.cq, M.ct, pw)
        fu_raw, fv_raw = M.fx * (pm[0] / pm[2]) + M.cx, M.fy * (pm[1] / pm[2]) + M.cy
        fu, fv = np.rint(fu_raw), np.rint(fv_raw)
        Hm, Wm = c["model"]["point"].shape[:2]
        inside = (fu >= 0) & (fu < f32(Wm)) & (fv >= 0) & (fv < f32(Hm))
        um, vm = (int(fu[0]), int(fv[0])) if inside[0] else (0, 0)
        q, n = c["model"]["point"][vm, um], c["model"]["normal"][vm, um]
        e = tuple(pw[i] - q[i] for i in range(3))
        e2 = ref.dot3(e, e)
    assert fu_raw.dtype == f32 and e2.dtype == f32
    return dict(d=d[0], pm=np.array([a[0] for a in pm]), fu_raw=fu_raw[0], fv_raw=fv_raw[0], fu=fu[0], fv=fv[0],
                inside=bool(inside[0]), n=n, e2=e2[0], max_dist2=f32(c["max_dist"]) * f32(c["max_dist"]))


def gate_cases():
    """name -> (case, kept, twin, gated): `twin` names the case that differs in the gated quantity alone
    (None: the plain case "plain" is the twin), `gated` the probe() key that differs."""
    md = 3.7  # a max_depth that is no power of two
    sub = f32(1e-40)
    assert 0 < sub < np.finfo(f32).tiny
    tiny = f32(2.0 ** -100)
    C = {}
    C["plain"] = (_gate_case(), True, None, None)
    # d
    C["d_eq_max"] = (_gate_case(d=f32(md), px=(4, 3), max_depth=md), True, "d_above_max", "d")
    C["d_above_max"] = (_gate_case(d=succ(md), near=f32(md), px=(4, 3), max_depth=md), False, "d_eq_max", "d")
    # d > 0 alone decides these: the model lies at the point the bad depth produces (the camera centre for
    # -0, 1 m behind the camera for -1) and the model camera stands back along z, so pm.z > 0, the model
    # pixel is (cx_m, cy_m) and e is inside the gate; GATES_WITHOUT_D_POSITIVE keeps each of them. The kept
    # twins differ in the depth alone: 2^-100 on the model at the centre, +1 on the model at z = -1 (2 m
    # away, inside a 2.5 m gate).
    C["d_negzero"] = (_gate_case(d=f32(-0.0), near=0.0, model_t=(0, 0, 1.0)), False, "d_tiny_positive", "d")
    C["d_tiny_positive"] = (_gate_case(d=tiny, near=0.0, model_t=(0, 0, 1.0)), True, "d_negzero", "d")
    C["d_negative"] = (_gate_case(d=f32(-1.0), near=-1.0, model_t=(0, 0, 2.0), max_dist=2.5), False, "d_positive_far",
                       "d")
    C["d_positive_far"] = (_gate_case(d=f32(1.0), near=-1.0, model_t=(0, 0, 2.0), max_dist=2.5), True, "d_negative",
                           "d")
    # a subnormal depth is > 0: the header keeps it (the model lies at its point). A build that flushes
    # subnormals to zero would drop it.
    C["d_subnormal"] = (_gate_case(d=sub, near=sub, model_t=(0, 0, 1.0)), True, "d_subnormal_negative", "d")
    C["d_subnormal_negative"] = (_gate_case(d=-sub, near=sub, model_t=(0, 0, 1.0)), False, "d_subnormal", "d")
    # (a NaN fails every later comparison too: no input can leave the d gate alone to decide it)
    C["d_nan"] = (_gate_case(d=f32(np.nan), near=1.0), False, None, "d")
    # pm.z: the model camera moved back by d (pm.z == 0), by d / 2 (kept), and turned half round about y.
    # pmz_negative is the case that pins pm.z > 0. pmz_zero cannot tell it from pm.z >= 0: with pm.z == 0
    # the projection is 0 / 0 or x / 0, NaN or inf, and the inside-the-map test drops the pixel anyway, by
    # the arithmetic of any input. It shows only that a zero pm.z comes out as count 0.
    C["pmz_half"] = (_gate_case(model_t=(0, 0, -0.5)), True, "pmz_zero", "pm")
    C["pmz_zero"] = (_gate_case(model_t=(0, 0, -1.0)), False, "pmz_half", "pm")
    C["pmz_negative"] = (_gate_case(model_q=(0, 1, 0, 0)), False, None, "pm")
    # um, vm: the pixel's ray is (0, 0, 1), so the unrounded model pixel is (cx_m, cy_m)
    for ax, n_even, n_odd in (("u", 6, 7), ("v", 4, 5)):
        def km(x, ax=ax):
            return (32.0, 32.0, float(x), 1.25) if ax == "u" else (32.0, 32.0, 2.25, float(x))

        def size(n, ax=ax):
            return dict(Wm=n) if ax == "u" else dict(Hm=n)
        g = "f%s_raw" % ax
        C[ax + "m_minus_half"] = (_gate_case(Km=km(-0.5)), True, ax + "m_below_minus_half", g)  # rint -> -0
        C[ax + "m_below_minus_half"] = (_gate_case(Km=km(succ(-0.5, -np.inf))), False, ax + "m_minus_half", g)
        C[ax + "m_minus_0.3"] = (_gate_case(Km=km(f32(-0.3))), True, ax + "m_minus_0.6", g)  # rint -> -0
        C[ax + "m_minus_0.6"] = (_gate_case(Km=km(f32(-0.6))), False, ax + "m_minus_0.3", g)
        # the map's far edge: exactly on it; a tie that goes out (even size) and one that stays in (odd)
        C[ax + "m_eq_size"] = (_gate_case(Km=km(n_even), **size(n_even)), False, ax + "m_last", g)
        C[ax + "m_last"] = (_gate_case(Km=km(n_even - 1), **size(n_even)), True, ax + "m_eq_size", g)
        C[ax + "m_even_tie_out"] = (_gate_case(Km=km(n_even - 0.5), **size(n_even)), False, ax + "m_even_below_tie", g)
        C[ax + "m_even_below_tie"] = (_gate_case(Km=km(succ(n_even - 0.5, 0)), **size(n_even)), True,
                                      ax + "m_even_tie_out", g)
        C[ax + "m_odd_tie_in"] = (_gate_case(Km=km(n_odd - 0.5), **size(n_odd)), True, ax + "m_odd_above_tie", g)
        C[ax + "m_odd_above_tie"] = (_gate_case(Km=km(succ(n_odd - 0.5)), **size(n_odd)), False, ax + "m_odd_tie_in", g)
    # a projection that overflows: d = 2^-100 and the model camera moved by -d (1 - 2^-24) leave pm.z =
    # 2^-124; with pm.x = 1000, pm.x / pm.z is inf
    tz = -float(tiny) * (1 - 2.0 ** -24)
    C["proj_finite"] = (_gate_case(d=tiny, model_t=(0, 0, tz)), True, "proj_inf", "fu_raw")
    C["proj_inf"] = (_gate_case(d=tiny, model_t=(1000.0, 0, tz)), False, "proj_finite", "fu_raw")
    # the normal
    C["n_zero"] = (_gate_case(normal=(0, 0, 0)), False, "n_tiny", "n")
    C["n_tiny"] = (_gate_case(normal=(0, 0, tiny)), True, "n_zero", "n")
    C["point_nan"] = (_gate_case(point_nan=True), False, None, "e2")
    # the distance: d = 0.375, e = (0, 0, 0.25) exactly, and e.z one ulp more
    C["dist_eq"] = (_gate_case(d=0.375, offset=(0.0, 0.0, 0.25), encode=False), True, "dist_above", "e2")
    C["dist_above"] = (_gate_case(d=0.375, offset=(0.0, 0.0, float(succ(0.25))), encode=False), False, "dist_eq", "e2")
    C["dist_zero_gate"] = (_gate_case(offset=(0.0, 0.0, 0.0), max_dist=0.0, encode=False), True, "dist_zero_gate_off",
                           "e2")
    C["dist_zero_gate_off"] = (_gate_case(offset=(0.0, 0.0, 2.0 ** -24), max_dist=0.0, encode=False), False,
                               "dist_zero_gate", "e2")
    return C


# ---- the sum tree ----
TREE_NWG = (1, 2, 31, 32, 33, 65, 224, 225, 257, 1025, 1200)
TREE_RAGGED = ((250, 130, 1), (511, 97, 2))
TREE_MAX_DIST = 0.1


def tree_case(W, H, stride=1, seed=0):
    """A W x H depth frame and a model of the same size and camera, both at the identity, K = (256, 256,
    128, H / 2): depths seeded in (0.5, 3.9]; the model point of a pixel is its depth point plus an
    offset of up to 0.05 per axis, the normal a seeded direction times 10^-U(0, 3) (terms of both signs
    over six decades). About 2.5 % each: depth 0, depth NaN, no normal, offset (0.2, 0, 0) (outside the
    0.1 gate)."""
    rng = np.random.default_rng(1000 * W + H + seed)
    K = (256.0, 256.0, 128.0, float(H // 2))
    depth = (3.9 - rng.uniform(0, 3.4, (H, W))).astype(f32)
    F = ref.Camera(K, se3())
    v, u = np.mgrid[0:H, 0:W]
    ray = F.pixel_ray(u.reshape(-1), v.reshape(-1))
    d = depth.reshape(-1)
    pw = np.stack([ray[0] * d, ray[1] * d, d], -1).reshape(H, W, 3)
    point = pw + rng.uniform(-0.05, 0.05, pw.shape).astype(f32)
    nrm = rng.normal(size=pw.shape)
    nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True) * 10.0 ** -rng.uniform(0, 3, (H, W, 1))
    kind = rng.integers(0, 40, (H, W))
    depth[kind == 0] = 0.0
    depth[kind == 1] = np.nan
    nrm[kind == 2] = 0.0
    point[kind == 3] = pw[kind == 3] + np.array([0.2, 0, 0], f32)
    return dict(depth=depth, K=K, pose=se3(), model=dict(point=point.astype(f32), normal=nrm.astype(f32)), model_K=K,
                model_pose=se3(), max_dist=TREE_MAX_DIST, max_depth=ref.MAX_DEPTH, stride=stride)


def tree_scalar(terms, nsamples):
    """The documented tree as a scalar pure-Python walk over terms (nsamples, 29): for
    tests/test_icp_cases_cpu.py, against ref.icp_tree."""
    nwg = (nsamples + 255) // 256
    part = []
    for g in range(nwg):
        waves = []
        for w in range(4):
            a = [[float(terms[s, i]) if s < nsamples else 0.0 for i in range(29)]
                 for s in range(256 * g + 64 * w, 256 * g + 64 * w + 64)]
            for o in (32, 16, 8, 4, 2, 1):
                a = [[a[l][i] + a[l ^ o][i] for i in range(29)] for l in range(64)]
            waves.append(a[0])
        part.append([((waves[0][i] + waves[1][i]) + waves[2][i]) + waves[3][i] for i in range(29)])
    ln = (nwg + 31) // 32
    runs = []
    for c in range(32):
        acc = [0.0] * 29
        for g in range(c * ln, min(nwg, (c + 1) * ln)):
            acc = [acc[i] + part[g][i] for i in range(29)]
        runs.append(acc)
    out = [0.0] * 29
    for c in range(32):
        out = [out[i] + runs[c][i] for i in range(29)]
    return np.array(out)


# ---- the point-map normals ----
NRM_W, NRM_H, NRM_K = 37, 21, (40.0, 40.0, 18.0, 10.0)


def normals_case(tilt=0.45, radius=0.7):
    """(model, K, pose): a 37 x 21 point map of a cylinder (radius 0.7, axis through (0, 0, 2), tilted
    0.45 rad in the image plane; chosen from a scan of 5 radii x 4 tilts for a cosine within 0.01 of 0.3
    on both sides) seen from the origin, so the incidence angle sweeps from 0 to 90 degrees across
    the columns and crosses acos(0.3) at another sub-pixel offset in every row; beyond
    the silhouette a back plane at z = 3.5 (a depth edge). On it: isolated holes and a 3 x 3 hole; a
    5 x 5 patch mirrored in x (its c faces away from the camera: the flip); three pixels whose left
    and right neighbours are one point (nn == 0); four points 1e19 from the origin around one pixel
    (nn overflows at it and at its four diagonal neighbours); a NaN point."""
    K, pose = NRM_K, se3()
    F = ref.Camera(K, pose)
    v, u = np.mgrid[0:NRM_H, 0:NRM_W]
    ray = F.pixel_ray(u.reshape(-1), v.reshape(-1))
    r = np.stack(ray, -1).astype(np.float64)
    ax = np.array([np.sin(tilt), np.cos(tilt), 0.0])
    c0, R = np.array([0.0, 0.0, 2.0]), radius
    # |t r - c0 - ((t r - c0) . ax) ax| = R
    rp, cp = r - (r @ ax)[:, None] * ax, c0 - (c0 @ ax) * ax
    A, B, Cc = (rp * rp).sum(-1), -2 * rp @ cp, cp @ cp - R * R
    disc = B * B - 4 * A * Cc
    t = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), 3.5)
    point = (r * t[:, None]).astype(f32).reshape(NRM_H, NRM_W, 3)
    normal = np.zeros_like(point)
    normal[..., 2] = -1.0  # says only where a surface is
    for (hu, hv) in ((9, 4), (20, 3), (27, 15)):  # isolated holes
        normal[hv, hu] = 0
    normal[14:17, 12:15] = 0  # a 3 x 3 hole
    point[5:10, 21:26] = point[5:10, 21:26][:, ::-1].copy()  # mirrored in x
    for (du, dv) in ((5, 12), (8, 17), (17, 12)):  # duplicate neighbours
        point[dv, du + 1] = point[dv, du - 1]
    gu, gv = 22, 15
    point[gv, gu + 1], point[gv, gu - 1] = (1e19, 0, 2), (-1e19, 0, 2)
    point[gv + 1, gu], point[gv - 1, gu] = (0, 1e19, 2), (0, -1e19, 2)
    point[3, 14] = np.nan
    return dict(point=point, normal=normal), K, pose


def normals_rules(model, K, pose):
    """Which rule of k_surface_normals decides each pixel, restated in float32: dict of (H, W) bool maps
    border, hole (interior, a surface missing among the five), nn_zero, nn_not_finite, angle_drop (nn
    fine, the cosine test fails), kept, flip (kept and turned), plus cos (float64 |c . to| / sqrt(nn
    to . to) where that is finite, NaN elsewhere)."""
    pt = model["point"]
    H, W = pt.shape[:2]
    P = ref.Camera(K, pose)
    has = (model["normal"] != 0).any(axis=-1)
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    ok = np.zeros((H, W), bool)
    ok[1:-1, 1:-1] = has[1:-1, 1:-1] & has[1:-1, 2:] & has[1:-1, :-2] & has[2:, 1:-1] & has[:-2, 1:-1]
    out = {k: np.zeros((H, W), bool) for k in ("nn_zero", "nn_not_finite", "angle_drop", "kept", "flip")}
    cos = np.full((H, W), np.nan)
    if H > 2 and W > 2:
        with np.errstate(all="ignore"):
            dx = tuple(pt[1:-1, 2:, i] - pt[1:-1, :-2, i] for i in range(3))
            dy = tuple(pt[2:, 1:-1, i] - pt[:-2, 1:-1, i] for i in range(3))
            c = ref.cross3(dy, dx)
            to = tuple(pt[1:-1, 1:-1, i] - P.wt[i] for i in range(3))
            dv = ref.dot3(c, to)
            nn = ref.dot3(c, c)
            tt = ref.dot3(to, to)
            inner = ok[1:-1, 1:-1]
            fine = (nn > 0) & (nn < np.inf)
            test = dv * dv >= (f32(0.3) * f32(0.3)) * (nn * tt)
            out["nn_zero"][1:-1, 1:-1] = inner & (nn == 0)
            out["nn_not_finite"][1:-1, 1:-1] = inner & ~(nn == 0) & ~fine
            out["angle_drop"][1:-1, 1:-1] = inner & fine & ~test
            out["kept"][1:-1, 1:-1] = inner & fine & test
            out["flip"][1:-1, 1:-1] = inner & fine & test & (dv > 0)
            cos[1:-1, 1:-1] = np.abs(dv.astype(np.float64)) / np.sqrt(nn.astype(np.float64) * tt.astype(np.float64))
    return dict(border=border, hole=~border & ~ok, cos=cos, **out)
