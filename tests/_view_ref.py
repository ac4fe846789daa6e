"""numpy restatement of the view-gain contract (include/disinfect_tsdf.h, DESIGN.md "View gain") for
tests/test_view_cpu.py and tests/test_gpu_view.py: the predicted depth image by the plain march and the gain by
the free layer's own gather (_free_ref.terms) with valid reduced to d != 0 and the truncation replaced by the
margin. float32, one IEEE operation at a time: rays by _free_ref.ray_lengths' expression, the transform in
Eigen's order (_track_ref.se3_apply) with world_T_cam from tsdf_amd.SE3.Inverse, voxels by _geo_edges._round_away
(half away from zero, NaN -> 0). Not the GPU's algorithm: no culls, no skipping, every sample of every ray and
every voxel of the box. A view is (q xyzw, t); state is uint8 (nz, ny, nx); seen is a bool mask (nz, ny, nx)."""
import numpy as np

import _free_ref
from _geo_edges import _round_away
from _track_ref import se3_apply

f32 = np.float32


def samples(far, step):
    """J = f2i(far / step) in float32."""
    return int(f32(far) / f32(step))


def predict(state, origin, voxel, K, W, H, q, t, far, step, miss_depth):
    """pred (H, W) float32 of the view cam_T_world = (q, t)."""
    import tsdf_amd
    state = np.asarray(state, np.uint8)
    nz, ny, nx = state.shape
    o = [int(v) for v in origin]
    K = np.asarray(K, f32)
    ifx, ify = f32(1) / K[0], f32(1) / K[1]
    icx, icy = -K[2] * ifx, -K[3] * ify
    dx = np.broadcast_to(ifx * np.arange(W, dtype=f32)[None, :] + icx * f32(1), (H, W))
    dy = np.broadcast_to(ify * np.arange(H, dtype=f32)[:, None] + icy * f32(1), (H, W))
    inv = tsdf_amd.SE3(np.asarray(q, f32), np.asarray(t, f32)).Inverse()
    wq, wt = [f32(c) for c in inv.q], [f32(c) for c in inv.t]
    pred = np.full((H, W), f32(miss_depth), f32)
    done = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        for j in range(1, samples(far, step) + 1):
            z = f32(j) * f32(step)
            pw = se3_apply(wq, wt, (dx * z, dy * z, np.full((H, W), z, f32)))
            g = [_round_away(np.asarray(pw[a], f32) / f32(voxel)) - o[a] for a in range(3)]
            inside = (g[0] >= 0) & (g[0] < nx) & (g[1] >= 0) & (g[1] < ny) & (g[2] >= 0) & (g[2] < nz)
            s = state[np.where(inside, g[2], 0), np.where(inside, g[1], 0), np.where(inside, g[0], 0)]
            hit = inside & (s == 2) & ~done
            pred[hit] = z
            done |= hit
            if done.all():
                break
    return pred


def visible(origin, dims, voxel, K, q, t, pred, margin):
    """vis(., view) over the box: bool (nz, ny, nx)."""
    fr = _free_ref.frame(pred, K, q, t, np.inf)
    tm = _free_ref.terms(_free_ref.box_points(origin, dims), fr, voxel, margin)
    with np.errstate(all="ignore"):
        return tm["inb"] & (tm["d"] != 0) & (tm["sdf"] >= f32(margin)) & (tm["hz"] > 0)


def view_gain(state, origin, voxel, K, W, H, views, far, step, margin, miss_depth, seen=None):
    """(gain (V,) int64, pred (V, H, W) float32, vis (V, nz, ny, nx) bool)."""
    state = np.asarray(state, np.uint8)
    nz, ny, nx = state.shape
    cand = state == 0
    if seen is not None:
        cand = cand & ~np.asarray(seen, bool)
    gain, preds, viss = [], [], []
    for q, t in views:
        p = predict(state, origin, voxel, K, W, H, q, t, far, step, miss_depth)
        m = visible(origin, (nx, ny, nz), voxel, K, q, t, p, margin)
        preds.append(p)
        viss.append(m)
        gain.append(int((cand & m).sum()))
    return (np.asarray(gain, np.int64), np.asarray(preds, f32).reshape(len(views), H, W),
            np.asarray(viss, bool).reshape(len(views), nz, ny, nx))


def next_views(state, origin, voxel, trunc, K, W, H, views, k, far, step, miss_depth):
    """The greedy loop of esdf.next_views: (chosen, gains, seen mask). The margin is the truncation, and a
    commit is _free_ref's observe of the predicted image with max_depth 2 far."""
    state = np.asarray(state, np.uint8)
    nz, ny, nx = state.shape
    seen = np.zeros(state.shape, bool)
    _, preds, viss = view_gain(state, origin, voxel, K, W, H, views, far, step, trunc, miss_depth)
    chosen, gains = [], []
    for _ in range(k):
        if not len(views):
            break
        g = np.array([int(((state == 0) & ~seen & m).sum()) for m in viss], np.int64)
        i = int(np.argmax(g))
        if g[i] <= 0:
            break
        q, t = views[i]
        seen |= _free_ref.frame_mask(origin, (nx, ny, nz), _free_ref.frame(preds[i], K, q, t, f32(2) * f32(far)), voxel, trunc)
        chosen.append(i)
        gains.append(int(g[i]))
    return chosen, gains, seen
