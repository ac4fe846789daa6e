"""numpy restatement of the UV dose contract (include/disinfect_tsdf.h, DESIGN.md "UV dose") on an engine
dump, for tests/test_gpu_uv_dose.py. float32 one operation at a time, as the kernels' (no contraction, IEEE
division and square root); the voxel lookups, round_s16 and dot3 are _track_ref's."""
import numpy as np

from _track_ref import Blocks, dot3, round_s16

f32 = np.float32
DEFAULTS = dict(min_range=0.05, max_range=5.0, sample_offset=0.0, min_weight=1)


def _cols(a):
    a = np.ascontiguousarray(a, f32).reshape(-1, 3)
    return tuple(a[:, i].copy() for i in range(3))


def normals(dump, points, voxel, sample_offset=0.0):
    """tsdf_surface_normals: (n, 3) f32."""
    B = Blocks(dump)
    voxel, off = f32(voxel), f32(sample_offset)
    v = tuple(round_s16(c / voxel - off) for c in _cols(points))
    e = np.eye(3, dtype=np.int64)
    nr = tuple(B.sample(tuple(v[j] + e[i, j] for j in range(3))) - B.sample(tuple(v[j] - e[i, j] for j in range(3)))
               for i in range(3))
    nn = dot3(nr, nr)
    assert nn.dtype == f32
    with np.errstate(all="ignore"):
        good = (nn > 0) & (nn < np.inf)
        ln = np.sqrt(nn)
        return np.stack([np.where(good, nr[i] / ln, f32(0)) for i in range(3)], -1).astype(f32)


def dose(dump, points, nrm, emitters, voxel, dose0=None, bias=None, step=None, min_range=0.05, max_range=5.0,
         sample_offset=0.0, min_weight=1):
    """tsdf_uv_dose: (dose (n,) f32, counted (n, m) bool: in range and on the normal's side, visible (n, m)
    bool: counted and no sample occludes). bias / step None: the defaults, 2 voxels and 1 voxel."""
    B = Blocks(dump)
    voxel = f32(voxel)
    bias = f32(2) * voxel if bias is None else f32(bias)
    step = voxel if step is None else f32(step)
    off, rmin, rmax = f32(sample_offset), f32(min_range), f32(max_range)
    p, n = _cols(points), _cols(nrm)
    em = np.ascontiguousarray(emitters, f32).reshape(-1, 4)
    N, M = p[0].size, em.shape[0]
    out = np.zeros(N, f32) if dose0 is None else np.array(dose0, f32).reshape(N).copy()
    recv = (n[0] != 0) | (n[1] != 0) | (n[2] != 0)
    o = tuple(p[i] + bias * n[i] for i in range(3))
    ov = tuple(o[i] / voxel - off for i in range(3))
    sv = step / voxel
    acc = np.zeros(N, f32)
    counted, visible = np.zeros((N, M), bool), np.zeros((N, M), bool)
    with np.errstate(all="ignore"):
        for k in range(M):
            e, energy = em[k, :3], em[k, 3]
            d = tuple(e[i] - p[i] for i in range(3))
            r2 = dot3(d, d)
            r = np.sqrt(r2)
            c = dot3(n, d) / r
            cnt = recv & (r >= rmin) & (r <= rmax) & (c > 0)
            ev = tuple(e[i] / voxel - off for i in range(3))
            dv = tuple(ev[i] - ov[i] for i in range(3))
            L = np.sqrt(dot3(dv, dv))
            pos = L > 0
            sg = tuple(np.where(pos, dv[i] / L * sv, f32(0)).astype(f32) for i in range(3))
            J = np.where(pos & cnt, np.trunc(np.where(cnt, L / sv, 0)), 0).astype(np.int64)
            occ = np.zeros(N, bool)
            live = cnt.copy()
            j = 0
            while live.any():
                idx = np.flatnonzero(live)
                s = tuple(ov[i][idx] + f32(j) * sg[i][idx] for i in range(3))
                assert s[0].dtype == f32
                ok, vi = B.voxel(tuple(round_s16(a) for a in s))
                vi = np.where(ok, vi, 0)
                hit = ok & (B.rgbw[vi][:, 3].astype(np.int64) >= min_weight) & (B.tsdf[vi] <= 0)
                occ[idx[hit]] = True
                live[idx[hit]] = False
                live &= j < J
                j += 1
            vis = cnt & ~occ
            term = (energy * f32(0.07957747)) * (c / r2)
            assert term.dtype == f32
            acc = np.where(vis, acc + term, acc).astype(f32)
            counted[:, k], visible[:, k] = cnt, vis
    return np.where(recv, out + acc, out).astype(f32), counted, visible
