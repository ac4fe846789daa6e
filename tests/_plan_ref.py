"""numpy restatement of the tsdf_uv_plan contract (include/disinfect_tsdf.h, DESIGN.md "Lamp-stop planning")
and direct computations of the planner's helpers, for tests/test_plan_cpu.py and tests/test_gpu_plan.py.
The terms are float32 one operation at a time, as the kernel's; a gain is math.fsum of the exact terms --
the correctly rounded sum, the yardstick the library's fixed addition tree is measured against. The
irradiance needs no restatement of its own: row c is _uv_ref.dose over emitters[first[c]:first[c + 1]]."""
import math

import numpy as np

f32 = np.float32


def terms(E, need, weight):
    """g(c, i): (C, n) f32. Both tests: a NaN in E or need contributes nothing."""
    E = np.asarray(E, f32)
    need = np.asarray(need, f32)
    w = np.ones(need.shape, f32) if weight is None else np.asarray(weight, f32)
    with np.errstate(invalid="ignore"):
        ok = (E > 0) & (need > 0)[None, :]
        g = (w[None, :] * np.fmin(E, need[None, :])).astype(f32)
    assert g.dtype == f32
    return np.where(ok, g, f32(0))


def gain_bound(g):
    """n * 2^-53 * sum |term| per candidate (the ICP sums' bound): what any order of n double additions of
    exactly represented terms stays within of the exact sum."""
    return g.shape[1] * 2.0 ** -53 * np.array([math.fsum(np.abs(row).astype(np.float64).tolist()) for row in g])


def plan(E, need, weight=None, max_stops=16, min_gain=0.0):
    """dict(stops, gains (fsum), need, rounds): rounds holds per round the fsum gains of every candidate and
    their bound, the round that stopped the plan included."""
    E = np.ascontiguousarray(E, f32)
    need = np.array(need, f32).copy()
    stops, gains, rounds = [], [], []
    for _ in range(max_stops):
        g = terms(E, need, weight)
        G = np.array([math.fsum(row.astype(np.float64).tolist()) for row in g])
        rounds.append((G, gain_bound(g)))
        b = int(np.argmax(G))  # (the first of equal maxima: the lowest index)
        if not (G[b] > 0) or not (G[b] >= f32(min_gain)):
            break
        stops.append(b)
        gains.append(G[b])
        row = E[b]
        with np.errstate(invalid="ignore"):
            hit = row > 0
            need = np.where(hit, np.fmax((need - row).astype(f32), f32(0)), need).astype(f32)
    return dict(stops=np.array(stops, np.int32), gains=np.array(gains, np.float64), need=need, rounds=rounds)


def synthetic(C, n, seed):
    """The seeded matrices of the plan tests: (E, need, weight)."""
    rng = np.random.default_rng(seed)
    E = rng.random((C, n)) ** 4 * rng.random((C, 1)) * 20
    E[rng.random((C, n)) < 0.5] = 0
    need = rng.random(n) * 30
    need[::7] = 0
    weight = rng.random(n)
    weight[::11] = 0
    if n == 1:
        need[:] = 12.5  # (a single receiver: a plan with something to do)
        weight[:] = 0.75
        E[E == 0] = 3.0
    return E.astype(f32), need.astype(f32), weight.astype(f32)


# ---- the helpers, computed directly ----
def tube_candidates(centres, axis, length, power_w, dwell_s, segments):
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    a = np.asarray(axis, np.float64)
    h = a / math.sqrt(float(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])) * (length / 2)
    em = np.zeros((centres.shape[0] * segments, 4), f32)
    for c, p in enumerate(centres):
        for s in range(segments):
            t = (s + 0.5) / segments
            em[c * segments + s, :3] = (p - h) + t * ((p + h) - (p - h))
            em[c * segments + s, 3] = power_w * dwell_s / segments
    return em, np.arange(centres.shape[0] + 1, dtype=np.int32) * np.int32(segments)


def plan_need(dose, prob, target, prob_min=0.5):
    out = np.zeros(len(dose), f32)
    for i, (d, p) in enumerate(zip(dose, prob)):
        if f32(p) >= f32(prob_min):
            out[i] = max(f32(target) - f32(d), f32(0))
    return out


def vertex_area(positions, indices):
    p = np.asarray(positions, np.float64)
    out = np.zeros(p.shape[0], np.float64)
    for k in range(3):
        for t in np.asarray(indices):
            a = p[t[1]] - p[t[0]]
            b = p[t[2]] - p[t[0]]
            cr = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
            out[t[k]] += math.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]) / 6.0
    return out.astype(f32)


def standoff_candidates(field, voxel, lo, hi, stride):
    nx, ny, nz = field["dims"]
    out = []
    for z in range(0, nz, stride):
        for y in range(0, ny, stride):
            for x in range(0, nx, stride):
                d = f32(np.sqrt(f32(field["d2"][z, y, x]))) * f32(voxel)
                if field["state"][z, y, x] == 1 and f32(lo) <= d <= f32(hi):
                    out.append([f32(field["origin"][a] + v) * f32(voxel) for a, v in enumerate((x, y, z))])
    return np.array(out, f32).reshape(-1, 3)
