"""numpy restatement of the travel-field contract (include/disinfect_tsdf.h, DESIGN.md "Travel field") for
tests/test_travel_cpu.py and tests/test_gpu_travel.py: passable(), the cost field twice -- field() by heap
Dijkstra, sweep() by a vectorised relaxation over 26 shifted copies until nothing changes -- and paths() by
the walk-back rule. Neither is the GPU's algorithm (tile-wise label correcting). All integers. Arrays are
(nz, ny, nx); seeds and targets are box-local (x, y, z)."""
import heapq

import numpy as np

UNREACHED = 0xFFFFFFFF
# the contract's direction order: dz slowest, then dy, then dx, each -1, 0, 1, (0, 0, 0) skipped
DIRS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
W = [2 + abs(dx) + abs(dy) + abs(dz) for dx, dy, dz in DIRS]


def passable(d2, state, clearance2=0, unknown_free=False):
    d2, state = np.asarray(d2), np.asarray(state)
    ok = state == 1
    if unknown_free:
        ok = ok | (state == 0)
    return ok & (d2.astype(np.int64) >= clearance2)


def usable_seeds(ok, seeds):
    """The seeds inside the box and passable, as (x, y, z) rows, duplicates kept."""
    s = np.asarray(seeds, np.int64).reshape(-1, 3)
    nz, ny, nx = ok.shape
    inb = ((s >= 0) & (s < np.array([nx, ny, nz]))).all(axis=1)
    s = s[inb]
    return s[ok[s[:, 2], s[:, 1], s[:, 0]]]


def field(ok, seeds):
    """cost (nz, ny, nx) uint32 and the number of seeds used, by Dijkstra with a heap."""
    nz, ny, nx = ok.shape
    s = usable_seeds(ok, seeds)
    INF = 1 << 62
    okl = ok.ravel().tolist()
    dist = [INF] * (nx * ny * nz)
    heap = []
    for x, y, z in s.tolist():
        i = (z * ny + y) * nx + x
        if dist[i]:
            dist[i] = 0
            heap.append((0, i))
    heapq.heapify(heap)
    while heap:
        c, i = heapq.heappop(heap)
        if c > dist[i]:
            continue
        x, y, z = i % nx, i // nx % ny, i // (nx * ny)
        for (dx, dy, dz), w in zip(DIRS, W):
            a, b, d = x + dx, y + dy, z + dz
            if 0 <= a < nx and 0 <= b < ny and 0 <= d < nz:
                j = (d * ny + b) * nx + a
                if okl[j] and c + w < dist[j]:
                    dist[j] = c + w
                    heapq.heappush(heap, (c + w, j))
    out = np.array(dist, np.int64)
    out[out == INF] = UNREACHED
    return out.astype(np.uint32).reshape(ok.shape), int(s.shape[0])


def sweep(ok, seeds):
    """cost, seeds used and the number of passes: every voxel takes the least of itself and its 26 shifted
    neighbours plus the step, all at once, until a pass changes nothing."""
    nz, ny, nx = ok.shape
    s = usable_seeds(ok, seeds)
    INF = np.int64(1) << 40
    c = np.full((nz + 2, ny + 2, nx + 2), INF, np.int64)
    c[s[:, 2] + 1, s[:, 1] + 1, s[:, 0] + 1] = 0
    inner = (slice(1, -1),) * 3
    passes = 0
    while True:
        passes += 1
        best = c[inner].copy()
        for (dx, dy, dz), w in zip(DIRS, W):
            nb = c[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
            np.minimum(best, nb + w, out=best)
        best = np.where(ok, best, INF)
        if np.array_equal(best, c[inner]):
            break
        c[inner] = best
    out = c[inner].copy()
    out[out >= INF] = UNREACHED
    return out.astype(np.uint32), int(s.shape[0]), passes


def paths(cost, targets, max_len=None):
    """(list of int32 arrays of linear indices, target first; list of len) by the walk-back rule. With max_len
    only the first max_len voxels of a walk are kept; len is the full count, negated where the walk stopped
    without reaching cost 0."""
    cost = np.asarray(cost)
    nz, ny, nx = cost.shape
    cl = cost.ravel().astype(np.int64).tolist()
    out, lens = [], []
    for x, y, z in np.asarray(targets, np.int64).reshape(-1, 3).tolist():
        p = []
        n = 0
        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and cl[(z * ny + y) * nx + x] != UNREACHED:
            while True:
                i = (z * ny + y) * nx + x
                p.append(i)
                if cl[i] == 0:
                    n = len(p)
                    break
                for (dx, dy, dz), w in zip(DIRS, W):
                    a, b, d = x + dx, y + dy, z + dz
                    if 0 <= a < nx and 0 <= b < ny and 0 <= d < nz:
                        j = (d * ny + b) * nx + a
                        if cl[j] != UNREACHED and cl[j] + w == cl[i]:
                            x, y, z = a, b, d
                            break
                else:
                    n = -len(p)
                    break
        lens.append(n)
        out.append(np.array(p if max_len is None else p[:max_len], np.int32))
    return out, lens


def serpentine(nx, ny, nz, pitch=4, gap=4):
    """passable (nz, ny, nx) of a serpentine maze: a wall across every x = pitch - 1 (mod pitch) plane, with a
    gap of `gap` voxels in y alternating between the high-y and the low-y end, so a path from x = 0 to
    x = nx - 1 runs the length of y once per wall."""
    ok = np.ones((nz, ny, nx), bool)
    for k, x in enumerate(range(pitch - 1, nx, pitch)):
        ok[:, :, x] = False
        if k % 2 == 0:
            ok[:, ny - gap:, x] = True
        else:
            ok[:, :gap, x] = True
    return ok


def arrays(ok):
    """d2 and state arrays whose passable(d2, state) is ok: impassable voxels are inside (state 2)."""
    return np.where(ok, 100, 0).astype(np.uint16), np.where(ok, 1, 2).astype(np.uint8)
