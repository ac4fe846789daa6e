"""The frontier mask and the connected components restated in numpy (include/disinfect_tsdf.h "Frontiers and
connected components over a box"): mark() by six shifted comparisons, the labelling twice by methods that are
not the GPU's -- a raster-order flood fill and a vectorised minimum over 26 shifted copies -- and the cluster
table from a labelling. Arrays are (nz, ny, nx); a linear index is (z * ny + y) * nx + x."""
import numpy as np

NONE = 0xFFFFFFFF
UNREACHED = 0xFFFFFFFF
COMPONENT_DTYPE = np.dtype([("label", "<u4"), ("size", "<u4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)),
                            ("sum", "<i8", (3,)), ("goal", "<u4"), ("goal_key", "<u4")])
DIRS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


def _shift(a, d, fill):
    """b[z, y, x] = a[z + dz, y + dy, x + dx], `fill` where that lies outside the box."""
    out = np.full_like(a, fill)
    src, dst = [], []
    for n, k in zip(a.shape, d):
        src.append(slice(max(k, 0), n + min(k, 0)))
        dst.append(slice(max(-k, 0), n + min(-k, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def mark(state, cost=None):
    """mask uint8: state 1, reached when a cost is given, and a face neighbour inside the box of state 0."""
    state = np.asarray(state)
    unknown = state == 0
    touch = np.zeros(state.shape, bool)
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        touch |= _shift(unknown, d, False)
    m = (state == 1) & touch
    if cost is not None:
        m &= np.asarray(cost) != UNREACHED
    return m.astype(np.uint8)


def label_flood(mask):
    """Raster-order flood fill: the first unseen member met is its component's least index."""
    member = np.asarray(mask) != 0
    nz, ny, nx = member.shape
    lab = np.full(member.shape, NONE, np.uint32)
    flat_m, flat_l = member.reshape(-1), lab.reshape(-1)
    for i in np.flatnonzero(flat_m):
        if flat_l[i] != NONE:
            continue
        flat_l[i] = i
        stack = [int(i)]
        while stack:
            v = stack.pop()
            z, r = divmod(v, ny * nx)
            y, x = divmod(r, nx)
            for dz, dy, dx in DIRS:
                a, b, c = z + dz, y + dy, x + dx
                if 0 <= a < nz and 0 <= b < ny and 0 <= c < nx:
                    n = (a * ny + b) * nx + c
                    if flat_m[n] and flat_l[n] == NONE:
                        flat_l[n] = i
                        stack.append(n)
    return lab


def label_sweep(mask):
    """Every member takes the least label among itself and its 26 neighbours until nothing changes."""
    member = np.asarray(mask) != 0
    big = np.int64(1) << 40
    lab = np.where(member, np.arange(member.size, dtype=np.int64).reshape(member.shape), big)
    while True:
        new = lab.copy()
        for d in DIRS:
            np.minimum(new, _shift(lab, d, big), out=new)
        new = np.where(member, new, big)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(member, lab, NONE).astype(np.uint32)


def table(label, key=None, min_size=1):
    """(clusters with size >= min_size in ascending label, total) from a labelling."""
    label = np.asarray(label)
    nz, ny, nx = label.shape
    flat = label.reshape(-1)
    idx = np.flatnonzero(flat != NONE)
    roots, inv, sizes = np.unique(flat[idx], return_inverse=True, return_counts=True)
    out = np.zeros(roots.size, COMPONENT_DTYPE)
    out["label"], out["size"] = roots, sizes
    coords = np.stack([idx % nx, idx // nx % ny, idx // (nx * ny)], -1).astype(np.int64)
    k = np.zeros(idx.size, np.uint64) if key is None else np.asarray(key).reshape(-1)[idx].astype(np.uint64)
    packed = (k << np.uint64(32)) | idx.astype(np.uint64)
    order = np.argsort(inv, kind="stable")
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    if roots.size:
        c = coords[order]
        out["lo"] = np.minimum.reduceat(c, starts, axis=0)
        out["hi"] = np.maximum.reduceat(c, starts, axis=0)
        out["sum"] = np.add.reduceat(c, starts, axis=0)
        best = np.minimum.reduceat(packed[order], starts)
        out["goal"] = (best & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        out["goal_key"] = (best >> np.uint64(32)).astype(np.uint32)
    return out[out["size"] >= min_size], int(roots.size)


def tiles_spanned(label, root):
    """The number of 8^3 tiles (from the box's first voxel) that hold members of component `root`."""
    z, y, x = np.nonzero(np.asarray(label) == np.uint32(root))
    return len(set(zip(z // 8, y // 8, x // 8)))


def masks(shapes, density):
    """The shapes test's masks: one generator per density, the shapes drawn from it in order."""
    rng = np.random.default_rng(int(density * 100))
    return [rng.random(shape) < density for shape in shapes]
