"""Indexed semantic mesh (tsdf_extract_mesh_indexed) against a numpy restatement of its contract.

The scene is that of test_gpu_parity.test_marching_cubes_matches_oracle (96x72, 1 cm voxels, 4 cm
truncation, 4 frames, 2^13 blocks); a hand-built volume of seven blocks around the origin covers
vertices shared across block faces, edges and the corner, edges owned through their upper endpoint,
coincident vertices and NaN probabilities. Everything is compared bit for bit: the reference below
works in numpy float32 op by op, as the kernels do (no contraction, IEEE division).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "mesh_main")
VOXEL, TRUNC, NB_BITS, MISSING = 0.01, 0.04, 13, 0.99
ARRAYS = ("positions", "rgba", "prob", "keys", "indices")
CASES = [(0, False, 0), (1, False, 0), (1, True, 0), (0, False, 7)]
f32 = np.float32


# ---------------------------------------------------------------------------------------------
# numpy restatement
# ---------------------------------------------------------------------------------------------
class Volume:
    """The selected blocks of an engine dump in entry order, with the sampling rule applied."""

    def __init__(self, dump, voxel, missing, min_weight, bounds=None):
        live = np.flatnonzero(dump["entry_idx"] >= 0)
        blocks = dump["entry_pos"][live, :3].astype(np.int64)
        if bounds is not None:  # the Query block selection (k_query_count)
            scale = f32(1.0 / float(f32(voxel)))
            b = (np.asarray(bounds, f32) * scale).astype(np.int64)  # truncation toward zero, in range here
            lo, hi = b[[0, 2, 4]], b[[1, 3, 5]]
            keep = np.all(blocks * 8 >= lo, axis=1) & np.all(blocks * 8 + 7 <= hi, axis=1)
            live, blocks = live[keep], blocks[keep]
        pool = dump["entry_idx"][live].astype(np.int64)
        self.voxel, self.missing, self.blocks = f32(voxel), f32(missing), blocks
        self.n = n = blocks.shape[0]
        vox = (pool[:, None] * 512 + np.arange(512)[None, :])
        tsdf = dump["tsdf"][vox]
        self.rgbw = np.concatenate([dump["rgbw"][vox], np.zeros((1, 512, 4), np.uint8)])
        self.prob = np.concatenate([dump["prob"][vox], np.zeros((1, 512), f32)])
        ok = np.ones((n, 512), bool) if min_weight <= 0 else self.rgbw[:n, :, 3].astype(np.int64) >= min_weight
        # row n: every unselected block (all samples missing)
        self.ok = np.concatenate([ok, np.zeros((1, 512), bool)])
        self.val = np.concatenate([np.where(ok, tsdf, self.missing), np.full((1, 512), missing, f32)]).astype(f32)
        self._code = self._encode(blocks)
        self._order = np.argsort(self._code, kind="stable")
        self._sorted = self._code[self._order]
        assert np.unique(self._code).size == n

    @staticmethod
    def _encode(b):
        b = np.asarray(b, np.int64) + (1 << 19)
        return (b[..., 0] << 40) | (b[..., 1] << 20) | b[..., 2]

    def rank(self, blocks):
        """Selection rank of block coordinates (n = not selected)."""
        if self.n == 0:
            return np.full(np.shape(blocks)[:-1], 0, np.int64)
        code = self._encode(blocks)
        i = np.minimum(np.searchsorted(self._sorted, code), self.n - 1)
        return np.where(self._sorted[i] == code, self._order[i], self.n)

    def sample(self, g):
        """(value, valid, rank, voxel index) of global voxel coordinates g (..., 3)."""
        g = np.asarray(g, np.int64)
        r = self.rank(g >> 3)
        l = g & 7
        vi = l[..., 0] + 8 * l[..., 1] + 64 * l[..., 2]
        return self.val[r, vi], self.ok[r, vi], r, vi

    def lattice(self, g):
        return np.asarray(g).astype(f32) * self.voxel + f32(0.5) * self.voxel

    def crossed_edges(self):
        """Every grid edge with at least one endpoint in a selected block whose samples differ in sign:
        keys (gx, gy, gz, axis) of the lower endpoint, in no particular order."""
        loc = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
        out = []
        for axis in range(3):
            e = np.zeros(3, np.int64)
            e[axis] = 1
            # lower endpoint in a selected block
            a = (self.blocks[:, None, :] * 8 + loc[None, :, :]).reshape(-1, 3)
            va, vb = self.sample(a)[0], self.sample(a + e)[0]
            low_owned = a[(va < 0) != (vb < 0)]
            # upper endpoint on the low face of a selected block whose neighbour below is not selected
            face = loc[loc[:, axis] == 0]
            b = (self.blocks[:, None, :] * 8 + face[None, :, :]).reshape(-1, 3)
            b = b[self.rank((b - e) >> 3) == self.n]
            va, vb = self.sample(b - e)[0], self.sample(b)[0]
            up_owned = (b - e)[(va < 0) != (vb < 0)]
            a = np.concatenate([low_owned, up_owned])
            out.append(np.c_[a, np.full(a.shape[0], axis)])
        return np.concatenate(out).astype(np.int32)

    def vertex(self, keys):
        """positions, rgba, prob of the vertices with these keys, by the contract's rules."""
        keys = np.asarray(keys, np.int64)
        a, axis = keys[:, :3], keys[:, 3]
        b = a + np.eye(3, dtype=np.int64)[axis]
        va, oka, ra, ia = self.sample(a)
        vb, okb, rb, ib = self.sample(b)
        rows = np.arange(keys.shape[0])
        pos = self.lattice(a)
        pa, pb = pos[rows, axis], self.lattice(b)[rows, axis]
        with np.errstate(all="ignore"):
            tt = va / (va - vb)
            pos[rows, axis] = pa + tt * (pb - pa)
            qa, qb = self.prob[ra, ia], self.prob[rb, ib]
            both = oka & okb
            prob = np.where(both, qa + tt * (qb - qa), np.where(oka, qa, qb)).astype(f32)
            fa, fb = self.rgbw[ra, ia].astype(f32), self.rgbw[rb, ib].astype(f32)
            mix = (fa + tt[:, None] * (fb - fa) + f32(0.5)).astype(np.int32).astype(np.uint8)
        rgba = np.where(both[:, None], mix, np.where(oka[:, None], self.rgbw[ra, ia], self.rgbw[rb, ib]))
        assert pos.dtype == f32 and tt.dtype == f32
        return pos, rgba.astype(np.uint8), prob, both, oka | okb

    def order_key(self, keys):
        """(owner rank, local z, y, x, axis) of each vertex key."""
        keys = np.asarray(keys, np.int64)
        a, axis = keys[:, :3], keys[:, 3]
        b = a + np.eye(3, dtype=np.int64)[axis]
        ra, rb = self.rank(a >> 3), self.rank(b >> 3)
        lower = ra < self.n
        owner = np.where(lower, ra, rb)
        assert (owner < self.n).all(), "an edge without an endpoint in a selected block"
        l = a - 8 * np.where(lower[:, None], a >> 3, b >> 3)
        return owner, l[:, 2], l[:, 1], l[:, 0], axis


def same_floats(a, b):
    """Bit-identical float32 arrays where NaN (any payload) equals NaN."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb) and
                                       np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def key_codes(keys):
    """One int64 per (gx, gy, gz, axis) row (cheaper to sort and compare than rows)."""
    k = np.asarray(keys, np.int64)
    return ((k[:, 0] + (1 << 19)) << 42) | ((k[:, 1] + (1 << 19)) << 22) | ((k[:, 2] + (1 << 19)) << 2) | k[:, 3]


def same_mesh(a, b):
    return all(same_floats(a[k], b[k]) if a[k].dtype == f32 else np.array_equal(a[k], b[k]) for k in ARRAYS)


def check_mesh(vol, mesh, soup, unambiguous_share=None):
    """Checks 1-5 of one extraction against the reference volume `vol` and the engine's soup.
    Returns (corners, ambiguous corners, both-valid vertices, one-valid vertices)."""
    pos, rgba, prob, keys, idx = (mesh[k] for k in ARRAYS)
    n, m = pos.shape[0], idx.shape[0]
    assert pos.shape == (n, 3) and rgba.shape == (n, 4) and prob.shape == (n,) and keys.shape == (n, 4)
    assert idx.shape == (m, 3) and soup.shape == (m, 3, 3) and m > 0
    assert pos.dtype == f32 and rgba.dtype == np.uint8 and prob.dtype == f32
    assert keys.dtype == np.int32 and idx.dtype == np.int32
    # 1. de-indexing gives the soup; indices in range, every vertex referenced, keys unique
    assert idx.min() >= 0 and idx.max() < n
    assert np.array_equal(pos[idx].view(np.uint32), soup.view(np.uint32))
    assert np.unique(idx).size == n
    assert ((keys[:, 3] >= 0) & (keys[:, 3] <= 2)).all()
    codes = np.unique(key_codes(keys))
    assert codes.size == n
    # 2. the vertex count from first principles, and the vertices are exactly the crossed edges
    edges = vol.crossed_edges()
    print(f"vertices {n}, crossed edges {edges.shape[0]}, triangles {m}")
    assert n == edges.shape[0]
    assert np.array_equal(codes, np.unique(key_codes(edges)))
    # 3. every vertex re-derived from its key
    rpos, rrgba, rprob, both, any_ok = vol.vertex(keys)
    assert any_ok.all()
    assert np.array_equal(pos.view(np.uint32), rpos.view(np.uint32))
    assert same_floats(prob, rprob)
    assert np.array_equal(rgba, rrgba)
    # 4. the edge of a triangle corner with exactly two lattice coordinates, from its position alone
    c = soup.reshape(-1, 3)
    g = np.floor((c.astype(np.float64) - 0.5 * float(vol.voxel)) / float(vol.voxel)).astype(np.int64)
    low = np.full_like(g, np.iinfo(np.int64).min)  # largest g with lattice(g) < c, and is c on the lattice
    on = np.zeros(c.shape, bool)
    for d in (-1, 0, 1, 2):
        lat = vol.lattice(g + d)
        on |= lat == c
        low = np.where(lat < c, np.maximum(low, g + d), low)
    non = on.sum(axis=1)
    assert (non >= 2).all()
    clear = non == 2
    ambiguous = int((~clear).sum())
    print(f"corners {c.shape[0]}, ambiguous {ambiguous}")
    if unambiguous_share is not None:
        assert ambiguous <= unambiguous_share * c.shape[0]
    axis = np.argmin(on[clear], axis=1)
    lat_g = np.rint((c[clear].astype(np.float64) - 0.5 * float(vol.voxel)) / float(vol.voxel)).astype(np.int64)
    assert np.array_equal(vol.lattice(lat_g)[on[clear]], c[clear][on[clear]])
    want = np.where(on[clear], lat_g, low[clear])
    want = np.c_[want, axis]
    assert np.array_equal(keys[idx.reshape(-1)][clear], want)
    # 5. vertex order: by (owner block's rank in entry order, local z, y, x, axis)
    o = vol.order_key(keys)
    perm = np.lexsort(o[::-1])
    assert np.array_equal(perm, np.arange(n))
    return c.shape[0], ambiguous, int(both.sum()), int((~both).sum())


# ---------------------------------------------------------------------------------------------
# the scene (built once)
# ---------------------------------------------------------------------------------------------
def integrate_scene(eng, ora=None):
    import tsdf_amd
    from tsdf_amd import synth
    cam = synth.camera(96, 72, synth.TUM_FR1)
    for f in range(4):
        fr = synth.render(cam, f, touch="complement")
        eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, tsdf_amd.SE3(fr["q"], fr["t"]), 4.0)
        if ora is not None:
            ora.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], 4.0, cam.K, fr["q"], fr["t"])
    assert eng.stats()["status"] == 0


class Scene:
    def __init__(self):
        import tsdf_amd
        from _oracle import OracleGrid
        self.eng = tsdf_amd.Engine(VOXEL, TRUNC, max_width=96, max_height=72, num_block_bits=NB_BITS)
        self.ora = OracleGrid(VOXEL, TRUNC, NB_BITS)
        integrate_scene(self.eng, self.ora)
        self.dump = self.eng.dump()
        d = self.dump
        pos = d["entry_pos"][d["entry_idx"] >= 0, :3].astype(f32) * 8 * 0.01
        lo, hi = np.percentile(pos, 5, axis=0), np.percentile(pos, 95, axis=0) + 0.08
        self.bounds = np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], f32)
        self._ref = {}

    def reference(self, min_weight, bounded):
        """(numpy volume, oracle soup, default-grid indexed mesh), computed once per case."""
        k = (min_weight, bounded)
        if k not in self._ref:
            b = self.bounds if bounded else None
            self._ref[k] = (Volume(self.dump, VOXEL, MISSING, min_weight, b),
                            self.ora.extract_mesh(b, MISSING, min_weight),
                            self.eng.extract_mesh_indexed(b, MISSING, min_weight))
        return self._ref[k]

    def close(self):
        self.eng.close()
        self.ora.close()


@pytest.fixture(scope="module")
def _scene_holder():
    holder = []
    yield holder
    for s in holder:
        s.close()


@pytest.fixture
def scene(_scene_holder):
    """The scene, built by the first test that asks for it (function scope: after conftest's
    autouse fixture has initialised torch's HIP runtime, which must come before the first engine)."""
    if not _scene_holder:
        _scene_holder.append(Scene())
    return _scene_holder[0]


@pytest.mark.parametrize("min_weight,bounded,grid", CASES)
def test_indexed_mesh_matches_contract(scene, min_weight, bounded, grid, monkeypatch):
    """Checks 1-5 on the scene: de-indexing gives the soup (and the oracle's), the vertex count from
    first principles, every vertex re-derived from its key, keys of triangle corners, vertex order;
    TSDF_MESH_GRID=7 (grid-stride walk) and a second call give the same arrays."""
    import tsdf_amd
    vol, exp, base = scene.reference(min_weight, bounded)
    b = scene.bounds if bounded else None
    eng = scene.eng
    if grid:  # the knob is read when an engine is created: the same frames into a second engine
        monkeypatch.setenv("TSDF_MESH_GRID", str(grid))
        eng = tsdf_amd.Engine(VOXEL, TRUNC, max_width=96, max_height=72, num_block_bits=NB_BITS)
    try:
        if grid:
            integrate_scene(eng)
        mesh = eng.extract_mesh_indexed(b, MISSING, min_weight)
        soup = eng.extract_mesh(b, MISSING, min_weight)
        assert exp.shape[0] > (20 if bounded else 100)
        assert np.array_equal(soup.view(np.uint32), exp.view(np.uint32))
        corners, amb, both, one = check_mesh(vol, mesh, soup, unambiguous_share=1e-4)
        print(f"min_weight {min_weight} bounded {bounded} grid {grid}: both-valid {both}, one-valid {one}")
        assert both > 0 and one > 0
        assert same_mesh(mesh, base), "differs from the default-grid result"
        assert same_mesh(eng.extract_mesh_indexed(b, MISSING, min_weight), mesh), "a second call differs"
    finally:
        if grid:
            eng.close()


# ---------------------------------------------------------------------------------------------
# hand-built volume
# ---------------------------------------------------------------------------------------------
def hand_built_records(absent):
    """Seven of the eight blocks around the origin (`absent` is not there): a sphere of radius 6.3 voxels
    about the shared corner, a few samples exactly 0, weights 0 / 1 / 3, distinct prob and colour,
    a few NaN probabilities."""
    import tsdf_amd
    rng = np.random.default_rng(20261019)
    blocks = [(x, y, z) for z in (-1, 0) for y in (-1, 0) for x in (-1, 0) if (x, y, z) != absent]
    recs = np.zeros((len(blocks), tsdf_amd.BLOCK_RECORD_BYTES), np.uint8)
    lx, ly, lz = (np.arange(512) & 7), (np.arange(512) >> 3) & 7, np.arange(512) >> 6
    zeros = 0
    for i, (bx, by, bz) in enumerate(blocks):
        g = np.stack([8 * bx + lx, 8 * by + ly, 8 * bz + lz], 1).astype(np.float64)
        dist = np.sqrt(((g + 0.5) ** 2).sum(axis=1))  # from the corner the eight blocks share
        tsdf = np.clip((dist - 6.3) * 0.25, -1, 1).astype(f32)
        near = np.flatnonzero(np.abs(dist - 6.3) < 0.4)
        pick = near[::max(1, near.size // 3)][:3]  # exactly 0: several edges meet in one position
        tsdf[pick] = 0.0
        zeros += pick.size
        prob = (rng.permutation(512).astype(f32) + f32(i * 512 + 1)) / f32(4096)
        prob[rng.choice(512, 4, replace=False)] = np.nan
        rgbw = np.zeros((512, 4), np.uint8)
        rgbw[:, :3] = rng.integers(0, 256, (512, 3))
        rgbw[:, 3] = rng.choice([0, 1, 3], 512, p=[0.15, 0.15, 0.7])
        recs[i, :8] = np.array([bx, by, bz, 0], np.int16).view(np.uint8)
        recs[i, 16:16 + 2048] = tsdf.view(np.uint8)
        recs[i, 16 + 2048:16 + 4096] = prob.view(np.uint8)
        recs[i, 16 + 4096:] = rgbw.reshape(-1)
    assert zeros >= 7
    return recs


@pytest.mark.parametrize("absent", [(0, 0, 0), (-1, -1, -1)])
def test_hand_built_volume(absent):
    """Checks 1-5 on seven blocks around the origin with min_weight = 2: vertices shared across block
    faces, edges and the corner, coincident vertices (samples exactly 0) and NaN probabilities.
    Without block (0, 0, 0) every crossed edge has its lower endpoint in a present block; without
    (-1, -1, -1) its three neighbours own edges through their upper endpoint. The share of
    position-ambiguous corners is not bounded here: the volume is built to have them."""
    import tsdf_amd
    eng = tsdf_amd.Engine(0.01, 0.04, max_width=64, max_height=64, num_block_bits=10)
    try:
        eng.import_blocks(hand_built_records(absent), replace=True)
        vol = Volume(eng.dump(), 0.01, MISSING, 2)
        assert vol.n == 7
        mesh = eng.extract_mesh_indexed(None, MISSING, 2)
        soup = eng.extract_mesh(None, MISSING, 2)
        corners, amb, both, one = check_mesh(vol, mesh, soup)
        print(f"hand-built: corners {corners}, ambiguous {amb}, both-valid {both}, one-valid {one}")
        assert amb > 0 and both > 0 and one > 0
        # coincident vertices stay apart, upper-owned edges exist, NaN probabilities came through
        assert np.unique(mesh["positions"], axis=0).shape[0] < mesh["positions"].shape[0]
        o = vol.order_key(mesh["keys"])
        upper_owned = int(((o[1] == -1) | (o[2] == -1) | (o[3] == -1)).sum())
        print(f"hand-built: upper-owned edges {upper_owned}")
        assert (upper_owned > 0) == (absent == (-1, -1, -1))
        assert np.isnan(mesh["prob"]).any()
        assert same_mesh(eng.extract_mesh_indexed(None, MISSING, 2), mesh)
        dev = eng.extract_mesh_indexed(None, MISSING, 2, device=True)
        assert same_mesh({k: v.cpu().numpy() for k, v in dev.items()}, mesh)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------
# capacity, device form, facade
# ---------------------------------------------------------------------------------------------
def test_capacity_and_device_form(scene):
    """Device form: a vertex or a triangle capacity one short returns TSDF_ERR_CAPACITY with both
    counts set and the sentinel-filled buffers untouched; with room it equals the host form, as does
    Engine.extract_mesh_indexed(device=True) (which retries once with the returned counts)."""
    import torch
    import tsdf_amd
    from tsdf_amd import _lib
    L = tsdf_amd.load_library()
    eng = scene.eng
    _, _, host = scene.reference(0, False)
    n, m = host["positions"].shape[0], host["indices"].shape[0]

    def buffers(vcap, tcap):
        return dict(positions=torch.full((vcap, 3), -7.0, dtype=torch.float32, device="cuda"),
                    rgba=torch.full((vcap, 4), 201, dtype=torch.uint8, device="cuda"),
                    prob=torch.full((vcap,), -7.0, dtype=torch.float32, device="cuda"),
                    keys=torch.full((vcap, 4), -7, dtype=torch.int32, device="cuda"),
                    indices=torch.full((tcap, 3), -7, dtype=torch.int32, device="cuda"))

    def call(a, vcap, tcap):
        out = _lib.MeshOut(*(C.c_void_p(a[k].data_ptr()) for k in ARRAYS[:4]),
                           C.c_void_p(a["indices"].data_ptr()), vcap, tcap, tsdf_amd.TSDF_MEM_DEVICE)
        nv, nt = C.c_int64(-1), C.c_int64(-1)
        eng._wait_torch(*a.values())
        rc = L.tsdf_extract_mesh_indexed(eng._h, None, MISSING, 0, C.byref(out), C.byref(nv), C.byref(nt))
        eng._signal_torch(*a.values())
        return rc, nv.value, nt.value

    sentinel = {k: v.cpu().numpy() for k, v in buffers(n, m).items()}
    for vcap, tcap in ((n - 1, m), (n, m - 1)):
        a = buffers(n, m)
        rc, nv, nt = call(a, vcap, tcap)
        assert rc == _lib.TSDF_ERR_CAPACITY and (nv, nt) == (n, m)
        assert same_mesh({k: v.cpu().numpy() for k, v in a.items()}, sentinel), "a refused call wrote"
    a = buffers(n + 5, m + 5)
    rc, nv, nt = call(a, n + 5, m + 5)
    assert rc == 0 and (nv, nt) == (n, m)
    got = {k: v.cpu().numpy() for k, v in a.items()}
    assert same_mesh({k: got[k][:m] if k == "indices" else got[k][:n] for k in ARRAYS}, host)
    assert all((got[k][m:] if k == "indices" else got[k][n:]).size > 0 and
               np.array_equal(got[k][m:] if k == "indices" else got[k][n:],
                              sentinel[k][:5]) for k in ARRAYS), "wrote past the counts"
    # counts only
    nv, nt = C.c_int64(-1), C.c_int64(-1)
    assert L.tsdf_extract_mesh_indexed(eng._h, None, MISSING, 0, None, C.byref(nv), C.byref(nt)) == 0
    assert (nv.value, nt.value) == (n, m)
    # the wrapper: a first guess that is too small, then one that fits
    for caps in ((16, 16), (n + 1, m + 1)):
        eng._mesh_caps = caps
        dev = eng.extract_mesh_indexed(None, MISSING, 0, device=True)
        assert all(v.is_cuda for v in dev.values())
        assert same_mesh({k: v.cpu().numpy() for k, v in dev.items()}, host)
    # positions and indices alone; both are required
    a = buffers(n, m)
    out = _lib.MeshOut(C.c_void_p(a["positions"].data_ptr()), None, None, None,
                       C.c_void_p(a["indices"].data_ptr()), n, m, tsdf_amd.TSDF_MEM_DEVICE)
    eng._wait_torch(*a.values())
    assert L.tsdf_extract_mesh_indexed(eng._h, None, MISSING, 0, C.byref(out), C.byref(nv), C.byref(nt)) == 0
    eng._signal_torch(*a.values())
    assert np.array_equal(a["positions"].cpu().numpy().view(np.uint32), host["positions"].view(np.uint32))
    assert np.array_equal(a["indices"].cpu().numpy(), host["indices"])
    assert np.array_equal(a["keys"].cpu().numpy(), sentinel["keys"])
    out.indices = None
    assert L.tsdf_extract_mesh_indexed(eng._h, None, MISSING, 0, C.byref(out), C.byref(nv), C.byref(nt)) == 1


def test_shard_engine_is_refused():
    import tsdf_amd
    eng = tsdf_amd.Engine(VOXEL, TRUNC, max_width=64, max_height=64, num_block_bits=10, shard_index=0,
                          shard_count=2)
    try:
        with pytest.raises(tsdf_amd.TSDFError, match="shard"):
            eng.extract_mesh_indexed()
    finally:
        eng.close()


def test_facade_mesh_main(scene, tmp_path):
    """TSDFGrid::ExtractMesh through mesh_main on the scene's packed blocks == the Python result on
    the same imported blocks, and the same mesh as the scene's own (as a set of keyed vertices)."""
    import tsdf_amd
    recs = scene.eng.pack_blocks()
    recs.tofile(tmp_path / "blocks.bin")
    (tmp_path / "meta.txt").write_text(f"{VOXEL} {TRUNC} {NB_BITS} {MISSING} 1\n")
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    eng = tsdf_amd.Engine(VOXEL, TRUNC, max_width=64, max_height=64, num_block_bits=NB_BITS)
    try:
        eng.import_blocks(recs, replace=True)
        py = eng.extract_mesh_indexed(None, MISSING, 1)
    finally:
        eng.close()
    n, m = map(int, (tmp_path / "out_counts.txt").read_text().split())
    assert (n, m) == (py["positions"].shape[0], py["indices"].shape[0]) and n > 0 and m > 0
    verts = np.fromfile(tmp_path / "out_verts.bin", f32).reshape(-1, 3)
    assert np.array_equal(verts.view(np.uint32), py["positions"].view(np.uint32))
    assert np.array_equal(np.fromfile(tmp_path / "out_tris.bin", np.int32).reshape(-1, 3), py["indices"])
    assert np.array_equal(np.fromfile(tmp_path / "out_rgba.bin", np.uint8).reshape(-1, 4), py["rgba"])
    assert same_floats(np.fromfile(tmp_path / "out_prob.bin", f32), py["prob"])
    # the imported volume is the scene's: the same vertices whatever order its entries took
    ref = scene.reference(1, False)[2]
    assert (n, m) == (ref["positions"].shape[0], ref["indices"].shape[0])
    o, p = np.lexsort(py["keys"].T[::-1]), np.lexsort(ref["keys"].T[::-1])
    assert np.array_equal(py["keys"][o], ref["keys"][p])
    assert np.array_equal(py["positions"][o].view(np.uint32), ref["positions"][p].view(np.uint32))
    assert np.array_equal(py["rgba"][o], ref["rgba"][p]) and same_floats(py["prob"][o], ref["prob"][p])
