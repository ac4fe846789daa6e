"""The geometric gate-edge stream (tests/_geo_edges.py) really stands on every comparison and rounding
of the voxel update and of the visibility test, checked on the CPU oracle alone with the stream's own
float32 census (_geo_edges.gates): otherwise the bit-for-bit GPU comparison on it
(tests/test_gpu_geo_edges.py) could pass vacuously. These are conditions on the test's input, not
tolerances. Measured on the oracle over the 36 frames (the asserted floor in brackets):

  updated voxels with u on a tie 137 841 (60 000), with v on a tie 137 643 (60 000);
  quotient exactly -0.5 with the other coordinate in range 4 662 (2 000);
  quotient exactly W - 0.5 or H - 0.5, likewise 4 606 (2 000);
  updated ties that round onto the last column or row 2 984 (1 000);
  updated voxels with ph.z < 0: 92 in every pose-B frame, 1 380 (600);
  the 0 / 0 voxel updated: once per pose-B frame and in frame 0 under A, 16 (10);
  sdf == -trunc with valid depth, not updated 270 (100); sdf == trunc, updated 153 (60);
  wc on k + 0.5: 596 885 (250 000), of which k even 328 299 (120 000);
  wc == 0.5 over the first 24 frames 103 007 (40 000);
  updates with wc > 40: 25 031, all from frame 33 on (8 000); voxels at weight 40 at the end 11 254 (4 000);
  colour quotients on k + 0.5 over the first 24 frames 90 712 (30 000);
  block corners exactly on an image edge and visible: 472 - 476 per pose-A frame from frame 10 on, 8 346
  in all; fully visible blocks with such a corner 230 - 232; partially visible blocks in the update
  list 33 in every pose-B frame, 55 - 187 in the pose-A frames;
  peak 3 842 visible blocks of 2^13, the pool never exhausted;
  DDA sample coordinates on k + 0.5 (_geo_edges.dda_ties; counted, not a condition): none -- the central
  pixel's samples are whole voxels, and no other ray's land on a half.

The hook's one Allocate launch creates 63 of the 64 seed blocks (one ring key loses its bucket's lock
to another seed, as in the reference's launch; the DDA of frame 11 creates it). The four origin blocks
at block z = 0 are carved in frame 0 (every voxel the 64-voxel plane updates gets tsdf 1); the four at
z = -1 straddle pose B's camera plane and live on the 6-voxel frames: 3 of them and all 56 ring blocks
are alive at the end. The census equals the oracle's last_num_updated on 23 frames, among them all 21
in which no block is both created and carved.
"""
import collections

import numpy as np

import _geo_edges as ge

FLOORS = dict(u_tie=60000, v_tie=60000, minus_half=2000, size_minus_half_in=2000, last_tie_updated=1000,
              behind=600, zero_over_zero=10, sdf_minus_trunc=100, sdf_plus_trunc=60, wc_half=250000,
              wc_half_even=120000, wc_over_cap=8000)
FLOORS_24 = dict(wc_is_half=40000, colour_half=30000)  # over the first 24 frames


def test_stream_inputs_are_dyadic_and_sit_on_the_pixel_gates():
    frames = list(ge.frames(ge.FRAMES))
    assert ge.PLAN[0] == (64, "A") and len(frames) == 36
    assert np.float32(ge.VOXEL) == ge.VOXEL and np.float32(ge.TRUNC) == 4 * ge.VOXEL and ge.MAX_DEPTH == 1
    rng = ge.ray_lengths()
    assert rng.dtype == np.float32
    assert [float(rng[v, u]) for u, v in ge.ZERO_OFFSET] == [1.0, 1.25, 1.25, 1.25]
    for f, fr in enumerate(frames):
        plane, name = ge.PLAN[f % 12]
        d = fr["depth"]
        assert d.dtype == np.float32 and d.shape == (ge.H, ge.W) and fr["rgb"].shape == (ge.H, ge.W, 3)
        assert fr["ht"] is None and fr["lt"] is None and fr["pose"] == name
        assert np.array_equal(fr["q"], [0, 0, 0, 1]) and np.array_equal(fr["t"], [0, 0, 4 * ge.VOXEL * (name == "B")])
        assert d[5, 7] == 0 and d[40, 50] == ge.MAX_DEPTH
        assert d[41, 50] > ge.MAX_DEPTH and np.nextafter(d[41, 50], np.float32(0)) == ge.MAX_DEPTH
        keep = np.ones(d.shape, bool)
        keep[5, 7] = keep[40, 50] = keep[41, 50] = False
        half = d.astype(np.float64)[keep] * 256  # every depth is a whole number of half voxels, exactly
        assert np.array_equal(half, np.round(half))
        for u, v in ge.ZERO_OFFSET:
            assert d[v, u] * 128 == plane
        assert set(np.unique(half / 2 - plane)) == {-2, -1.5, -1, -0.5, 0, 0.5, 1, 1.5, 2}
    assert not np.array_equal(frames[0]["rgb"], frames[12]["rgb"]) and len(np.unique(frames[0]["rgb"])) == 256
    # w_new at the planes, in the update's own float operations
    w_new = {p: float((np.float32(1) - np.float32(p * ge.VOXEL) / ge.MAX_DEPTH) * np.float32(4)) for p, _ in ge.PLAN}
    assert [w_new[p] for p in (64, 32, 96, 112, 128)] == [2, 3, 1, 0.5, 0]
    # pose A: the corners at Z = 32 voxels project exactly onto the first / last column and row
    g = np.array([(-32, 0, 32), (31, 0, 32), (0, -24, 32), (0, 23, 32)])
    u, v, _, _ = ge._project(g, ge.T["A"])
    assert (float(u[0]), float(u[1]), float(v[2]), float(v[3])) == (0, ge.W - 1, 0, ge.H - 1)
    # pose B: the camera centre is a grid point, the block row z = -1 straddles the camera plane
    u, v, z, _ = ge._project(np.array([(0, 0, -4), (1, 0, -8), (1, 0, -1)]), ge.T["B"])
    assert np.isnan(u[0]) and np.isnan(v[0]) and z[0] == 0 and z[1] < 0 < z[2]
    # DDA sample coordinates on a rounding tie: counted, not a condition (measured: none)
    print("DDA sample coordinates on k + 0.5:", sum(ge.dda_ties(fr) for fr in frames))
    seeds = ge.seed_keys()
    assert seeds.shape == (64, 3) and len(set(map(tuple, seeds.tolist()))) == 64


def test_stream_stands_on_every_gate_on_the_oracle():
    state, rows = {}, []
    origin = set(map(tuple, ge.origin_keys().tolist()))
    ring = set(map(tuple, ge.ring_keys().tolist()))

    def each(f, fr, ora):
        d, s = ora.dump(), ora.stats()
        if f < 0:
            assert s["active_blocks"] >= 60, s  # (a key that loses its bucket's lock is dropped)
            live = ge.live_keys(d)
            assert len(live & origin) == 8 and len(live & ring) >= 52
        else:
            assert s["pool_exhausted"] == 0, (f, s)
            g = ge.gates(fr, state["dump"], d)
            live = ge.live_keys(d)
            rows.append((fr["pose"], s, g, len(live & origin), len(live & ring)))
        state["dump"] = d

    ge.run_oracle(ge.FRAMES, keep=(), each=each)
    assert len(rows) == ge.FRAMES
    tot, tot24 = collections.Counter(), collections.Counter()
    clean = 0
    for f, (name, s, g, _, _) in enumerate(rows):
        print(f, name, {k: s[k] for k in ("last_num_visible", "last_num_updated", "last_num_alloc", "last_num_deleted")}, g)
        tot.update(g)
        if f < 24:
            tot24.update(g)
        # the census is the oracle's update, voxel for voxel, wherever the dumps show every block
        if g["new_blocks"] == s["last_num_alloc"]:
            clean += 1
            assert g["updated"] == s["last_num_updated"], (f, g, s)
            assert g["visible"] == s["last_num_visible"], (f, g, s)
        if name == "B":
            assert g["behind"] == 92 and g["zero_over_zero"] == 1, (f, g)
            assert g["partial"] >= 33, (f, g)
        else:
            assert g["behind"] == 0 and g["zero_over_zero"] == (f == 0), (f, g)
            assert g["partial"] >= 55, (f, g)
            if f >= 6:
                assert g["corners_on_edge"] > 0 and g["full_with_edge_corner"] > 0, (f, g)
            if f >= 10:
                assert g["corners_on_edge"] >= 472 and g["full_with_edge_corner"] >= 230, (f, g)
        assert (g["wc_over_cap"] > 0) == (f >= 33), (f, g)
    print("total", dict(tot), "first 24", dict(tot24))
    assert clean >= 20, clean
    for k, floor in FLOORS.items():
        assert tot[k] >= floor, (k, tot[k], floor)
    for k, floor in FLOORS_24.items():
        assert tot24[k] >= floor, (k, tot24[k], floor)
    assert tot["corners_on_edge"] >= 8000, tot["corners_on_edge"]
    assert max(s["last_num_visible"] for _, s, _, _, _ in rows) <= 4096
    # the seed blocks of both kinds are alive at the end; many voxels sit at the weight cap
    assert rows[-1][3] >= 1 and rows[-1][4] >= 52, rows[-1][3:]
    d = state["dump"]
    pool = d["entry_idx"][d["entry_idx"] >= 0]
    at_cap = int((d["rgbw"].reshape(-1, 512, 4)[pool, :, 3] == 40).sum())
    assert at_cap >= 4000, at_cap


def test_snapshots_reproduce_the_oracle_dumps():
    """The compact per-frame states the GPU tests compare against (the hash table changes in every frame
    of this stream, so Snapshot keeps its changed entries only) are the oracle's dumps, bit for bit."""
    kept = {}

    def each(f, fr, ora):
        if f >= 0:
            kept[f] = (ora.dump(), ora.stats())

    snaps = ge.run_oracle(4, each=each)
    for f, (b, st) in kept.items():
        a = snaps[f].dump()
        assert a.keys() == b.keys() and a["free"] == b["free"]
        for k in b:
            if k != "free":
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
                assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (f, k)
        assert snaps[f].stats() == st
        assert "tsdf" not in snaps[f].dump(pool=False)
    assert not np.array_equal(kept[0][0]["entry_idx"], kept[3][0]["entry_idx"])
