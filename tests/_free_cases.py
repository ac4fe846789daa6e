"""The observed-free-space tests' shared cases (TEST INFRASTRUCTURE, numpy and the CPU oracle only): the gate
census stream and the wall-with-a-gap scenario, each computed once. tests/test_free_cpu.py asserts on them
with the restatement alone; tests/test_gpu_free.py compares the engine with them bit for bit.

Census: the dyadic setting of tests/_geo_edges.py (64 x 48, K = (32, 32, 32, 24), voxel 2^-7, truncation 2^-5,
max_depth 1, poses A and B, exact arithmetic) over a box that spans the camera plane and is wide enough for
the quotients -1/2 and W - 1/2, H - 1/2 (at Z = 64 voxels: gx = -65 and 63, gy = -49 and 47). Frames 0 (A,
plane 64), 5 (B, 96), 8 (A, 128: most pixels at max_depth exactly) and 11 (B, 64) of that stream, and one
frame of this file: frame 3 (A, plane 32) with depth[24, 0] set to the float 0x3CF504F3. No dyadic depth puts
a voxel's sdf one ulp below the truncation (at ray length 1 that needs a depth with 26 significant bits), so
this pixel's is not: voxel (-1, 0, 1) projects onto it with hz = 2^-7, and ray length times (d - hz) rounds
to pred(2^-5). Everything else in that frame stays exact.

Scenario: a wall with a gap nobody looked through. Camera 64 x 48, K = (60, 60, 31.5, 23.5), identity pose,
depth 0.6 m everywhere except an 8 x 8 pixel hole of depth 0; voxel 0.01, truncation 0.04, max_depth 2, three
integrations into the oracle; the distance field of the box (-24, -20, 2) + (48, 40, 90) with max_dist 16, a
layer over the same box observing the same frame, clearance2 4, a seed 6 cm in front of the camera."""
import functools

import numpy as np

import _free_ref as fref
import _geo_edges as ge

f32 = np.float32

# ---- census ----
CENSUS_ORIGIN, CENSUS_DIMS = (-72, -56, -12), (144, 112, 84)
CENSUS_FRAMES = (0, 5, 8, 11, "below")
BELOW_PIXEL, BELOW_DEPTH_BITS, BELOW_VOXEL = (24, 0), 0x3CF504F3, (-1, 0, 1)  # (row, column)
GATES = ("sdf_at_trunc", "sdf_below_trunc", "tie", "minus_half", "size_minus_half", "hz_zero", "hz_zero_else_free",
         "behind_else_free", "d_at_max_free", "d_above_max", "d_zero")


@functools.lru_cache(None)
def census_frames():
    """{name: frame dict of _free_ref.frame} in CENSUS_FRAMES order."""
    stream = list(ge.frames(12))
    own = dict(stream[3], depth=stream[3]["depth"].copy())
    own["depth"][BELOW_PIXEL] = np.array([BELOW_DEPTH_BITS], np.uint32).view(f32)[0]
    pick = {k: stream[k] for k in CENSUS_FRAMES if k != "below"}
    pick["below"] = own
    return {k: fref.frame(s["depth"], ge.K, s["q"], s["t"], ge.MAX_DEPTH) for k, s in pick.items()}


@functools.lru_cache(None)
def census_terms(name):
    return fref.terms(fref.box_points(CENSUS_ORIGIN, CENSUS_DIMS), census_frames()[name], ge.VOXEL, ge.TRUNC)


def gates(T):
    """The voxels of one frame's terms on each gate. *_else_free: only hz > 0 keeps the voxel from being free."""
    W, H, trunc = ge.W, ge.H, f32(ge.TRUNC)
    front = T["hz"] > 0
    u_in, v_in = (T["u"] >= 0) & (T["u"] < W), (T["v"] >= 0) & (T["v"] < H)
    with np.errstate(invalid="ignore"):
        would = T["valid"] & (T["sdf"] >= trunc)
        n = dict(
            sdf_at_trunc=T["free"] & (T["sdf"] == trunc),
            sdf_below_trunc=T["valid"] & front & (T["sdf"] == np.nextafter(trunc, f32(0))),
            tie=T["free"] & (ge._on_half(T["uq"]) | ge._on_half(T["vq"])),
            minus_half=front & (((T["uq"] == f32(-0.5)) & v_in) | ((T["vq"] == f32(-0.5)) & u_in)),
            size_minus_half=front & (((T["uq"] == f32(W - 0.5)) & v_in) | ((T["vq"] == f32(H - 0.5)) & u_in)),
            hz_zero=T["hz"] == 0,
            hz_zero_else_free=(T["hz"] == 0) & would,
            behind_else_free=(T["hz"] < 0) & would,
            d_at_max_free=T["free"] & (T["d"] == ge.MAX_DEPTH),
            d_above_max=T["inb"] & front & (T["d"] == np.nextafter(ge.MAX_DEPTH, f32(np.inf))),
            d_zero=T["inb"] & front & (T["d"] == 0))
    return {k: int(v.sum()) for k, v in n.items()}


# ---- scenario ----
S_W, S_H = 64, 48
S_K = np.array([60, 60, 31.5, 23.5], f32)
S_Q, S_T = np.array([0, 0, 0, 1], f32), np.zeros(3, f32)
S_VOXEL, S_TRUNC, S_MAX_DEPTH, S_NB_BITS = 0.01, 0.04, 2.0, 13
S_ORIGIN, S_DIMS, S_MAX_DIST, S_CLEARANCE2 = (-24, -20, 2), (48, 40, 90), 16, 4
S_SEED_LOCAL = (24, 20, 8)
S_WALL_Z = 66  # global z beyond which a voxel is behind the wall


def scenario_depth():
    depth = np.full((S_H, S_W), 0.6, f32)
    depth[20:28, 44:52] = 0
    return depth


@functools.lru_cache(None)
def scenario():
    """dict(field: the restatement's distance field on the oracle's volume, mask: the frame's free mask over
    the box, promoted: (state, count), cost: {"volume_strict", "volume_optimistic", "promoted"} -> (cost,
    seeded) by Dijkstra)."""
    import _edt_ref
    import _travel_ref as tr
    from _oracle import OracleGrid
    depth = scenario_depth()
    ora = OracleGrid(S_VOXEL, S_TRUNC, S_NB_BITS)
    try:
        for _ in range(3):
            ora.integrate(np.zeros((S_H, S_W, 3), np.uint8), depth, None, None, S_MAX_DEPTH, S_K, S_Q, S_T)
        dump = ora.dump()
    finally:
        ora.close()
    field = _edt_ref.distance_field(dump, S_ORIGIN, S_DIMS, max_dist=S_MAX_DIST)
    mask = fref.frame_mask(S_ORIGIN, S_DIMS, fref.frame(depth, S_K, S_Q, S_T, S_MAX_DEPTH), S_VOXEL, S_TRUNC)
    promoted = fref.apply(mask, S_ORIGIN, field["state"], S_ORIGIN)
    cost = {}
    for name, state, unknown_free in (("volume_strict", field["state"], False), ("volume_optimistic", field["state"], True),
                                      ("promoted", promoted[0], False)):
        cost[name] = tr.field(tr.passable(field["d2"], state, S_CLEARANCE2, unknown_free), [S_SEED_LOCAL])
    return dict(field=field, mask=mask, promoted=promoted, cost=cost, dump=dump)


def reached(cost):
    """(voxels reached, of them behind the wall, the largest cost or 0)."""
    r = cost != 0xFFFFFFFF
    z = np.arange(S_DIMS[2])[:, None, None] + S_ORIGIN[2]
    return int(r.sum()), int((r & (z > S_WALL_Z)).sum()), int(cost[r].max()) if r.any() else 0
