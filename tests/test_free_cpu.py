"""Observed free space without a GPU: the numpy restatement of the contract (tests/_free_ref.py) against the
CPU oracle's voxel update, the census of the geometric gates the GPU tests then stand on, the wall-with-a-gap
scenario on the restatements alone, and the layers above the C ABI that need no device (the layer helpers,
the exported symbols). Every comparison is exact."""
import numpy as np
import pytest

import _free_cases as fc
import _free_ref as fref
import _geo_edges as ge

f32 = np.float32


@pytest.mark.parametrize("frame, compared, free", [(0, 102990, 33519), (40, 124389, 64115), (200, 106693, 35277)])
def test_restatement_against_the_oracle(frame, compared, free):
    """One synth frame into an empty oracle volume: on every voxel of every live block with fusion weight >= 1
    and hz > 0, the update wrote tsdf == 1.0 exactly where free() holds. Nothing else is excluded."""
    from _oracle import OracleGrid
    from tsdf_amd import synth
    cam = synth.camera(80, 60)
    s = synth.render(cam, frame)
    ora = OracleGrid(0.02, 0.08, 14)
    try:
        ora.integrate(s["rgb"], s["depth"], s["ht"], s["lt"], 4.0, cam.K, s["q"], s["t"])
        d = ora.dump()
    finally:
        ora.close()
    live = np.flatnonzero(d["entry_idx"] >= 0)
    idx = d["entry_idx"][live]
    g = d["entry_pos"][live, :3].astype(np.int64)[:, None, :] * 8 + ge._OFF[None]
    weight = d["rgbw"].reshape(-1, 512, 4)[idx][..., 3]
    tsdf = d["tsdf"].reshape(-1, 512)[idx]
    T = fref.terms(g, fref.frame(s["depth"], cam.K, s["q"], s["t"], 4.0), 0.02, 0.08)
    sel = (weight >= 1) & (T["hz"] > 0)
    n_sel, n_free = int(sel.sum()), int((sel & T["free"]).sum())
    wrong = int((sel & ((tsdf == f32(1)) != T["free"])).sum())
    print(f"frame {frame}: compared {n_sel}, free {n_free}, mismatches {wrong}")
    assert n_sel > 50000 and n_free > 20000
    assert wrong == 0
    assert (n_sel, n_free) == (compared, free)


def test_gate_census():
    """The census frames put voxels on every gate of the contract, and where they decide, they decide as the
    contract says."""
    assert np.array([fc.BELOW_DEPTH_BITS], np.uint32).view(f32)[0] == f32(0.029909586533904076)
    total = dict.fromkeys(fc.GATES, 0)
    for name in fc.CENSUS_FRAMES:
        T = fc.census_terms(name)
        n = fc.gates(T)
        print(name, n, "free", int(T["free"].sum()))
        for k, v in n.items():
            total[k] += v
        # the gates' verdicts: a quotient of -1/2 or size - 1/2 rounds out of the image, hz <= 0 is never free
        with np.errstate(invalid="ignore"):
            assert not (T["free"] & ((T["uq"] == f32(-0.5)) | (T["vq"] == f32(-0.5)) | (T["uq"] == f32(ge.W - 0.5)) |
                                     (T["vq"] == f32(ge.H - 0.5)))).any()
            assert not (T["free"] & ~(T["hz"] > 0)).any()
            assert not (T["free"] & ((T["d"] == 0) | (T["d"] > ge.MAX_DEPTH))).any()
            assert not (T["free"] & (T["sdf"] < f32(ge.TRUNC))).any()
    print("total", total)
    for k in fc.GATES:
        assert total[k] > 0, k
    # the voxel the own frame was made for
    T = fc.census_terms("below")
    x, y, z = (np.array(fc.BELOW_VOXEL) - np.array(fc.CENSUS_ORIGIN)).tolist()
    assert (int(T["v"][z, y, x]), int(T["u"][z, y, x])) == fc.BELOW_PIXEL
    assert T["sdf"][z, y, x] == np.nextafter(f32(ge.TRUNC), f32(0)) and T["valid"][z, y, x] and not T["free"][z, y, x]
    # the camera centre under pose A: 0 / 0 is NaN, the conversion gives pixel (0, 0), and only hz > 0 says no
    x, y, z = (-np.array(fc.CENSUS_ORIGIN)).tolist()
    T = fc.census_terms(0)
    assert T["hz"][z, y, x] == 0 and np.isnan(T["uq"][z, y, x]) and T["valid"][z, y, x] and not T["free"][z, y, x]


def test_scenario_wall_with_a_gap():
    """The volume alone either does not start (unknown_free = 0) or leaks through the unobserved gap
    (unknown_free = 1); with the observed-free layer applied the strict field floods the room and stays in it."""
    s = fc.scenario()
    st, m = s["field"]["state"], s["mask"]
    bits = (int(m.sum()), int((m & (st == 0)).sum()), int((m & (st == 2)).sum()))
    print("bits set, on state 0, on state 2:", bits, "promoted", s["promoted"][1])
    assert bits == (46319, 44832, 0) and s["promoted"][1] == 44832
    strict, optimistic, promoted = (s["cost"][k] for k in ("volume_strict", "volume_optimistic", "promoted"))
    assert strict[1] == 0 and fc.reached(strict[0]) == (0, 0, 0)
    print("optimistic", fc.reached(optimistic[0]), "promoted", fc.reached(promoted[0]))
    assert optimistic[1] == 1 and fc.reached(optimistic[0])[1] > 0
    assert promoted[1] == 1 and fc.reached(promoted[0])[0] > 0 and fc.reached(promoted[0])[1] == 0
    assert fc.reached(optimistic[0])[:2] == (166584, 48000)
    assert fc.reached(promoted[0]) == (50766, 0, 187)


def test_apply_restatement_and_layer_helpers():
    """pack / unpack, esdf.free_layer / free_mask / free_fraction, and apply on boxes that nest, overlap partly
    and are disjoint."""
    from tsdf_amd import esdf
    rng = np.random.default_rng(3)
    for nx in (1, 31, 32, 33, 64, 65):
        mask = rng.random((3, 2, nx)) < 0.5
        layer = esdf.free_layer((5, -7, 2), (nx, 2, 3))
        assert layer["bits"].shape == (3, 2, (nx + 31) // 32) and layer["bits"].dtype == np.uint32 and not layer["bits"].any()
        layer["bits"] |= fref.pack(mask)
        assert fref.padding(layer["bits"], nx) == 0
        assert np.array_equal(fref.unpack(layer["bits"], nx), mask) and np.array_equal(esdf.free_mask(layer), mask)
        assert esdf.free_fraction(layer) == mask.sum() / mask.size
    mask = rng.random((6, 5, 40)) < 0.6
    lo = (10, 20, 30)
    for origin, dims, some in (((12, 21, 31), (20, 3, 4), True), ((-5, 18, 28), (30, 9, 5), True),
                               ((10, 20, 30), (40, 5, 6), True), ((60, 20, 30), (8, 5, 6), False)):
        state = rng.integers(0, 3, dims[::-1]).astype(np.uint8)
        out, n = fref.apply(mask, lo, state, origin)
        assert (n > 0) == some and n == int((out != state).sum())
        assert np.array_equal(out[state != 0], state[state != 0]) and set(np.unique(out[out != state])) <= {1}
        # voxel by voxel
        for z, y, x in np.argwhere(state == 0)[::7]:
            l = np.array(origin) + (x, y, z) - lo
            inside = (l >= 0).all() and (l < (40, 5, 6)).all()
            assert out[z, y, x] == (1 if inside and mask[l[2], l[1], l[0]] else 0)


def test_the_library_exports_the_calls():
    import ctypes as C
    import tsdf_amd
    lib = tsdf_amd._lib
    L = lib.load()
    for name in ("tsdf_free_words", "tsdf_free_observe", "tsdf_free_apply"):
        assert name in lib.EXPORTS and hasattr(L, name)
    words = lambda *d: L.tsdf_free_words((C.c_int32 * 3)(*d))
    assert words(1, 1, 1) == 1 and words(32, 2, 3) == 6 and words(33, 2, 3) == 12 and words(2048, 2048, 64) == 64 * 2048 * 64
    assert words(0, 1, 1) == 0 and words(2049, 1, 1) == 0 and words(2048, 2048, 65) == 0 and words(4, -1, 4) == 0
    assert L.tsdf_free_words(None) == 0
    for name in ("free_observe", "free_apply"):
        assert callable(getattr(tsdf_amd.Engine, name))
