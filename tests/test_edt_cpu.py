"""The distance field's restatement (tests/_edt_ref.py) against brute force and scipy, its classes on the
analytic scene, and the tsdf_amd.esdf helpers. No GPU, no engine library."""
import numpy as np
import pytest

import _edt_ref
from tsdf_amd import esdf


def brute(site, R):
    """min(R^2, min over the sites of |v - s|^2), every pair."""
    nz, ny, nx = site.shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.stack([z, y, x], -1).reshape(-1, 1, 3).astype(np.int64)
    s = np.argwhere(site).reshape(1, -1, 3).astype(np.int64)
    if s.shape[1] == 0:
        return np.full(site.shape, R * R, np.uint16)
    d = ((v - s) ** 2).sum(axis=-1).min(axis=1)
    return np.minimum(d, R * R).astype(np.uint16).reshape(site.shape)


def test_transform_is_the_brute_force_minimum():
    rng = np.random.default_rng(7)
    shapes = [(7, 9, 12), (1, 1, 1), (5, 1, 8), (1, 9, 1), (7, 2, 3), (6, 9, 11)]
    for k, shape in enumerate(shapes):
        for density in (0.002, 0.02, 0.3):
            site = rng.random(shape) < density
            for R in (255, 3):
                assert np.array_equal(_edt_ref.transform(site, R), brute(site, R)), (shape, density, R)
    none = np.zeros((7, 9, 12), bool)
    assert (_edt_ref.transform(none, 255) == 255 * 255).all() and (_edt_ref.transform(none, 4) == 16).all()
    one = none.copy()
    one[6, 0, 11] = True
    assert np.array_equal(_edt_ref.transform(one, 255), brute(one, 255))
    assert _edt_ref.transform(one, 255)[0, 8, 0] == 36 + 64 + 121
    assert np.array_equal(_edt_ref.transform(one, 5), brute(one, 5)) and _edt_ref.transform(one, 5).max() == 25
    assert (_edt_ref.transform(~none, 255) == 0).all()


def test_transform_is_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    site = rng.random((9, 14, 17)) < 0.01
    site[4, 7, 3] = True
    want = np.rint(ndi.distance_transform_edt(~site) ** 2).astype(np.int64)
    assert np.array_equal(_edt_ref.transform(site, 255), want.astype(np.uint16))
    assert np.array_equal(_edt_ref.transform(site, 4), np.minimum(want, 16).astype(np.uint16))
    dump = _edt_ref.records_dump(_edt_ref.scene_records())
    f = _edt_ref.distance_field(dump, (-37, -35, -21), (77, 70, 59))
    want = np.rint(ndi.distance_transform_edt(~f["site"]) ** 2).astype(np.int64)
    assert np.array_equal(f["d2"], want.astype(np.uint16))


def test_scene_classes():
    """The figures tests/test_gpu_edt.py relies on, from the restatement alone."""
    dump = _edt_ref.records_dump(_edt_ref.scene_records())
    f = _edt_ref.distance_field(dump, (-37, -35, -21), (77, 70, 59))
    assert int(f["site"].sum()) == 4516
    assert np.bincount(f["state"].ravel(), minlength=3).tolist() == [281502, 19100, 17408]
    assert int(f["d2"].max()) == 2098
    # a site is inside, and no unobserved voxel is one
    assert (f["state"][f["site"]] == 2).all()
    # the site set does not depend on the box: a box whose top face is the floor's top inside layer (its
    # free neighbours outside the box), against the big box's slice
    s, site = _edt_ref.classes(dump, (-20, -18, -12), (33, 29, 5))
    big = (slice(-12 + 21, -7 + 21), slice(-18 + 35, 11 + 35), slice(-20 + 37, 13 + 37))
    assert np.array_equal(s, f["state"][big]) and np.array_equal(site, f["site"][big]) and site[-1].sum() > 800
    # min_weight above the scene's weight: nothing is observed
    s, site = _edt_ref.classes(dump, (-20, -18, -12), (33, 29, 5), min_weight=11)
    assert not s.any() and not site.any()


def field(d2, state, origin, unknown=False):
    d2, state = np.asarray(d2, np.uint16), None if state is None else np.asarray(state, np.uint8)
    return dict(d2=d2, state=state, origin=origin, dims=d2.shape[::-1], max_dist=255, unknown=unknown)


def test_esdf_helpers():
    d2 = np.arange(24, dtype=np.uint16).reshape(2, 3, 4) ** 2
    state = np.array([0, 1, 2], np.uint8)[np.arange(24).reshape(2, 3, 4) % 3]
    f = field(d2, state, (10, -5, 2))
    m = esdf.metres(f, 0.01)
    assert m.dtype == np.float32 and m.shape == (2, 3, 4)
    assert np.array_equal(m, (np.arange(24, dtype=np.float32) * np.float32(0.01)).reshape(2, 3, 4))
    s = esdf.signed(f, 0.01)
    assert s.dtype == np.float32
    assert np.isnan(s[state == 0]).all() and np.array_equal(s[state == 1], m[state == 1])
    assert np.array_equal(s[state == 2], -m[state == 2])
    su = esdf.signed(field(d2, state, (10, -5, 2), unknown=True), 0.01)
    assert not np.isnan(su).any() and np.array_equal(su[state == 0], m[state == 0])
    with pytest.raises(ValueError):
        esdf.signed(field(d2, None, (0, 0, 0)), 0.01)
    # box_around: every point and the margin inside
    pts = np.array([[0.1, -0.2, 0.3], [0.52, 0.0, 0.31], [0.3, 0.11, 0.249]])
    origin, dims = esdf.box_around(pts, 0.01, 0.05)
    lo, hi = np.array(origin), np.array(origin) + np.array(dims) - 1
    assert (lo * 0.01 <= pts.min(axis=0) - 0.05 + 1e-12).all() and (hi * 0.01 >= pts.max(axis=0) + 0.05 - 1e-12).all()
    assert (lo >= np.floor((pts.min(axis=0) - 0.05) / 0.01) - 1).all() and (hi <= np.ceil((pts.max(axis=0) + 0.05) / 0.01) + 1).all()
    assert esdf.box_around(np.array([[0.125, -0.205, 0.3]]), 0.01) == ((12, -21, 30), (2, 2, 1))
    with pytest.raises(ValueError):
        esdf.box_around(np.zeros((0, 3)), 0.01, 0.1)
    # the library's rounding: half away from zero
    v = esdf.voxel_of(np.array([[0.025, -0.025, 0.0049], [-0.0149, 0.0151, -0.2]], np.float32), 0.01)
    assert v.tolist() == [[3, -3, 0], [-1, 2, -20]]
    assert esdf.voxel_of(np.array([[0.03, 0.03, 0.03]], np.float32), 0.01, 0.5).tolist() == [[3, 3, 3]]
    # clearance: nearest-voxel lookup; (0, 0) outside the box
    p = np.array([[0.10, -0.05, 0.02], [0.13, -0.03, 0.03], [0.14, -0.03, 0.03], [0.10, -0.05, 0.04], [0.09, -0.05, 0.02]])
    dist, st = esdf.clearance(f, 0.01, p)
    assert dist.dtype == np.float32 and st.dtype == np.uint8
    assert np.array_equal(dist, np.array([0, 23, 0, 0, 0], np.float32) * np.float32(0.01))
    assert st.tolist() == [0, int(state[1, 2, 3]), 0, 0, 0]
    dist, st = esdf.clearance(field(d2, None, (10, -5, 2)), 0.01, p)
    assert st.tolist() == [1, 1, 0, 0, 0]
