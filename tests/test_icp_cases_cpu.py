"""The hand-built tracking inputs of tests/_icp_cases.py stand where they claim to, shown on the numpy
restatement (tests/_track_ref.py) alone: no GPU. tests/test_gpu_icp_edges.py runs the kernels on them."""
import math

import numpy as np
import pytest

import _icp_cases as ic
import _track_ref as ref

f32 = np.float32


@pytest.fixture(scope="module")
def gates():
    return ic.gate_cases()


def _inputs_that_differ(a, b):
    out = [k for k in ("depth",) if not np.array_equal(a[k], b[k], equal_nan=True)]
    out += ["model." + k for k in ("point", "normal")
            if not np.array_equal(a["model"][k], b["model"][k], equal_nan=True)]
    out += [k for k in ("K", "model_K", "max_dist", "max_depth", "px")
            if tuple(np.ravel(a[k])) != tuple(np.ravel(b[k]))]
    out += [k for k in ("pose", "model_pose")
            if not (np.array_equal(a[k].q, b[k].q) and np.array_equal(a[k].t, b[k].t))]
    return out


def test_icp_terms_is_the_kept_rows_of_icp_terms_full():
    c = ic.tree_case(250, 130)
    for stride in (1, 3):
        t = ic.full_terms(c, stride)
        J, r = ref.icp_terms(c["depth"], c["K"], c["pose"], c["model"], c["model_K"], c["model_pose"], stride,
                             c["max_dist"], c["max_depth"])
        assert np.array_equal(J, t["J"][t["keep"]]) and np.array_equal(r, t["r"][t["keep"]])
        nsx = len(range(0, 250, stride))
        s = np.arange(t["keep"].size)
        assert t["nsx"] == nsx
        assert np.array_equal(t["u"], stride * (s % nsx)) and np.array_equal(t["v"], stride * (s // nsx))
        assert 0 < t["keep"].sum() < t["keep"].size


def test_gate_twins_differ_in_one_input_and_in_the_count(gates):
    """Every case keeps exactly its pixel or nothing, as it claims; its twin claims the opposite and
    differs from it in a single input (the depth, one model map, the model camera or the model pose)."""
    for name, (c, kept, twin, gated) in gates.items():
        t = ic.full_terms(c)
        assert int(t["keep"].sum()) == int(kept), name
        if kept:
            s = int(np.flatnonzero(t["keep"])[0])
            assert (t["u"][s], t["v"][s]) == c["px"], name
        if name == "plain":
            continue
        other = gates[twin or "plain"]
        assert other[1] != kept, name
        assert len(_inputs_that_differ(c, other[0])) == 1, (name, _inputs_that_differ(c, other[0]))
        a, b = ic.probe(c)[gated], ic.probe(other[0])[gated]
        assert not np.array_equal(a, b, equal_nan=True), name


def test_lower_depth_gate_alone_decides_its_cases(gates):
    """d_negzero, d_negative and d_subnormal_negative are dropped by `d > 0` and by nothing else: the
    restatement without that gate keeps their pixel (pm.z > 0, inside the map, a normal, inside the
    distance gate). No other case changes its own pixel's outcome."""
    for name, (c, kept, _, _) in gates.items():
        t = ic.full_terms(c, d_positive=False)
        s = c["px"][1] * ic.GATE_W + c["px"][0]
        assert bool(t["keep"][s]) == (kept or name in ic.GATES_WITHOUT_D_POSITIVE), name
    assert all(not gates[n][1] for n in ic.GATES_WITHOUT_D_POSITIVE)


def test_equality_cases_stand_on_the_comparison(gates):
    """Where a case claims equality, the gated quantity compares equal in float32 to its bound; its twin
    is the neighbouring float (or the neighbouring integer after rounding)."""
    P = {k: ic.probe(v[0]) for k, v in gates.items()}
    md = gates["d_eq_max"][0]["max_depth"]
    assert P["d_eq_max"]["d"] == f32(md) and P["d_above_max"]["d"] == np.nextafter(f32(md), f32(np.inf))
    assert P["d_negzero"]["d"] == 0 and np.signbit(P["d_negzero"]["d"])
    assert 0 < P["d_subnormal"]["d"] < np.finfo(f32).tiny and np.isnan(P["d_nan"]["d"])
    assert P["d_subnormal_negative"]["d"] == -P["d_subnormal"]["d"] and P["d_negative"]["d"] == -1
    assert 0 < P["d_tiny_positive"]["d"] == f32(2.0 ** -100)
    assert P["pmz_zero"]["pm"][2] == 0 and P["pmz_half"]["pm"][2] == f32(0.5) and P["pmz_negative"]["pm"][2] == -1
    for ax, n_even, n_odd in (("u", 6, 7), ("v", 4, 5)):
        raw, rnd = "f%s_raw" % ax, "f%s" % ax
        for k in ("m_minus_half", "m_minus_0.3"):  # -0: kept at index 0 (roundf would give -1 for -0.5)
            p = P[ax + k]
            assert p[rnd] == 0 and np.signbit(p[rnd]) and p["inside"]
        assert P[ax + "m_minus_half"][raw] == f32(-0.5)
        assert P[ax + "m_below_minus_half"][raw] == np.nextafter(f32(-0.5), f32(-1))
        assert P[ax + "m_below_minus_half"][rnd] == -1
        assert P[ax + "m_eq_size"][raw] == n_even == P[ax + "m_eq_size"][rnd] and not P[ax + "m_eq_size"]["inside"]
        assert P[ax + "m_last"][rnd] == n_even - 1 and P[ax + "m_last"]["inside"]
        assert P[ax + "m_even_tie_out"][raw] == n_even - 0.5 and P[ax + "m_even_tie_out"][rnd] == n_even
        assert P[ax + "m_even_below_tie"][raw] == np.nextafter(f32(n_even - 0.5), f32(0))
        assert P[ax + "m_even_below_tie"][rnd] == n_even - 1
        assert P[ax + "m_odd_tie_in"][raw] == n_odd - 0.5 and P[ax + "m_odd_tie_in"][rnd] == n_odd - 1
        assert P[ax + "m_odd_above_tie"][raw] == np.nextafter(f32(n_odd - 0.5), f32(np.inf))
        assert P[ax + "m_odd_above_tie"][rnd] == n_odd
    assert P["proj_inf"]["fu_raw"] == np.inf and 0 < P["proj_inf"]["pm"][2] < 1e-36 and P["proj_inf"]["pm"][0] == 1000
    assert np.isfinite(P["proj_finite"]["fu_raw"]) and P["proj_finite"]["pm"][2] == P["proj_inf"]["pm"][2]
    assert not P["n_zero"]["n"].any() and np.array_equal(P["n_tiny"]["n"], np.array([0, 0, 2.0 ** -100], f32))
    assert np.isnan(P["point_nan"]["e2"])
    assert P["dist_eq"]["e2"] == P["dist_eq"]["max_dist2"] == f32(0.0625)
    e2 = P["dist_above"]["e2"]  # e.z = succ(0.25): e . e = 0.0625 + 2^-26 (+ 2^-50, rounded away)
    assert e2 == f32(0.0625 + 2.0 ** -26) and e2 > P["dist_above"]["max_dist2"]
    assert P["dist_zero_gate"]["e2"] == 0 == P["dist_zero_gate"]["max_dist2"]
    assert P["dist_zero_gate_off"]["e2"] == f32(2.0 ** -48) and P["dist_zero_gate_off"]["max_dist2"] == 0


def test_onehot_lattice():
    """Every pixel of the one-hot frame is kept by the restatement; odd columns and rows are ties that
    round to even (columns 1, 5, 9, ... down to 0, 2, 4, where roundf would give 1, 3, 5; column 22 lands
    on 11); the depths are 1.0, 2.0 and one that is no power of two; all entries of J and r are distinct
    between pixels and none but one is zero."""
    c = ic.onehot()
    t = ic.full_terms(c)
    assert t["keep"].all() and t["keep"].size == 23 * 17
    um, vm = t["um"].reshape(17, 23), t["vm"].reshape(17, 23)
    assert list(um[0]) == [0, 0, 1, 2, 2, 2, 3, 4, 4, 4, 5, 6, 6, 6, 7, 8, 8, 8, 9, 10, 10, 10, 11]
    assert list(vm[:, 0]) == [0, 0, 1, 2, 2, 2, 3, 4, 4, 4, 5, 6, 6, 6, 7, 8, 8]
    for u in range(1, 23, 2):  # a tie: half to even; half away from zero reads the other neighbour at u % 4 == 1
        assert um[0, u] == round(u / 2) and (um[0, u] != math.floor(u / 2 + 0.5)) == (u % 4 == 1)
    assert set(np.unique(c["depth"])) == {f32(1.0), f32(2.0), f32(1.3)}
    for k in range(6):
        # (pw x n).z is zero at the principal point (11, 8) alone
        assert np.unique(t["J"][:, k]).size >= 12 * 9 and (t["J"][:, k] != 0).sum() >= 23 * 17 - (k == 2)
    assert np.unique(t["r"]).size == 23 * 17 and (t["r"] != 0).all()
    for stride, n, last in ((3, 8 * 6, 21), (5, 5 * 4, 20), (64, 1, 0)):
        ts = ic.full_terms(c, stride)
        assert ts["keep"].all() and ts["keep"].size == n and ts["u"].max() == last < 23


@pytest.fixture(scope="module")
def tree_small():
    c = ic.tree_case(256, 3)
    return c, ic.full_terms(c)


def test_tree_equals_scalar_walk(tree_small):
    """ref.icp_tree (vectorised) is bit-equal to a scalar pure-Python walk of the documented tree on a
    3-workgroup input, and on its first 700 samples (a last workgroup with 188 live lanes)."""
    c, t = tree_small
    for n in (768, 700):
        J, r, keep = t["J"][:n], t["r"][:n], t["keep"][:n]
        a = ref.icp_tree(J, r, keep, n)
        b = ic.tree_scalar(ref.icp_lane_terms(J, r, keep), n)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert a[28] == keep.sum()


@pytest.mark.parametrize("shape", [(256, 1, 1), (256, 33, 1), (256, 225, 1), (250, 130, 1), (511, 97, 2)])
def test_tree_within_the_bound_of_fsum(shape):
    """icp_tree is within count * 2^-53 * sum |term| of math.fsum of the exact terms, the bound the GPU
    tests use; the case gates about a tenth of its pixels, by every gate it names, and its terms have
    both signs and span six decades."""
    W, H, stride = shape
    c = ic.tree_case(W, H, stride)
    t = ic.full_terms(c, stride)
    keep = t["keep"]
    got = ref.icp_tree(t["J"], t["r"], keep, keep.size)
    want, mag = ref.icp_sums_exact(t["J"][keep], t["r"][keep])
    assert got[28] == want[28] == keep.sum()
    assert (np.abs(got[:28] - want[:28]) <= want[28] * 2.0 ** -53 * mag[:28]).all()
    if W * H > 1000:
        assert 0.06 < 1 - keep.mean() < 0.14
        d = c["depth"][::stride, ::stride].reshape(-1)
        assert (d == 0).sum() > 5 and np.isnan(d).sum() > 5
        assert (~c["model"]["normal"].any(-1)).sum() > 5
        terms = ref.icp_lane_terms(t["J"], t["r"], keep)[keep, :27]
        assert (terms > 0).any() and (terms < 0).any()
        a = np.abs(terms[:, 20])  # n.z^2
        assert np.percentile(a, 99) / np.percentile(a, 1) > 1e5


def test_tree_depends_on_the_order():
    """The order of addition shows in the last bits of this data: the documented tree and a plain
    left-to-right sum of the same terms differ in some sum."""
    c = ic.tree_case(256, 33)
    t = ic.full_terms(c)
    terms = ref.icp_lane_terms(t["J"], t["r"], t["keep"])
    seq = np.zeros(29)
    for row in terms:
        seq = seq + row
    assert not np.array_equal(ref.icp_tree(t["J"], t["r"], t["keep"], t["keep"].size), seq)


def test_normals_case_shows_both_outcomes_of_every_rule():
    """On the restatement: the angle rule alone drops at least 20 interior pixels and keeps at least 20,
    the nearest cosine on each side is within 0.01 of 0.3, and border, hole, nn == 0, nn not finite and
    the flip each decide at least 3 pixels; the restated census agrees with ref.point_map_normals."""
    model, K, pose = ic.normals_case()
    assert model["point"].shape == (21, 37, 3)
    r = ic.normals_rules(model, K, pose)
    out = ref.point_map_normals(model, K, pose)["normal"]
    assert np.array_equal((out != 0).any(-1), r["kept"]) and not np.isnan(out).any()
    assert r["angle_drop"].sum() >= 20 and r["kept"].sum() >= 20
    lo, hi = np.nanmax(np.where(r["angle_drop"], r["cos"], np.nan)), np.nanmin(np.where(r["kept"], r["cos"], np.nan))
    print(f"angle rule: {r['angle_drop'].sum()} dropped, {r['kept'].sum()} kept, cosines {lo:.4f} / {hi:.4f}")
    assert 0.29 <= lo < 0.3 <= hi <= 0.31
    for k in ("border", "hole", "nn_zero", "nn_not_finite", "flip"):
        assert r[k].sum() >= 3, k
    assert (r["kept"] & ~r["flip"]).sum() >= 3
    assert np.isnan(model["point"]).any() and np.abs(np.nan_to_num(model["point"])).max() == f32(1e19)
    total = sum(r[k].astype(int) for k in ("border", "hole", "nn_zero", "nn_not_finite", "angle_drop", "kept"))
    assert (total == 1).all()


def test_track_early_stop_rule():
    """ref.track's early stop is the engine's: only when either eps is positive, and then both norms
    must be within their eps (shown on a stub engine whose model is a plane)."""
    W, H, K = 24, 18, (20.0, 20.0, 12.0, 9.0)
    F = ref.Camera(K, ic.se3())
    v, u = np.mgrid[0:H, 0:W]
    ray = F.pixel_ray(u.reshape(-1), v.reshape(-1))
    # three planes meeting in a corner, so that all six degrees of freedom are held
    z = np.where(u < 12, 2.0 + 0.05 * (12 - u), 2.0 + 0.04 * (u - 12)) + np.where(v < 9, 0.06 * (9 - v), 0.0)
    d = z.astype(f32).reshape(-1)
    point = np.stack([ray[0] * d, ray[1] * d, d], -1).reshape(H, W, 3)
    normal = np.zeros_like(point)
    normal[..., 2] = -1

    class Stub:
        def raycast_surface(self, K, W, H, pose, max_depth, maps=()):
            return dict(point=point, normal=normal)

    guess = ic.se3()
    depth = (z + 0.004).astype(f32)
    kw = dict(levels=2, stride=(2, 1), iterations=(4, 6))
    n0 = []
    base = ref.track(Stub(), depth, K, guess, norms=n0, **kw)
    assert base[1] == 0 and base[2] == 10 and len(n0) == 10 and [l for l, _, _ in n0] == [0] * 4 + [1] * 6
    assert all(w > 0 and t > 0 for _, w, t in n0)
    big = ref.track(Stub(), depth, K, guess, eps_rot=1e9, eps_trans=1e9, **kw)
    assert big[1] == 0 and big[2] == 2  # one iteration per level
    for one in (dict(eps_rot=1e9), dict(eps_trans=1e9)):  # && : the other norm is never <= 0
        got = ref.track(Stub(), depth, K, guess, **one, **kw)
        assert got[2] == 10 and np.array_equal(got[0].q, base[0].q) and np.array_equal(got[0].t, base[0].t)
