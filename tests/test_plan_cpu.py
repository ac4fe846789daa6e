"""The host side of lamp-stop planning, no GPU: the numpy restatement of tsdf_uv_plan (tests/_plan_ref.py) on
hand-made matrices, the helpers of tsdf_amd.uv / tsdf_amd.esdf against direct computations, the binding's
declarations, and host/uv_dose.h's twins through the stand-alone plan_host_main."""
import os
import subprocess

import numpy as np
import pytest

import _plan_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "plan_host_main")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_plan_disjoint_coverage_in_gain_order():
    # three candidates over disjoint receivers; gains 2 * 5 = 10, 3 * 4 = 12, 1 * 3 = 3
    E = np.array([[5, 5, 0, 0, 0, 0], [0, 0, 4, 4, 4, 0], [0, 0, 0, 0, 0, 3]], f32)
    need = np.array([5, 5, 4, 4, 4, 3], f32)
    r = _plan_ref.plan(E, need, max_stops=5)
    assert r["stops"].tolist() == [1, 0, 2]
    assert r["gains"].tolist() == [12.0, 10.0, 3.0]
    assert r["need"].tolist() == [0] * 6
    # a weight turns the order round
    r = _plan_ref.plan(E, need, weight=np.array([1, 1, 0.5, 0.5, 0.5, 8], f32), max_stops=5)
    assert r["stops"].tolist() == [2, 0, 1] and r["gains"].tolist() == [24.0, 10.0, 6.0]


def test_plan_repeats_a_pick_while_need_remains():
    E = np.array([[4, 4], [1, 0]], f32)
    r = _plan_ref.plan(E, np.array([10, 6], f32), max_stops=8)
    # candidate 0 removes 8, 6 (4 + 2), then 2 (2 + 0); then candidate 1 has nothing left either
    assert r["stops"].tolist() == [0, 0, 0]
    assert r["gains"].tolist() == [8.0, 6.0, 2.0]
    assert r["need"].tolist() == [0, 0]


def test_plan_stops_by_min_gain_and_by_max_stops():
    E = np.array([[4, 4], [1, 0]], f32)
    need = np.array([10, 6], f32)
    r = _plan_ref.plan(E, need, max_stops=8, min_gain=5.0)
    assert r["stops"].tolist() == [0, 0] and r["need"].tolist() == [2, 0]
    r = _plan_ref.plan(E, need, max_stops=1)
    assert r["stops"].tolist() == [0] and r["need"].tolist() == [6, 2]
    r = _plan_ref.plan(E, need, max_stops=8, min_gain=9.0)
    assert r["stops"].size == 0 and r["need"].tolist() == [10, 6]
    assert _plan_ref.plan(E, need, max_stops=0)["stops"].size == 0


def test_plan_all_zero_matrix_and_ties_and_nan():
    r = _plan_ref.plan(np.zeros((3, 5), f32), np.ones(5, f32), max_stops=4)
    assert r["stops"].size == 0 and r["gains"].size == 0 and r["need"].tolist() == [1] * 5
    # two identical rows: the lower index
    E = np.array([[0, 1, 0], [2, 2, 0], [2, 2, 0]], f32)
    assert _plan_ref.plan(E, np.full(3, 2, f32), max_stops=1)["stops"].tolist() == [1]
    # a NaN in E or in need contributes nothing, and a negative entry neither
    E = np.array([[np.nan, 1, 1], [3, -5, 0]], f32)
    r = _plan_ref.plan(E, np.array([4, 4, np.nan], f32), max_stops=1)
    assert r["stops"].tolist() == [1] and r["gains"].tolist() == [3.0]
    assert r["need"][:2].tolist() == [1, 4] and np.isnan(r["need"][2])


def test_tube_candidates():
    from tsdf_amd import uv
    centres = np.array([[0.5, -1.0, 0.25], [0.0, 0.0, 1.0], [-2.0, 0.125, 0.75]], f32)
    em, first = uv.tube_candidates(centres, (0.0, 3.0, 4.0), 1.5, 36.0, 2.5, 4)
    want, wfirst = _plan_ref.tube_candidates(centres, (0.0, 3.0, 4.0), 1.5, 36.0, 2.5, 4)
    assert em.dtype == f32 and em.shape == (12, 4) and first.dtype == np.int32
    assert first.tolist() == [0, 4, 8, 12] and np.array_equal(first, wfirst)
    assert np.array_equal(bits(em), bits(want))
    # candidate c is tube_emitters of its two ends, and its energies sum to power * dwell
    h = np.array([0.0, 0.6, 0.8]) * 0.75
    for c in range(3):
        p = centres[c].astype(np.float64)
        assert np.array_equal(em[4 * c:4 * c + 4], uv.tube_emitters(p - h, p + h, 36.0, 2.5, 4))
        assert abs(float(em[4 * c:4 * c + 4, 3].astype(np.float64).sum()) - 90.0) <= 1e-5
    e0, f0 = uv.tube_candidates(np.zeros((0, 3)), (1, 0, 0), 1.0, 1.0, 1.0, 2)
    assert e0.shape == (0, 4) and f0.tolist() == [0]
    with pytest.raises(ValueError):
        uv.tube_candidates(centres, (0, 0, 0), 1.0, 1.0, 1.0, 2)
    with pytest.raises(ValueError):
        uv.tube_candidates(centres, (1, 0, 0), 1.0, 1.0, 1.0, 0)


def test_plan_need():
    from tsdf_amd import uv
    dose = np.array([12.0, 3.0, 10.0, 50.0, 0.0, 9.999], f32)
    prob = np.array([0.9, 0.6, 0.5, 0.2, 0.8, 0.49], f32)
    got = uv.plan_need(dose, prob, 10.0)
    assert got.dtype == f32 and np.array_equal(bits(got), bits(_plan_ref.plan_need(dose, prob, 10.0)))
    assert got.tolist() == [0.0, 7.0, 0.0, 0.0, 10.0, 0.0]
    assert uv.plan_need(dose, prob, 10.0, prob_min=0.85).tolist() == [0.0] * 6
    rng = np.random.default_rng(2)
    dose, prob = (rng.random(200) * 20).astype(f32), rng.random(200).astype(f32)
    assert np.array_equal(bits(uv.plan_need(dose, prob, 7.3, 0.3)), bits(_plan_ref.plan_need(dose, prob, 7.3, 0.3)))
    with pytest.raises(ValueError):
        uv.plan_need(dose, prob[:3], 1.0)


def _random_mesh(rng, n, m):
    return rng.standard_normal((n, 3)).astype(f32), rng.integers(0, n, (m, 3)).astype(np.int32)


def test_vertex_area():
    from tsdf_amd import uv
    # a unit square of two triangles: corners 0 and 2 touch both (1/3), corners 1 and 3 one (1/6)
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 5]], f32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    a = uv.vertex_area(pos, idx)
    assert a.dtype == f32 and np.allclose(a, [1 / 3, 1 / 6, 1 / 3, 1 / 6, 0.0], atol=1e-7)
    pos, idx = _random_mesh(np.random.default_rng(8), 40, 90)
    got = uv.vertex_area(pos, idx)
    assert np.array_equal(bits(got), bits(_plan_ref.vertex_area(pos, idx)))
    # the areas add up to the mesh's
    p = pos.astype(np.float64)
    total = np.linalg.norm(np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]]), axis=1).sum() / 2
    assert abs(float(got.astype(np.float64).sum()) - total) <= 1e-5 * total
    assert uv.vertex_area(pos, np.zeros((0, 3), np.int32)).tolist() == [0.0] * 40


def _field(rng, dims, origin, unknown=False):
    nx, ny, nz = dims
    return dict(d2=rng.integers(0, 400, (nz, ny, nx)).astype(np.uint16),
                state=rng.integers(0, 3, (nz, ny, nx)).astype(np.uint8), origin=origin, dims=dims, max_dist=20,
                unknown=unknown)


def test_standoff_candidates_brute_force():
    from tsdf_amd import esdf
    rng = np.random.default_rng(4)
    for dims, origin, stride in (((7, 5, 6), (-3, 10, -20), 1), ((7, 5, 6), (-3, 10, -20), 2), ((10, 7, 8), (0, 0, 0), 3)):
        field = _field(rng, dims, origin)
        got = esdf.standoff_candidates(field, 0.02, 0.1, 0.3, stride)
        want = _plan_ref.standoff_candidates(field, 0.02, 0.1, 0.3, stride)
        assert got.dtype == f32 and got.shape == want.shape and want.shape[0] > 0
        assert np.array_equal(bits(got), bits(want))
    # with unknown sites the unobserved voxels hold distance 0: nothing stands in them or at them
    field = _field(rng, (6, 6, 6), (0, 0, 0), unknown=True)
    field["d2"][field["state"] == 0] = 0
    got = esdf.standoff_candidates(field, 0.02, 0.02, 1.0, 1)
    st = field["state"][np.rint(got[:, 2] / 0.02).astype(int), np.rint(got[:, 1] / 0.02).astype(int),
                        np.rint(got[:, 0] / 0.02).astype(int)]
    assert got.shape[0] > 0 and np.all(st == 1)
    assert np.array_equal(bits(got), bits(_plan_ref.standoff_candidates(field, 0.02, 0.02, 1.0, 1)))
    no_state = dict(field, state=None)
    with pytest.raises(ValueError):
        esdf.standoff_candidates(no_state, 0.02, 0.0, 1.0, 1)
    with pytest.raises(ValueError):
        esdf.standoff_candidates(field, 0.02, 0.0, 1.0, 0)


def test_binding_declares_plan():
    import ctypes as C
    import tsdf_amd
    from tsdf_amd import _lib
    L = tsdf_amd.load_library()
    for name in ("tsdf_uv_irradiance", "tsdf_uv_plan_config_default", "tsdf_uv_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert C.sizeof(_lib.UvPlanConfig) == 8
    assert callable(tsdf_amd.Engine.uv_irradiance) and callable(tsdf_amd.Engine.uv_plan)
    c = _lib.UvPlanConfig()
    L.tsdf_uv_plan_config_default(C.byref(c))
    assert (c.max_stops, c.min_gain) == (16, 0.0)
    # invalid arguments are refused before any device work
    assert L.tsdf_uv_irradiance(None, None, None, 0, None, None, 0, None, None, 0) == 1
    num = C.c_int32(7)
    assert L.tsdf_uv_plan(None, None, 0, 0, None, None, None, None, None, C.byref(num), 0) == 1


def _run(lines):
    r = subprocess.run([BIN], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [ln.split() for ln in out]


def host_lines():
    """The commands test_host_header_matches_numpy sends to plan_host_main, with what numpy answers."""
    from tsdf_amd import esdf, uv
    rng = np.random.default_rng(6)
    num = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))
    ints = lambda a: " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))
    centres = rng.standard_normal((5, 3)).astype(f32)
    axis = np.array([0.25, -1.5, 0.75], f32)
    dose, prob = (rng.random(50) * 20).astype(f32), rng.random(50).astype(f32)
    pos, idx = _random_mesh(rng, 30, 70)
    field = _field(rng, (7, 5, 6), (-3, 10, -20))
    voxel, lo, hi = f32(0.02), f32(0.1), f32(0.3)
    lines = [
        f"candidates 5 {num(centres)} {num(axis)} 1.5 36.0 2.5 4",
        f"need 50 7.25 0.375 {num(dose)} {num(prob)}",
        f"area 30 70 {num(pos)} {ints(idx)}",
        f"standoff 7 5 6 -3 10 -20 {float(voxel)!r} {float(lo)!r} {float(hi)!r} 2 {ints(field['d2'])} {ints(field['state'])}",
        f"candidates 1 0 0 0 0 0 0 1.0 1.0 1.0 2",
        "area 1 1 0 0 0 0 1 2",
    ]
    want = [uv.tube_candidates(centres, axis, 1.5, 36.0, 2.5, 4), uv.plan_need(dose, prob, 7.25, 0.375),
            uv.vertex_area(pos, idx), esdf.standoff_candidates(field, voxel, lo, hi, 2)]
    return lines, want


def test_host_header_matches_numpy():
    """host/uv_dose.h (C++) against tsdf_amd.uv / tsdf_amd.esdf on the same inputs."""
    lines, (cand, need, area, stand) = host_lines()
    got_c, got_n, got_a, got_s, bad_axis, bad_index = _run(lines)
    k = got_c.index("first")
    assert np.array_equal(bits(np.array([float(v) for v in got_c[:k]], f32).reshape(-1, 4)), bits(cand[0]))
    assert [int(v) for v in got_c[k + 1:]] == cand[1].tolist()
    assert np.array_equal(bits(np.array([float(v) for v in got_n], f32)), bits(need))
    assert np.array_equal(bits(np.array([float(v) for v in got_a], f32)), bits(area))
    assert stand.shape[0] > 0
    assert np.array_equal(bits(np.array([float(v) for v in got_s], f32).reshape(-1, 3)), bits(stand))
    assert bad_axis[0] == "error" and bad_index[0] == "error"
