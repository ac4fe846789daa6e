"""Lamp-stop planning on the GPU (tsdf_uv_irradiance / tsdf_uv_plan): the irradiance rows against tests/
_uv_ref.py and against Engine.uv_dose, bit for bit; the plan against tests/_plan_ref.py; both on the scene;
and through the facade. The volume, its receivers and the emitters A, FAR, BELOW are tests/
test_gpu_uv_dose.py's (its docstring describes them): 64 x 64 x 48 voxels of 1 cm, 3600 floor receivers."""
import os
import subprocess

import numpy as np
import pytest

import _plan_ref
import _uv_ref
import test_gpu_uv_dose as S

pytestmark = pytest.mark.gpu

scene = S.scene  # (the module's fixture, here as this module's)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "plan_main")
VOXEL = S.VOXEL
f32 = np.float32
same = S.same
X = np.array([[-0.22, 0.0, 0.24, 10.0], [0.2, 0.15, 0.3, 4.0]], f32)  # (test_accumulation_and_edges's)
FAR25 = np.array([[-0.5, 0.3, 25.0, 1000.0]], f32)                    # (test_grid_fallback's)
ALT = dict(bias=0.035, step=0.007, min_weight=10)                      # (the scene's weights are 10)


def batch():
    """The six candidates: A lit; FAR out of range; BELOW under the floor; an empty one; the two-emitter X; a
    3-segment tube across the box, 15 cm up."""
    from tsdf_amd import uv
    tube = uv.tube_emitters((-0.2, 0.0, 0.15), (0.2, 0.0, 0.15), 30.0, 1.0, 3)
    cands = [S.A, S.FAR, S.BELOW, np.zeros((0, 4), f32), X, tube]
    first = np.cumsum([0] + [c.shape[0] for c in cands]).astype(np.int32)
    return cands, np.concatenate(cands), first


@pytest.fixture(scope="module")
def refs(scene):
    """The restatement's rows, computed once: all receivers with the defaults; the 37-receiver subset (three
    normals zeroed) with the defaults and with ALT; every seventh receiver with max_range 30 for the batch
    plus the emitter at 25 m."""
    dump, pts, nrm = scene["dump"], scene["pts"], scene["nrm"]
    cands, _, _ = batch()
    sub = slice(2292, 2329)  # x = 8.25 voxels, y = -17.75 .. 18.25: a row across the box's shadow
    nz = nrm[sub].copy()
    nz[[3, 17, 36]] = 0
    full = [_uv_ref.dose(dump, pts, nrm, c, VOXEL) for c in cands]
    r = dict(sub=sub, nz=nz, full=np.stack([f[0] for f in full]), tube=full[5],
             small=np.stack([_uv_ref.dose(dump, pts[sub], nz, c, VOXEL)[0] for c in cands]),
             alt=np.stack([_uv_ref.dose(dump, pts[sub], nz, c, VOXEL, **ALT)[0] for c in cands]),
             far=np.stack([_uv_ref.dose(dump, pts[::7], nrm[::7], c, VOXEL, max_range=30.0)[0]
                           for c in cands + [FAR25]]))
    return r


def rows_by_dose(eng, pts, nrm, cands, **cfg):
    """The path the batched call replaces: one uv_dose per candidate into zeros."""
    return np.stack([eng.uv_dose(pts, nrm, c, **cfg) for c in cands])


def test_irradiance_rows_bit_for_bit(scene, refs):
    import torch
    eng, pts, nrm = scene["eng"], scene["pts"], scene["nrm"]
    cands, em, first = batch()
    assert first.tolist() == [0, 1, 2, 3, 3, 5, 8] and pts.shape[0] == 3600  # 14 workgroups and 16 lanes
    want = refs["full"]
    assert same(want[0], scene["refA"]) and np.count_nonzero(want[0]) > 2000
    assert not want[1].any() and not want[2].any() and not want[3].any()
    _, counted, visible = refs["tube"]
    assert (counted & ~visible).any() and visible.any()  # the tube: partly shadowed
    got = eng.uv_irradiance(pts, nrm, em, first)
    assert got.shape == (6, 3600) and got.dtype == f32
    for c in range(6):
        assert same(got[c], want[c]), c
    assert same(got, rows_by_dose(eng, pts, nrm, cands))
    assert same(eng.uv_irradiance(pts, nrm, em, first, use_grid=0), want)
    dp, dn = torch.as_tensor(pts, device="cuda"), torch.as_tensor(nrm, device="cuda")
    for g in (1, 0):
        dev = eng.uv_irradiance(dp, dn, em, first, device=True, use_grid=g)
        assert dev.is_cuda and tuple(dev.shape) == (6, 3600) and same(dev.cpu().numpy(), want)
    # the rows do not depend on the other candidates of the batch
    assert same(eng.uv_irradiance(pts, nrm, cands[5], [0, 3]), want[5:6])
    assert same(eng.uv_irradiance(pts, nrm, np.concatenate([cands[5], cands[0]]), [0, 0, 3, 4]),
                np.stack([want[3], want[5], want[0]]))
    # less than a wave, three receivers without a normal
    sub, nz = refs["sub"], refs["nz"]
    small = eng.uv_irradiance(pts[sub], nz, em, first)
    assert small.shape == (6, 37) and same(small, refs["small"])
    print("subset: lit by A", int((small[0] > 0).sum()), "of 37")
    assert not small[:, [3, 17, 36]].any() and (small[0] > 0).any()
    assert same(small, rows_by_dose(eng, pts[sub], nz, cands))
    assert same(eng.uv_irradiance(pts[sub], nz, em, first, use_grid=0), refs["small"])
    # another bias, step and min_weight
    alt = eng.uv_irradiance(pts[sub], nz, em, first, **ALT)
    assert same(alt, refs["alt"])
    assert same(alt, rows_by_dose(eng, pts[sub], nz, cands, **ALT))
    assert eng.stats()["status"] == 0


def test_irradiance_batch_wide_fallback(scene, refs):
    """One emitter at 25 m makes the rays' cube too wide for a block grid: every candidate of the batch takes
    hash lookups, and every row is still the contract's."""
    eng = scene["eng"]
    pts, nrm = scene["pts"][::7], scene["nrm"][::7]
    cands, _, _ = batch()
    cands = cands + [FAR25]
    first = np.cumsum([0] + [c.shape[0] for c in cands]).astype(np.int32)
    want = refs["far"]
    assert want[6].any() and want[1].any()  # (FAR is in range now)
    got = eng.uv_irradiance(pts, nrm, np.concatenate(cands), first, max_range=30.0)
    for c in range(7):
        assert same(got[c], want[c]), c
    assert same(got, rows_by_dose(eng, pts, nrm, cands, max_range=30.0))


SHAPES = [(1, 1), (3, 255), (70, 257), (70, 3600), (130, 1025), (300, 129)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plan_matches_restatement(scene, shape):
    import torch
    eng = scene["eng"]
    C, n = shape
    E, need, weight = _plan_ref.synthetic(C, n, seed=1000 + C + n)
    ref = _plan_ref.plan(E, need, weight, max_stops=12)
    assert ref["stops"].size > 0
    # no pick of the restatement hinges on rounding: best and second best differ by more than twice the bound
    least = np.inf
    for G, bound in ref["rounds"]:
        order = np.argsort(-G, kind="stable")
        if C > 1 and G[order[0]] > 0:
            b = max(bound[order[0]], bound[order[1]])
            assert G[order[0]] - G[order[1]] > 2 * b
            least = min(least, (G[order[0]] - G[order[1]]) / b)
    print(f"plan {C}x{n}: {ref['stops'].size} stops, least margin / bound {least:.3g}")
    got = eng.uv_plan(E, need, weight, max_stops=12)
    assert got["stops"].dtype == np.int32 and got["gains"].dtype == np.float64 and got["need"].dtype == f32
    assert got["stops"].tolist() == ref["stops"].tolist()
    assert same(got["need"], ref["need"])
    worst = 0.0
    for r, c in enumerate(ref["stops"]):
        bound = ref["rounds"][r][1][c]
        err = abs(got["gains"][r] - ref["gains"][r])
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
        assert err <= bound, (r, c, got["gains"][r], ref["gains"][r], bound)
    print(f"plan {C}x{n}: largest gain error / bound {worst:.3g}")
    assert same(need, _plan_ref.synthetic(C, n, seed=1000 + C + n)[1])  # the caller's need is not written
    # the same bits from a second call and from device arrays
    again = eng.uv_plan(E, need, weight, max_stops=12)
    assert np.array_equal(again["gains"].view(np.uint64), got["gains"].view(np.uint64))
    assert again["stops"].tolist() == got["stops"].tolist() and same(again["need"], got["need"])
    dn = torch.as_tensor(need, device="cuda")
    dev = eng.uv_plan(torch.as_tensor(E, device="cuda"), dn, torch.as_tensor(weight, device="cuda"), max_stops=12,
                      device=True)
    assert dev["need"].is_cuda and same(dev["need"].cpu().numpy(), got["need"]) and same(dn.cpu().numpy(), need)
    assert np.array_equal(dev["gains"].view(np.uint64), got["gains"].view(np.uint64))
    assert dev["stops"].tolist() == got["stops"].tolist()


def test_plan_ties_nan_and_limits(scene):
    eng = scene["eng"]
    rng = np.random.default_rng(77)
    E = (rng.random((5, 700)) * 3).astype(f32)
    need = (rng.random(700) * 8 + 1).astype(f32)
    E[3] = E[1] = (rng.random(700) * 10 + 5).astype(f32)  # two identical rows that beat the rest
    got = eng.uv_plan(E, need, max_stops=1)
    assert got["stops"].tolist() == [1] and got["stops"].tolist() == _plan_ref.plan(E, need, max_stops=1)["stops"].tolist()
    # weight None is all 1
    assert np.array_equal(eng.uv_plan(E, need, np.ones(700, f32), max_stops=3)["gains"].view(np.uint64),
                          eng.uv_plan(E, need, max_stops=3)["gains"].view(np.uint64))
    # one NaN in E and one in need are ignored
    E, need, weight = _plan_ref.synthetic(9, 500, seed=5)
    E[3, 10], need[20] = np.nan, np.nan
    E[:, 20] = np.abs(E[:, 20]) + 1  # (every row irradiates the receiver whose need is a NaN)
    ref = _plan_ref.plan(E, need, weight, max_stops=6)
    got = eng.uv_plan(E, need, weight, max_stops=6)
    assert got["stops"].tolist() == ref["stops"].tolist() and len(ref["stops"]) == 6
    assert same(got["need"], ref["need"]) and np.isfinite(got["gains"]).all()
    assert np.abs(got["gains"] - ref["gains"]).max() <= max(ref["rounds"][r][1][c] for r, c in enumerate(ref["stops"]))
    # min_gain above the first gain: no stop, need untouched; max_stops 0 likewise
    first = float(ref["gains"][0])
    for kw in (dict(min_gain=first * 1.5), dict(max_stops=0)):
        none = eng.uv_plan(E, need, weight, **kw)
        assert none["stops"].size == 0 and none["gains"].size == 0 and same(none["need"], need)
    keep = eng.uv_plan(E, need, weight, max_stops=6, min_gain=float(ref["gains"][2]) * 0.999)
    assert keep["stops"].tolist() == ref["stops"][:3].tolist()
    # an all-zero matrix, no candidates, no receivers
    assert eng.uv_plan(np.zeros((4, 300), f32), need[:300], max_stops=5)["stops"].size == 0
    assert eng.uv_plan(np.zeros((0, 300), f32), need[:300])["stops"].size == 0
    assert eng.uv_plan(np.zeros((3, 0), f32), need[:0])["need"].shape == (0,)


@pytest.fixture(scope="module")
def candidates(scene):
    """Tubes of 3 segments, 10 cm along x, at the free voxels 2 to 4 cm from the surface on a lattice of 8
    voxels (z = -5: 3 voxels over the floor; z = 11: over the box's top)."""
    from tsdf_amd import esdf, uv
    field = scene["eng"].distance_field((-32, -32, -13), (64, 64, 40), max_dist=40)
    centres = esdf.standoff_candidates(field, VOXEL, 0.02, 0.04, 8)
    em, first = uv.tube_candidates(centres, (1.0, 0.0, 0.0), 0.1, 30.0, 1.0, 3)
    return centres, em, first


def test_plan_on_the_scene(scene, candidates):
    from tsdf_amd import uv
    eng, pts, nrm = scene["eng"], scene["pts"], scene["nrm"]
    centres, em, first = candidates
    C = centres.shape[0]
    print("scene: candidates", C, "over the floor", int((centres[:, 2] < 0).sum()))
    assert 30 <= C <= 200 and (centres[:, 2] < 0).sum() >= 30
    E = eng.uv_irradiance(pts, nrm, em, first)
    target = 20.0
    prob = (pts[:, 0] > 0).astype(f32)  # the half of the floor that wants its dose
    need0 = uv.plan_need(np.zeros(3600, f32), prob, target)
    assert np.count_nonzero(need0) == 1800
    plan = eng.uv_plan(E, need0, max_stops=6)
    stops = plan["stops"]
    print("scene: stops", stops.tolist(), "gains", plan["gains"].tolist())
    assert stops.size == 6 and centres[stops[0], 0] > 0
    ref = _plan_ref.plan(E, need0, max_stops=6)
    assert stops.tolist() == ref["stops"].tolist() and same(plan["need"], ref["need"])
    # The stops' emitters applied in order by uv_dose. Stop k adds the row E[s_k] to the dose, so the dose is
    # the fp32 sum of the K rows in order and max(need0 - dose, 0) one more subtraction, where the plan took K
    # subtractions clamped at 0. With e >= 0 both are max(need0 - S, 0), S the exact sum of the rows, in real
    # arithmetic, and clamping and subtracting pass an error on without enlarging it. The plan's K roundings
    # are each at most u times a value in [0, need0]; the dose's K - 1 additions each at most u times a partial
    # sum <= S, and the last subtraction at most u max(need0, S): together at most
    # u (K need0 + (K - 1) S + max(need0, S)) <= u (K + 1) (need0 + S), u = 2^-24; gamma = k u / (1 - k u)
    # with k = K + 1 covers the second-order terms.
    dose = np.zeros(3600, f32)
    cov = [uv.coverage(dose, prob, target)]
    for s in stops:
        eng.uv_dose(pts, nrm, em[first[s]:first[s + 1]], dose=dose)
        cov.append(uv.coverage(dose, prob, target))
    K = stops.size
    Ssum = E[stops].astype(np.float64).sum(axis=0)
    k = (K + 1) * 2.0 ** -24
    tol = k / (1 - k) * (need0.astype(np.float64) + Ssum)
    left = np.maximum(need0 - dose, f32(0))
    err = np.abs(left.astype(np.float64) - plan["need"].astype(np.float64))
    print("scene: coverage", cov, "largest |need - (need0 - dose)| / bound", (err / np.maximum(tol, 1e-300)).max())
    assert np.all(err <= tol)
    assert all(b >= a for a, b in zip(cov, cov[1:])) and cov[-1] > cov[0]
    assert not plan["need"][prob == 0].any()


def test_refusals(scene):
    import tsdf_amd
    lib = tsdf_amd._lib
    eng, pts, nrm = scene["eng"], scene["pts"][:100], scene["nrm"][:100]
    _, em, first = batch()
    bad_first = [np.array([1, 1, 2, 3, 3, 5, 8], np.int32), np.array([0, 1, 2, 3, 3, 2, 8], np.int32), np.append(first[:-1], 7).astype(np.int32),
                 np.append(first[:-1], 9).astype(np.int32)]
    for bad in bad_first:
        with pytest.raises(lib.TSDFError, match="invalid argument"):
            eng.uv_irradiance(pts, nrm, em, bad)
    for bad in (dict(step=0.0), dict(step=-0.01), dict(min_range=0.0), dict(max_range=5.0, step=5.0 / 65537)):
        with pytest.raises(lib.TSDFError, match="invalid argument"):
            eng.uv_irradiance(pts, nrm, em, first, **bad)
    with pytest.raises(lib.TSDFError, match="invalid argument"):
        eng.uv_plan(np.zeros((2, 3), f32), np.zeros(3, f32), max_stops=-1)
    # no candidates, no receivers
    assert eng.uv_irradiance(pts, nrm, np.zeros((0, 4), f32), [0]).shape == (0, 100)
    assert eng.uv_irradiance(pts[:0], nrm[:0], em, first).shape == (6, 0)
    # a shard engine: no irradiance; the plan does not touch the volume and runs
    shard = tsdf_amd.Engine(VOXEL, S.TRUNC, max_width=64, max_height=64, num_block_bits=S.NB_BITS, shard_index=0,
                            shard_count=2)
    try:
        with pytest.raises(lib.TSDFError, match="shard engine"):
            shard.uv_irradiance(pts, nrm, em, first)
        E, need, weight = _plan_ref.synthetic(6, 300, seed=9)
        ref = _plan_ref.plan(E, need, weight, max_stops=4)
        got = shard.uv_plan(E, need, weight, max_stops=4)
        assert got["stops"].tolist() == ref["stops"].tolist() and same(got["need"], ref["need"])
    finally:
        shard.close()
    assert eng.stats()["status"] == 0


def test_facade(scene, candidates, tmp_path):
    """DISINFSystem::query_mesh + plan_irradiation (plan_main) on the same records: Python's stops, gains and
    need for the mesh's high-touch vertices (the box: prob 0.9)."""
    from tsdf_amd import uv
    eng = scene["eng"]
    _, em, first = candidates
    target, max_stops = 15.0, 5
    (tmp_path / "meta.txt").write_text(f"{VOXEL} {S.TRUNC} {S.NB_BITS} {target} {max_stops}\n")
    scene["recs"].tofile(tmp_path / "blocks.bin")
    em.tofile(tmp_path / "emitters.bin")
    first.tofile(tmp_path / "first.bin")
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = eng.extract_mesh_indexed()
    pos, prob = m["positions"], m["prob"]
    n = pos.shape[0]
    assert int((tmp_path / "out_counts.txt").read_text()) == n
    nrm = eng.surface_normals(pos, 0.5)
    E = eng.uv_irradiance(pos, nrm, em, first, sample_offset=0.5)
    need = uv.plan_need(np.zeros(n, f32), prob, target)
    weight = (uv.vertex_area(pos, m["indices"]) * prob).astype(f32)
    assert np.count_nonzero(need) > 100
    plan = eng.uv_plan(E, need, weight, max_stops=max_stops)
    assert plan["stops"].size > 0
    assert np.fromfile(tmp_path / "out_stops.bin", np.int32).tolist() == plan["stops"].tolist()
    assert np.array_equal(np.fromfile(tmp_path / "out_gains.bin", np.uint64), plan["gains"].view(np.uint64))
    assert same(np.fromfile(tmp_path / "out_need.bin", f32), plan["need"])
