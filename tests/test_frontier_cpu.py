"""Frontiers and components without a GPU: the restatement's two labellings against each other, the figures
tests/test_gpu_frontier.py relies on, the binding's declarations and the host helper against esdf."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _edt_ref
import _frontier_ref as fr
import _travel_ref as tr
from tsdf_amd import esdf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "frontier_host_main")
SHAPES = [(7, 9, 12), (1, 1, 1), (5, 1, 8), (1, 9, 1), (9, 17, 20), (16, 16, 24), (9, 10, 21)]
# density: (components, those over more than one 8^3 tile, the largest's voxels, its tiles)
FIGURES = {0.04: (300, 24, 9, 1), 0.1: (294, 57, 84, 8), 0.3: (24, 4, 1762, 12)}
ORIGIN, DIMS, SEED = (-37, -35, -21), (77, 70, 59), (-20, -20, -5)
# the floor-and-box scene: (marked, clusters of 8 voxels or more, the largest) without a travel field and
# with the one of clearance2 = 4 from SEED
SCENE = {False: (5528, 1, 5528), True: (5276, 1, 5276)}


def both(mask):
    a, b = fr.label_flood(mask), fr.label_sweep(mask)
    assert a.dtype == np.uint32 and np.array_equal(a, b)
    assert np.array_equal(a != fr.NONE, np.asarray(mask) != 0)
    return a


@pytest.mark.parametrize("density", sorted(FIGURES))
def test_shape_figures(density):
    total, multi, largest = 0, 0, (0, 0)
    for mask in fr.masks(SHAPES, density):
        lab = both(mask)
        tab, n = fr.table(lab)
        assert n == len(tab) and int(tab["size"].sum()) == int(mask.sum())
        assert np.array_equal(tab["label"], np.unique(lab[lab != fr.NONE])) and (tab["goal"] == tab["label"]).all()
        total += n
        for c in tab:
            tiles = fr.tiles_spanned(lab, c["label"])
            multi += tiles > 1
            largest = max(largest, (int(c["size"]), tiles))
    assert (total, multi, *largest) == FIGURES[density]


def test_table_fields():
    """A hand-made mask: two components, a key with ties, min_size."""
    m = np.zeros((2, 3, 4), np.uint8)
    m[0, 0, 0] = m[0, 1, 1] = m[1, 2, 2] = 1  # a diagonal chain: (0,0,0) - (1,1,0) - (2,2,1)
    m[0, 0, 3] = 1                            # alone
    lab = both(m)
    key = np.full(m.shape, 9, np.uint32)
    key[0, 1, 1] = key[1, 2, 2] = 4           # a tie: the lesser index wins
    tab, total = fr.table(lab, key)
    assert total == 2 and tab["label"].tolist() == [0, 3] and tab["size"].tolist() == [3, 1]
    assert tab["lo"].tolist() == [[0, 0, 0], [3, 0, 0]] and tab["hi"].tolist() == [[2, 2, 1], [3, 0, 0]]
    assert tab["sum"].tolist() == [[3, 3, 1], [3, 0, 0]]
    assert tab["goal"].tolist() == [5, 3] and tab["goal_key"].tolist() == [4, 9]
    assert fr.table(lab, key, 2)[0]["label"].tolist() == [0] and len(fr.table(lab, key, 4)[0]) == 0
    assert fr.COMPONENT_DTYPE.itemsize == 64


def test_maze_figures():
    ok = tr.serpentine(64, 64, 8, pitch=2, gap=1)
    for mask, label in ((ok, 0), (ok[::-1, :, ::-1], None)):
        lab = both(mask)
        tab, total = fr.table(lab)
        assert total == 1 and tab["size"][0] == 16640 == 64 * 8 * 32 + 32 * 8
        assert label is None or tab["label"][0] == label
    tab, total = fr.table(fr.label_flood(~ok))
    assert total == 32 and set(tab["size"].tolist()) == {504}


def test_mark():
    state = np.ones((3, 4, 5), np.uint8)
    assert fr.mark(state).sum() == 0  # neighbours outside the box never count
    state[1, 2, 2] = 0
    m = fr.mark(state)
    assert m.sum() == 6 and m[1, 2, 1] and m[1, 2, 3] and m[0, 2, 2] and m[2, 2, 2] and not m[0, 1, 1] and not m[1, 2, 2]
    state[1, 2, 1] = 2  # inside a surface: no frontier
    cost = np.zeros(state.shape, np.uint32)
    cost[1, 2, 3] = fr.UNREACHED
    assert fr.mark(state).sum() == 5 and fr.mark(state, cost).sum() == 4


@pytest.fixture(scope="module")
def scene():
    return _edt_ref.distance_field(_edt_ref.records_dump(_edt_ref.scene_records()), ORIGIN, DIMS)


@pytest.mark.parametrize("with_travel", [False, True])
def test_scene_figures(scene, with_travel):
    """The figures tests/test_gpu_frontier.py relies on, from the restatement alone."""
    cost = None
    if with_travel:
        cost = tr.field(tr.passable(scene["d2"], scene["state"], 4, False), [np.array(SEED) - np.array(ORIGIN)])[0]
    mask = fr.mark(scene["state"], cost)
    tab, _ = fr.table(fr.label_flood(mask), cost, 8)
    assert (int(mask.sum()), len(tab), int(tab["size"].max())) == SCENE[with_travel]


def test_binding_declares_frontier():
    import tsdf_amd
    from tsdf_amd import _lib
    L = tsdf_amd.load_library()
    for name in ("tsdf_components_config_default", "tsdf_frontier_mark", "tsdf_components"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert C.sizeof(_lib.ComponentsConfig) == 16 and C.sizeof(_lib.Component) == 64
    assert tsdf_amd.COMPONENT_DTYPE == fr.COMPONENT_DTYPE and tsdf_amd.COMPONENT_DTYPE.itemsize == 64
    for name, typ in _lib.Component._fields_:
        assert getattr(_lib.Component, name).offset == fr.COMPONENT_DTYPE.fields[name][1], name
    assert _lib.TSDF_COMPONENT_NONE == fr.NONE == tsdf_amd.TSDF_COMPONENT_NONE
    for m in ("frontier_mask", "components", "frontiers"):
        assert callable(getattr(tsdf_amd.Engine, m))
    c = _lib.ComponentsConfig(dims=(C.c_int32 * 3)(7, 7, 7), min_size=5)
    L.tsdf_components_config_default(C.byref(c))
    assert list(c.dims) == [0, 0, 0] and c.min_size == 1
    # the header's argument lists, parameter for parameter
    text = open(os.path.join(ROOT, "include", "disinfect_tsdf.h")).read()
    for name, fn in {"tsdf_frontier_mark": L.tsdf_frontier_mark, "tsdf_components": L.tsdf_components}.items():
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
        assert len(params) == len(fn.argtypes), name
        for p, a in zip(params, fn.argtypes):
            if "*" in p or "[" in p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            elif p.startswith("int32_t"):
                assert a is C.c_int32, (name, p)
            else:
                assert p.startswith("int ") and a is C.c_int, (name, p)
        assert fn.restype is C.c_int
    # invalid arguments are refused before any device work
    n, one, two = C.c_int64(7), C.c_int32(7), C.c_int32(7)
    assert L.tsdf_frontier_mark(None, None, None, None, None, 0, C.byref(n)) == 1 and n.value == 7
    assert L.tsdf_components(None, None, None, None, None, 0, None, 0, C.byref(one), C.byref(two)) == 1
    assert (one.value, two.value) == (7, 7)


def test_esdf_helpers_match_host_header():
    rng = np.random.default_rng(21)
    dims, origin, voxel = (12, 9, 7), (10, -5, 2), np.float32(0.02)
    mask = rng.random(dims[::-1]) < 0.04
    key = rng.integers(0, 6, mask.shape).astype(np.uint32) * 7
    key[rng.random(mask.shape) < 0.5] = fr.UNREACHED
    lab = fr.label_flood(mask)
    tab, total = fr.table(lab, key)
    assert total >= 3 and (tab["goal_key"] == fr.UNREACHED).any() and (tab["goal_key"] != fr.UNREACHED).any()
    res = dict(label=lab, clusters=tab, count=len(tab), total=total, origin=origin, dims=dims)
    g = esdf.frontier_goals(res, voxel)
    assert g["goal"].dtype == g["centroid"].dtype == g["metres"].dtype == np.float32
    assert g["goal"].shape == g["centroid"].shape == (len(tab), 3) and g["metres"].shape == (len(tab),)
    # by hand for the first cluster
    c = tab[0]
    gz, r = divmod(int(c["goal"]), dims[0] * dims[1])
    gy, gx = divmod(r, dims[0])
    assert np.array_equal(g["goal"][0], (np.array([gx, gy, gz]) + origin).astype(np.float32) * voxel)
    assert lab.reshape(-1)[c["goal"]] == c["label"] and key.reshape(-1)[c["goal"]] == c["goal_key"]
    for k in range(len(tab)):
        v = esdf.frontier_voxels(res, k)
        assert v.shape == (tab["size"][k], 3) and v.dtype == np.int64
        assert np.array_equal(v.sum(0) - tab["size"][k] * np.array(origin), tab["sum"][k])
        assert np.array_equal(v.min(0) - origin, tab["lo"][k]) and np.array_equal(v.max(0) - origin, tab["hi"][k])
    line = f"goals {dims[0]} {dims[1]} {dims[2]} {origin[0]} {origin[1]} {origin[2]} {float(voxel)!r} {len(tab)} " + \
        " ".join(f"{c['label']} {c['size']} {c['sum'][0]} {c['sum'][1]} {c['sum'][2]} {c['goal']} {c['goal_key']}" for c in tab)
    r = subprocess.run([BIN], input=line + "\nnonsense\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == 2 and out[1].startswith("error")
    got = np.array([float(v) for v in out[0].split()], np.float32).reshape(-1, 7)
    assert np.array_equal(got[:, :3], g["goal"]) and np.array_equal(got[:, 3:6], g["centroid"])
    assert np.array_equal(got[:, 6], g["metres"]) and np.isinf(got[:, 6]).any()
