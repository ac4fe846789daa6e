"""The box calls' sections and staging (csrc/tsdf_box.h Sections, tsdf_host.h Stage; DESIGN.md "Box calls"): every
box call with every combination of its optional arrays gives the same bits through host arrays and through device
tensors, whichever layout its scratch buffer served before. The box, 33 x 9 x 5 voxels, crosses a 32-bit word and an
8-voxel tile in x: the smallest setting in which a mis-resolved section or a skipped zero-size section shows."""
import numpy as np
import pytest

import _free_ref as fref

pytestmark = pytest.mark.gpu

VOXEL, TRUNC = 0.005, 0.03
DIMS, ORIGIN = (33, 9, 5), (-16, -4, 6)
SHAPE = DIMS[::-1]
K, W, H = (20.0, 20.0, 7.5, 5.5), 16, 12


def host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)


def inputs():
    """The hand-made arrays every call reads; nothing changes them (each call gets a copy where it writes)."""
    rng = np.random.default_rng(5)
    state = rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), size=SHAPE)
    d2 = rng.integers(0, 12, SHAPE).astype(np.uint16)
    seeds = np.argwhere((state == 1) & (d2 >= 4))[::37][:, ::-1] + np.asarray(ORIGIN)
    bits = fref.pack(rng.random(SHAPE) < 0.4)
    cost = np.where(state == 1, rng.integers(0, 200, SHAPE), 0xFFFFFFFF).astype(np.uint32)
    mask = (rng.random(SHAPE) < 0.3).astype(np.uint8)
    depth = np.full((H, W), 0.3, np.float32)
    depth[::5, ::3] = 0.0
    depth[3:6, 4:9] = 0.04
    return dict(state=state, d2=d2, seeds=seeds, cost=cost, mask=mask, bits=np.ascontiguousarray(bits), depth=depth)


def new_engine():
    """An engine whose volume holds one synthetic frame, and a box of DIMS around a surface point of it."""
    import tsdf_amd
    from tsdf_amd import esdf, synth
    cam = synth.camera(80, 60)
    eng = tsdf_amd.Engine(voxel_size=VOXEL, truncation=TRUNC, max_width=80, max_height=60, num_block_bits=14)
    fr = synth.render(cam, 0)
    pose = tsdf_amd.SE3(fr["q"], fr["t"])
    eng.integrate(fr["rgb"], fr["depth"], fr["ht"], fr["lt"], cam.K, pose, 4.0)
    pt = eng.raycast_surface(cam.K, 80, 60, pose, 4.0, maps=())["point"]
    hit = pt[np.abs(pt).sum(axis=-1) > 0]
    assert len(hit), "the synthetic frame shows no surface"
    c = esdf.voxel_of(hit[len(hit) // 2][None], VOXEL)[0]
    return eng, tuple(int(v) for v in c - np.asarray(DIMS) // 2)


def calls(eng, edt_origin, X):
    """(name, fn(device) -> the call's results as host arrays), in the order that serves each buffer's layout with
    the optional sections first."""
    import torch
    import tsdf_amd
    field = dict(d2=X["d2"], state=X["state"], origin=ORIGIN, dims=DIMS)
    views = [tsdf_amd.SE3(), tsdf_amd.SE3((0.0, 0.0, 0.0, 1.0), (0.01, 0.0, 0.02))]

    def layer(device):
        b = X["bits"].copy()
        return dict(bits=torch.as_tensor(b.view(np.int32), device=f"cuda:{eng.device}") if device else b,
                    origin=ORIGIN, dims=DIMS)

    def travel(device):
        r = eng.travel_field(field, X["seeds"], clearance2=4, device=device)
        assert r["seeded"] > 0 and (host(r["cost"]) != 0xFFFFFFFF).sum() > r["seeded"]
        return host(r["cost"]), r["seeded"]

    tv = dict(cost=X["cost"], origin=ORIGIN, dims=DIMS)

    def frontier(with_travel, count):
        def fn(device):
            r = eng.frontier_mask(field, tv if with_travel else None, device=device, count=count)
            m = host(r["mask"])
            assert (r["marked"] is None) == (not count) and 0 < m.sum() < m.size
            return m, r["marked"]
        return fn

    def components(with_key):
        def fn(device):
            r = eng.components(X["mask"], DIMS, key=X["cost"] if with_key else None, device=device)
            assert r["count"] >= 1 and r["total"] >= r["count"]
            return host(r["label"]), r["clusters"].tobytes(), r["count"], r["total"]
        return fn

    def apply(count):
        def fn(device):
            r = eng.free_apply(layer(device), field, count=count)
            assert (r["promoted"] is None) == (not count) and not np.shares_memory(host(r["state"]), X["state"])
            return host(r["state"]), r["promoted"]
        return fn

    def observe(device):
        lay = eng.free_observe(layer(device), X["depth"], K, tsdf_amd.SE3(), 1.0)
        got = host(lay["bits"]).view(np.uint32)
        assert (got & X["bits"] == X["bits"]).all() and (got != X["bits"]).any() and fref.padding(got, DIMS[0]) == 0
        return (got,)

    def gain(with_seen, depth):
        def fn(device):
            seen = dict(bits=X["bits"], origin=ORIGIN, dims=DIMS) if with_seen else None
            r = eng.view_gain(field, views, K, W, H, 0.3, margin=VOXEL, seen=seen, depth=depth, device=device)
            assert (r["depth"] is None) == (not depth) and r["gain"].sum() > 0
            return (r["gain"],) + ((host(r["depth"]).view(np.uint32),) if depth else ())
        return fn

    def edt(with_state):
        def fn(device):
            r = eng.distance_field(edt_origin, DIMS, max_dist=9, state=with_state, device=device)
            d2 = host(r["d2"])
            assert d2.min() == 0 and d2.max() > 0 and (r["state"] is None) == (not with_state)
            return (d2,) + ((host(r["state"]),) if with_state else ())
        return fn

    return [("travel_field", travel),
            ("frontier_mask travel count", frontier(True, True)), ("frontier_mask travel", frontier(True, False)),
            ("frontier_mask count", frontier(False, True)), ("frontier_mask", frontier(False, False)),
            ("components key", components(True)), ("components", components(False)),
            ("free_apply count", apply(True)), ("free_apply", apply(False)), ("free_observe", observe),
            ("view_gain seen depth", gain(True, True)), ("view_gain seen", gain(True, False)),
            ("view_gain depth", gain(False, True)), ("view_gain", gain(False, False)),
            ("distance_field state", edt(True)), ("distance_field", edt(False))]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def run_all(backwards):
    """Every call through host arrays and device tensors on a fresh engine: the host call's layout (with its
    staging sections) first, or with backwards everything the other way round."""
    eng, edt_origin = new_engine()
    X = inputs()
    kept = {k: v.copy() for k, v in X.items()}
    out = {}
    seq = calls(eng, edt_origin, X)
    for name, fn in (seq[::-1] if backwards else seq):
        got = [fn(device) for device in ((True, False) if backwards else (False, True))]
        assert same(got[0], got[1]), f"{name}: host arrays and device tensors differ"
        out[name] = got[0]
    assert all(np.array_equal(X[k], kept[k]) for k in X), "a call changed its input"
    assert eng.stats()["status"] == 0
    eng.close()
    return out, edt_origin


def test_host_and_device_agree_in_either_order():
    fwd, o1 = run_all(False)
    bwd, o2 = run_all(True)
    assert o1 == o2 and fwd.keys() == bwd.keys() and len(fwd) == 16
    for name in fwd:
        assert same(fwd[name], bwd[name]), f"{name}: the result depends on what the buffer served before"
