"""bench.py without a GPU: the options of the plain / --full split, and the sample --dump-outputs
reads (a stub engine stands in for the volume)."""
import os
import sys
import types

import numpy as np


def _parse(monkeypatch, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, ["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


class _StubEngine:
    """Holds the voxels with even x (the other stub: odd x), as two shards of one volume would."""

    def __init__(self, parity):
        self.parity = parity

    def hash_retrieve(self, points):
        p = np.asarray(points)
        own = (p[:, 0] & 1) == self.parity
        return dict(rgbw=np.where(own[:, None], np.uint8(7), np.uint8(0)) * np.ones((1, 4), np.uint8),
                    tsdf=np.where(own, np.float32(0.25), np.float32(1.0)),
                    prob=np.where(own, np.float32(0.5), np.float32(0.0)),
                    block_idx=np.where(own, 3, -1).astype(np.int32))

    def stats(self):
        return dict(active_blocks=10, last_num_visible=4, last_num_updated=100)


def test_dump_outputs_sample_is_fixed_and_float(tmp_path):
    import bench
    from tsdf_amd import synth
    cam = synth.camera(80, 60)
    depth = synth.render(cam, 5)["depth"]
    out = []
    for name in ("a", "b"):
        a = types.SimpleNamespace(dump_outputs=str(tmp_path / name), width=80, height=60, voxel=0.005)
        bench.dump_outputs(a, [_StubEngine(0), _StubEngine(1)], depth, 5,
                           images={"raycast_rgba": None}, mesh_tris=[12])
        out.append({f[:-4]: np.load(os.path.join(a.dump_outputs, f)) for f in sorted(os.listdir(a.dump_outputs))})
    a, b = out
    assert set(a) == {"voxel_xyz", "tsdf", "prob", "rgbw", "counts", "mesh_triangles"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    n = a["voxel_xyz"].shape[0]
    assert n > 1000 and a["rgbw"].shape == (n, 4)
    # every sampled coordinate lies inside the room (6 x 5 x 3 m, 5 mm voxels, +- the sampled band)
    assert a["voxel_xyz"].min() >= -5 and np.all(a["voxel_xyz"].max(0) <= np.array([1205, 1005, 605]))
    assert len(np.unique(a["voxel_xyz"], axis=0)) == n
    # each voxel came from the shard that holds it
    assert np.all(a["tsdf"] == 0.25) and np.all(a["prob"] == 0.5) and np.all(a["rgbw"] == 7)
    assert list(a["counts"]) == [20, 8, 200] and list(a["mesh_triangles"]) == [12]
