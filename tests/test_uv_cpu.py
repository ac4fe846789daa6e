"""The host side of the UV dose feature, no GPU: tsdf_amd.uv (tube lamp, dose carry-over, coverage), the
PLY writer's optional dose property, the binding's declarations, and host/uv_dose.h through the stand-alone
uv_host_main."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "uv_host_main")
f32 = np.float32


def test_tube_emitters():
    from tsdf_amd import uv
    p0, p1 = np.array([0.5, -1.0, 0.25]), np.array([0.5, 1.0, 1.25])
    e = uv.tube_emitters(p0, p1, 36.0, 2.5, 8)
    assert e.shape == (8, 4) and e.dtype == f32
    assert abs(float(e[:, 3].astype(np.float64).sum()) - 36.0 * 2.5) <= 1e-5
    assert np.all(e[:, 3] == f32(36.0 * 2.5 / 8))
    mid = p0 + ((np.arange(8) + 0.5) / 8)[:, None] * (p1 - p0)
    assert np.abs(e[:, :3] - mid).max() <= 1e-6
    one = uv.tube_emitters(p0, p1, 10.0, 1.0, 1)
    assert np.allclose(one[0], [0.5, 0.0, 0.75, 10.0])
    with pytest.raises(ValueError):
        uv.tube_emitters(p0, p1, 1.0, 1.0, 0)


def _keys(rng, n):
    k = np.unique(np.concatenate([rng.integers(-300, 300, (n, 3)), rng.integers(0, 3, (n, 1))], axis=1), axis=0)
    return rng.permutation(k).astype(np.int32)


def test_carry_dose_permuted_and_partly_new():
    from tsdf_amd import uv
    rng = np.random.default_rng(11)
    old = _keys(rng, 500)
    dose = rng.random(old.shape[0]).astype(f32) * 100
    fresh = _keys(rng, 200) + np.array([1000, 0, 0, 0], np.int32)  # keys the old mesh never had
    keep = rng.permutation(old.shape[0])[:300]
    new = np.concatenate([old[keep], fresh])
    perm = rng.permutation(new.shape[0])
    got = uv.carry_dose(old, dose, new[perm])
    want = np.concatenate([dose[keep], np.zeros(fresh.shape[0], f32)])[perm]
    assert got.dtype == f32 and np.array_equal(got, want)
    # the axis is part of the key; negative coordinates are keys like any other
    old2 = np.array([[-1, -2, -3, 0], [-1, -2, -3, 1]], np.int32)
    assert np.array_equal(uv.carry_dose(old2, [5.0, 7.0], [[-1, -2, -3, 1], [-1, -2, -3, 2], [-1, -2, -3, 0]]),
                          np.array([7, 0, 5], f32))
    assert uv.carry_dose(np.zeros((0, 4), np.int32), [], old).tolist() == [0.0] * old.shape[0]
    assert uv.carry_dose(old, dose, np.zeros((0, 4), np.int32)).shape == (0,)


def test_coverage_hand_made():
    from tsdf_amd import uv
    dose = [12.0, 3.0, 10.0, 50.0, 0.0]
    prob = [0.9, 0.6, 0.5, 0.2, 0.8]
    # prob >= 0.5: vertices 0, 1, 2, 4 (weights 0.9 + 0.6 + 0.5 + 0.8 = 2.8); dosed (>= 10): 0 and 2 -> 1.4
    assert abs(uv.coverage(dose, prob, 10.0) - 1.4 / 2.8) <= 1e-12
    assert abs(uv.coverage(dose, prob, 10.0, prob_min=0.85) - 1.0) <= 1e-12
    assert uv.coverage(dose, prob, 100.0) == 0.0
    assert uv.coverage([1.0], [0.1], 10.0) == 1.0  # no high-touch vertex: nothing left to do


def _mesh():
    rng = np.random.default_rng(5)
    n, m = 9, 4
    return dict(positions=rng.standard_normal((n, 3)).astype(f32), rgba=rng.integers(0, 256, (n, 4)).astype(np.uint8),
                prob=rng.random(n).astype(f32), indices=rng.integers(0, n, (m, 3)).astype(np.int32))


def test_ply_dose_round_trip_and_identity_without(tmp_path):
    from tsdf_amd import mesh_io
    mesh = _mesh()
    n, m = 9, 4
    dose = (np.arange(n) * 1.5).astype(f32)
    dose[3] = np.inf
    path = tmp_path / "dose.ply"
    mesh_io.write_ply(path, mesh, dose=dose)
    back = mesh_io.read_ply(path)
    assert np.array_equal(back["dose"].view(np.uint32), dose.view(np.uint32)) and back["dose"].dtype == f32
    for k in ("positions", "rgba", "prob", "indices"):
        assert np.array_equal(back[k], mesh[k]), k
    head = path.read_bytes().split(b"end_header\n")[0].decode("ascii").split("\n")
    props = [ln for ln in head if ln.startswith("property")]
    assert props[7:] == ["property float quality", "property float dose", "property list uchar int vertex_indices"]
    assert path.stat().st_size == len(mesh_io.header(n, m, True)) + n * 24 + m * 13
    # without a dose: the file as it has always been, written out here by hand
    plain = tmp_path / "plain.ply"
    mesh_io.write_ply(plain, mesh)
    want = ("ply\nformat binary_little_endian 1.0\ncomment tsdf_amd indexed semantic mesh\n"
            f"element vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
            f"property float quality\nelement face {m}\nproperty list uchar int vertex_indices\nend_header\n"
            ).encode("ascii")
    for i in range(n):
        want += struct.pack("<3f4Bf", *mesh["positions"][i], *mesh["rgba"][i], mesh["prob"][i])
    for t in mesh["indices"]:
        want += struct.pack("<B3i", 3, *t)
    assert plain.read_bytes() == want
    assert "dose" not in mesh_io.read_ply(plain)
    mesh_io.write_ply(plain, mesh, dose=None)
    assert plain.read_bytes() == want


def test_binding_declares_uv_dose():
    import ctypes as C
    import tsdf_amd
    from tsdf_amd import _lib
    L = tsdf_amd.load_library()
    for name in ("tsdf_uv_config_default", "tsdf_surface_normals", "tsdf_uv_dose"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert C.sizeof(_lib.UvEmitter) == 16 and C.sizeof(_lib.UvConfig) == 28
    assert [f[0] for f in _lib.UvConfig._fields_] == ["bias", "step", "min_range", "max_range", "sample_offset",
                                                      "min_weight", "use_grid"]
    assert callable(tsdf_amd.Engine.uv_dose) and callable(tsdf_amd.Engine.surface_normals)
    c = _lib.UvConfig()
    L.tsdf_uv_config_default(None, C.byref(c))  # without an engine: the reference's 5 mm voxel
    assert (c.min_range, c.max_range, c.min_weight, c.use_grid) == (f32(0.05), 5.0, 1, 1)
    # invalid arguments are refused before any device work
    assert L.tsdf_uv_dose(None, None, None, 0, None, 0, None, None, 0) == 1
    assert L.tsdf_surface_normals(None, None, 0, 0.0, None, 0) == 1


def _run(lines):
    r = subprocess.run([BIN], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [ln.split() for ln in out]


def test_host_header_matches_numpy():
    """host/uv_dose.h (C++) against tsdf_amd.uv on the same inputs."""
    from tsdf_amd import uv
    rng = np.random.default_rng(3)
    p0, p1 = np.array([0.5, -1.0, 0.25], f32), np.array([0.5, 1.0, 1.25], f32)
    old = _keys(rng, 60)
    dose = rng.random(old.shape[0]).astype(f32)
    new = np.concatenate([old[rng.permutation(old.shape[0])[:40]], _keys(rng, 20) + np.array([900, 0, 0, 0], np.int32)])
    new = new[rng.permutation(new.shape[0])]
    num = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))
    ints = lambda a: " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))
    tube, carry, bad, zero = _run([
        f"tube {num(p0)} {num(p1)} 36.0 2.5 8",
        f"carry {old.shape[0]} {new.shape[0]} {ints(old)} {num(dose)} {ints(new)}",
        f"tube {num(p0)} {num(p1)} 36.0 2.5 0",
        "carry 0 2 1 2 3 0 4 5 6 1",
    ])
    got = np.array([float(v) for v in tube], f32).reshape(8, 4)
    assert np.array_equal(got, uv.tube_emitters(p0, p1, 36.0, 2.5, 8))
    assert np.array_equal(np.array([float(v) for v in carry], f32), uv.carry_dose(old, dose, new))
    assert bad[0] == "error"
    assert [float(v) for v in zero] == [0.0, 0.0]
