"""tsdf_amd.mesh_io (binary PLY of an indexed semantic mesh) and the binding's declaration of
tsdf_extract_mesh_indexed. No GPU."""
import numpy as np


def _mesh():
    rng = np.random.default_rng(7)
    n, m = 37, 61
    prob = rng.random(n).astype(np.float32)
    prob[5] = np.nan
    return dict(positions=rng.standard_normal((n, 3)).astype(np.float32),
                rgba=rng.integers(0, 256, (n, 4)).astype(np.uint8), prob=prob,
                keys=rng.integers(-500, 500, (n, 4)).astype(np.int32),
                indices=rng.integers(0, n, (m, 3)).astype(np.int32))


def test_ply_round_trip(tmp_path):
    from tsdf_amd import mesh_io
    mesh = _mesh()
    path = tmp_path / "mesh.ply"
    mesh_io.write_ply(path, mesh)
    back = mesh_io.read_ply(path)
    assert np.array_equal(back["positions"].view(np.uint32), mesh["positions"].view(np.uint32))
    assert np.array_equal(back["rgba"], mesh["rgba"])
    assert np.array_equal(back["prob"].view(np.uint32), mesh["prob"].view(np.uint32))
    assert np.array_equal(back["indices"], mesh["indices"])
    assert back["positions"].dtype == np.float32 and back["rgba"].dtype == np.uint8
    assert back["prob"].dtype == np.float32 and back["indices"].dtype == np.int32
    # a vertex is 3 floats, 4 bytes and 1 float; a face 1 count byte and 3 ints
    head = len(mesh_io.header(37, 61).encode("ascii"))
    assert path.stat().st_size == head + 37 * 20 + 61 * 13


def test_ply_header_and_empty_mesh(tmp_path):
    from tsdf_amd import mesh_io
    path = tmp_path / "mesh.ply"
    mesh_io.write_ply(path, _mesh())
    lines = path.read_bytes().split(b"end_header\n")[0].decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    assert "element vertex 37" in lines and "element face 61" in lines
    props = [ln for ln in lines if ln.startswith("property")]
    assert props == ["property float x", "property float y", "property float z",
                     "property uchar red", "property uchar green", "property uchar blue",
                     "property uchar alpha", "property float quality",
                     "property list uchar int vertex_indices"]
    empty = dict(positions=np.zeros((0, 3), np.float32), rgba=np.zeros((0, 4), np.uint8),
                 prob=np.zeros(0, np.float32), indices=np.zeros((0, 3), np.int32))
    mesh_io.write_ply(path, empty)
    back = mesh_io.read_ply(path)
    assert all(back[k].shape == empty[k].shape for k in empty)
    # positions and indices alone: white, probability 0
    mesh_io.write_ply(path, dict(positions=_mesh()["positions"], indices=_mesh()["indices"]))
    back = mesh_io.read_ply(path)
    assert (back["rgba"] == 255).all() and (back["prob"] == 0).all()


def test_binding_declares_indexed_mesh():
    import ctypes as C
    import tsdf_amd
    from tsdf_amd import _lib
    assert "tsdf_extract_mesh_indexed" in _lib.EXPORTS
    L = tsdf_amd.load_library()
    fn = L.tsdf_extract_mesh_indexed
    assert fn.restype is C.c_int and len(fn.argtypes) == 7
    assert [f[0] for f in _lib.MeshOut._fields_] == ["positions", "rgba", "prob", "keys", "indices",
                                                     "vertex_capacity", "triangle_capacity", "mem_kind"]
    assert C.sizeof(_lib.MeshOut) == 5 * 8 + 2 * 8 + 8  # as the C struct on LP64 (int + padding)
    assert callable(tsdf_amd.Engine.extract_mesh_indexed)
    # invalid arguments are refused before any device work
    nv = C.c_int64()
    assert fn(None, None, 0.99, 0, None, C.byref(nv), C.byref(nv)) == 1
