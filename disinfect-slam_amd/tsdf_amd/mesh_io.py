"""Binary little-endian PLY of an indexed semantic mesh (Engine.extract_mesh_indexed), pure numpy.

Vertex properties: x y z float, red green blue alpha uchar (alpha = the fusion weight), quality
float (the high-touch probability: MeshLab and CloudCompare show it as a scalar field), and when a dose
is given a further float `dose` (the accumulated UV dose, J/m^2). Faces: `list uchar int vertex_indices`.
"""
from __future__ import annotations

import numpy as np

VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                         ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1"),
                         ("quality", "<f4")])
DOSE_VERTEX_DTYPE = np.dtype(VERTEX_DTYPE.descr + [("dose", "<f4")])
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
_PLY_TYPES = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}


def _host(a, dtype):
    if hasattr(a, "detach"):  # a torch tensor (extract_mesh_indexed(device=True))
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def header(num_vertices: int, num_faces: int, dose: bool = False) -> str:
    vt = DOSE_VERTEX_DTYPE if dose else VERTEX_DTYPE
    lines = ["ply", "format binary_little_endian 1.0", "comment tsdf_amd indexed semantic mesh",
             f"element vertex {num_vertices}"]
    lines += [f"property {_PLY_TYPES[vt[n].str]} {n}" for n in vt.names]
    lines += [f"element face {num_faces}", "property list uchar int vertex_indices", "end_header"]
    return "\n".join(lines) + "\n"


def write_ply(path, mesh: dict, dose=None) -> None:
    """mesh: positions (n, 3), indices (m, 3), and optionally rgba (n, 4) and prob (n,); a missing
    colour is written as opaque white, a missing probability as 0. dose (n,): written as one more
    vertex property `dose`; without it the file has the eight properties alone."""
    pos = _host(mesh["positions"], np.float32).reshape(-1, 3)
    idx = _host(mesh["indices"], np.int32).reshape(-1, 3)
    n = pos.shape[0]
    v = np.zeros(n, VERTEX_DTYPE if dose is None else DOSE_VERTEX_DTYPE)
    v["x"], v["y"], v["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    rgba = mesh.get("rgba")
    rgba = np.full((n, 4), 255, np.uint8) if rgba is None else _host(rgba, np.uint8).reshape(n, 4)
    v["red"], v["green"], v["blue"], v["alpha"] = rgba[:, 0], rgba[:, 1], rgba[:, 2], rgba[:, 3]
    prob = mesh.get("prob")
    v["quality"] = 0 if prob is None else _host(prob, np.float32).reshape(n)
    if dose is not None:
        v["dose"] = _host(dose, np.float32).reshape(n)
    f = np.zeros(idx.shape[0], FACE_DTYPE)
    f["n"] = 3
    f["v"] = idx
    with open(path, "wb") as out:
        out.write(header(n, idx.shape[0], dose is not None).encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def read_ply(path) -> dict:
    """Reads what write_ply wrote (its two headers only): positions, rgba, prob, indices, and dose
    when the file has it."""
    with open(path, "rb") as inp:
        data = inp.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    n, m = counts["vertex"], counts["face"]
    has_dose = data[:end].decode("ascii") == header(n, m, True)
    if not has_dose and data[:end].decode("ascii") != header(n, m):
        raise ValueError("not a PLY file written by tsdf_amd.mesh_io.write_ply")
    vt = DOSE_VERTEX_DTYPE if has_dose else VERTEX_DTYPE
    v = np.frombuffer(data, vt, n, end)
    f = np.frombuffer(data, FACE_DTYPE, m, end + n * vt.itemsize)
    if m and not (f["n"] == 3).all():
        raise ValueError("faces must be triangles")
    out = dict(positions=np.stack([v["x"], v["y"], v["z"]], axis=1) if n else np.zeros((0, 3), np.float32),
               rgba=np.stack([v["red"], v["green"], v["blue"], v["alpha"]], axis=1) if n else np.zeros((0, 4), np.uint8),
               prob=v["quality"].copy(), indices=f["v"].copy().reshape(-1, 3))
    if has_dose:
        out["dose"] = v["dose"].copy()
    return out
