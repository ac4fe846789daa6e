"""The lamp model and the dose bookkeeping around Engine.uv_dose (DESIGN.md "UV dose"), numpy only:
a tube lamp as point emitters, the dose of a re-extracted mesh carried over by vertex key, and the
coverage of the high-touch surface; for the lamp-stop planner (DESIGN.md "Lamp-stop planning";
Engine.uv_irradiance / uv_plan) a batch of candidate tubes, the missing dose and the vertex areas.
host/uv_dose.h is the same in C++."""
from __future__ import annotations

import numpy as np


def tube_emitters(p0, p1, power_w: float, dwell_s: float, segments: int) -> np.ndarray:
    """A tube lamp from p0 to p1 [m] that radiated power_w for dwell_s seconds, as `segments` point
    emitters at the midpoints of its equal segments, each with power_w * dwell_s / segments joules:
    (segments, 4) f32 rows x, y, z, energy, as Engine.uv_dose takes them."""
    if segments < 1:
        raise ValueError("tube_emitters: segments >= 1")
    p0, p1 = np.asarray(p0, np.float64).reshape(3), np.asarray(p1, np.float64).reshape(3)
    t = (np.arange(segments, dtype=np.float64) + 0.5) / segments
    out = np.empty((segments, 4), np.float32)
    out[:, :3] = p0 + t[:, None] * (p1 - p0)
    out[:, 3] = float(power_w) * float(dwell_s) / segments
    return out


def _key_view(keys) -> np.ndarray:
    k = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, 4)
    return k.view(np.dtype((np.void, 16))).reshape(-1)


def carry_dose(old_keys, old_dose, new_keys) -> np.ndarray:
    """The dose of every vertex of a new extraction whose (gx, gy, gz, axis) key (extract_mesh_indexed's
    `keys`) existed in the old one, 0 for the rest: (len(new_keys),) f32."""
    old, new = _key_view(old_keys), _key_view(new_keys)
    old_dose = np.asarray(old_dose, np.float32).reshape(-1)
    if old.size != old_dose.size:
        raise ValueError("carry_dose: one dose per old key")
    out = np.zeros(new.size, np.float32)
    if old.size == 0 or new.size == 0:
        return out
    order = np.argsort(old, kind="stable")
    sk = old[order]
    i = np.minimum(np.searchsorted(sk, new), sk.size - 1)
    hit = sk[i] == new
    out[hit] = old_dose[order[i[hit]]]
    return out


def coverage(dose, prob, target: float, prob_min: float = 0.5) -> float:
    """The share of the high-touch surface that has its dose: over the vertices with prob >= prob_min,
    sum(prob where dose >= target) / sum(prob). 1.0 when no vertex qualifies (nothing left to do)."""
    dose, prob = np.asarray(dose, np.float64).reshape(-1), np.asarray(prob, np.float64).reshape(-1)
    if dose.size != prob.size:
        raise ValueError("coverage: one probability per dose")
    sel = prob >= prob_min
    total = prob[sel].sum()
    if not total > 0:
        return 1.0
    return float(prob[sel & (dose >= target)].sum() / total)


def tube_candidates(centres, axis, length: float, power_w: float, dwell_s: float, segments: int):
    """One tube lamp per (C, 3) centre [m], all along `axis` (any length, not zero) and `length` metres
    long: tube_emitters(centre - h, centre + h, ...) with h = axis / |axis| * length / 2 for each, as
    Engine.uv_irradiance takes them: (emitters (C * segments, 4) f32, first (C + 1,) int32)."""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    a = np.asarray(axis, np.float64).reshape(3)
    norm = float(np.sqrt((a * a).sum()))
    if not norm > 0:
        raise ValueError("tube_candidates: axis is zero")
    if segments < 1:
        raise ValueError("tube_candidates: segments >= 1")
    h = a / norm * (float(length) / 2)
    em = [tube_emitters(p - h, p + h, power_w, dwell_s, segments) for p in c]
    emitters = np.concatenate(em) if em else np.zeros((0, 4), np.float32)
    return emitters, (np.arange(c.shape[0] + 1, dtype=np.int64) * segments).astype(np.int32)


def plan_need(dose, prob, target: float, prob_min: float = 0.5) -> np.ndarray:
    """What each vertex still lacks, as Engine.uv_plan takes it: max(target - dose, 0) in float32 where
    prob >= prob_min (coverage's high-touch surface), 0 elsewhere."""
    dose, prob = np.asarray(dose, np.float32).reshape(-1), np.asarray(prob, np.float32).reshape(-1)
    if dose.size != prob.size:
        raise ValueError("plan_need: one probability per dose")
    miss = np.maximum(np.float32(target) - dose, np.float32(0))
    return np.where(prob >= np.float32(prob_min), miss, np.float32(0)).astype(np.float32)


def vertex_area(positions, indices) -> np.ndarray:
    """A third of the area [m^2] of the triangles around each vertex of an indexed mesh (positions (n, 3),
    indices (t, 3)), summed in float64 in triangle order: (n,) f32. Meant for weight = area * prob."""
    p = np.asarray(positions, np.float64).reshape(-1, 3)
    t = np.asarray(indices, np.int64).reshape(-1, 3)
    e1, e2 = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    cr = np.cross(e1, e2)
    third = np.sqrt((cr * cr).sum(axis=1)) / 6.0
    out = np.zeros(p.shape[0], np.float64)
    for k in range(3):
        np.add.at(out, t[:, k], third)
    return out.astype(np.float32)
