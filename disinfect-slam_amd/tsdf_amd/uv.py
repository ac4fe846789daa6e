"""The lamp model and the dose bookkeeping around Engine.uv_dose (DESIGN.md "UV dose"), numpy only:
a tube lamp as point emitters, the dose of a re-extracted mesh carried over by vertex key, and the
coverage of the high-touch surface. host/uv_dose.h is the same in C++."""
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
