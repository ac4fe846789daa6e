"""Codegen pin of the update's write-back: in the record loops of k_frame, k_frame_g
and the four k_integrate_t a lane stores its three 16-B vectors (tsdf, probability, rgbw) in one exec
region, and the per-word form -- 4-B and 8-B pool stores under each voxel's own mask -- is gone from them
(C5's k_integrate_vg keeps it, where it measured faster, and is not pinned here). The loops are
recognised as tests/test_isa_update_scalars.py recognises them (its helper is used). CPU only
(llvm-objdump on the built library)."""
import pytest

from test_isa_update_scalars import update_loops

FRAME = ("_ZN4tsdf7k_frame", "_ZN4tsdf9k_frame_g", "_ZN4tsdf13k_integrate_t")


@pytest.fixture(scope="module")
def frame_loops():
    found = {name: ls for name, ls in update_loops().items() if name.startswith(FRAME)}
    assert {k for k in FRAME for name in found if name.startswith(k)} == set(FRAME), sorted(found)
    return found


def test_frame_update_loops_store_three_vectors_and_no_words(frame_loops):
    assert len(frame_loops) == 6, sorted(frame_loops)  # k_frame, k_frame_g, four k_integrate_t
    for name, ls in frame_loops.items():
        ops = min(ls, key=len)  # the record loop (the loops around it contain it)
        stores = {o: ops.count(o) for o in set(ops) if o.startswith("global_store")}
        assert stores == {"global_store_dwordx4": 3}, (name, stores)
