"""Occupancy of the pipelined frame kernels, from the built library's code-object metadata (CPU only).

k_frame and k_frame_g are built for 7 waves per SIMD (TSDF_FRAME_WAVES, csrc/tsdf_fuse.hip): 512 VGPRs per
SIMD lane / 7 = 73, allocated in units of 8, so at most 72 VGPRs; one workgroup is 4 waves, one per SIMD,
so 7 workgroups share a CU and 160 KiB of LDS -- at most 160 KiB / 7 each. The record loop must reach
that without more scratch than it had at 6 waves (8 B: a spilled loop is what made 7 and 8 waves slower in
rounds 5 and 6, DESIGN.md 4 "Round 11").

Only register counts and segment sizes are read (llvm-readobj --notes); no instruction is inspected.
"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "disinfect-slam_amd", "libdisinfect_tsdf.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

FRAME_WAVES = 7
MAX_VGPRS = 72                       # 512 / 7 = 73, in allocation units of 8
MAX_PRIVATE = 8                      # bytes: the parent's k_frame at 6 waves
MAX_LDS = 160 * 1024 // FRAME_WAVES  # bytes per workgroup


FIELDS = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "wavefront_size",
          "max_flat_workgroup_size")


def _kernel_entries(notes):
    """{kernel name: {field: int}} from the metadata note as llvm-readobj prints it: one entry per item of the
    `amdhsa.kernels` list. An item begins with `  - .` at the list's own indent (its arguments' items are nested
    deeper), its own keys stand at four spaces, and its `.name` is in the middle of them (the keys are sorted), so
    an entry is cut at the item boundaries, never at `.name`."""
    out, lines = {}, notes.splitlines()
    i = 0
    while i < len(lines):
        if lines[i].strip() != "amdhsa.kernels:":
            i += 1
            continue
        i += 1
        entry = None
        while i < len(lines) and (lines[i].startswith("  ") or not lines[i].strip()):
            line = lines[i]
            if line.startswith("  - ."):
                entry = {}
                out[id(entry)] = entry
                line = "    " + line[4:]
            m = re.match(r"^    \.(\w+):\s+(\S+)\s*$", line)
            if m and entry is not None:
                entry[m.group(1)] = m.group(2)
            i += 1
    named = {}
    for e in out.values():
        assert "name" in e and e["name"] not in named, e
        assert all(f in e for f in FIELDS), e
        named[e["name"]] = {k: int(v) for k, v in e.items() if v.isdigit()}
    return named


def _metadata():
    """{kernel symbol: {field: int}} of every gfx950 kernel in the library."""
    assert os.path.exists(LIB), f"{LIB} is not built"
    if not os.path.exists(os.path.join(LLVM, "llvm-readobj")):
        pytest.skip("llvm tools absent")
    tmp = tempfile.mkdtemp()
    try:
        fb = os.path.join(tmp, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", LIB,
                               os.path.join(tmp, "copy.so")])
        data = open(fb, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        out = {}
        for i, st in enumerate(starts):
            part = os.path.join(tmp, f"b{i}")
            with open(part, "wb") as f:
                f.write(data[st:starts[i + 1] if i + 1 < len(starts) else len(data)])
            co = part + ".co"
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                                   f"--input={part}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   f"--output={co}"])
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readobj"), "--notes", co], text=True)
            out.update(_kernel_entries(notes))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.fixture(scope="module")
def frame_kernels():
    md = _metadata()
    found = {k: next((v for n, v in md.items() if n.startswith(p)), None)
             for k, p in (("k_frame", "_ZN4tsdf7k_frameE"), ("k_frame_g", "_ZN4tsdf9k_frame_gE"))}
    assert all(found.values()), sorted(md)[:20]
    return found


@pytest.mark.parametrize("kernel", ["k_frame", "k_frame_g"])
def test_frame_kernel_fits_seven_waves(frame_kernels, kernel):
    m = frame_kernels[kernel]
    print(kernel, {k: m.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
    assert m["vgpr_count"] + m.get("agpr_count", 0) <= MAX_VGPRS, m
    assert m["private_segment_fixed_size"] <= MAX_PRIVATE, m
    assert m["group_segment_fixed_size"] <= MAX_LDS, m
    assert m["wavefront_size"] == 64 and m["max_flat_workgroup_size"] == 256, m
