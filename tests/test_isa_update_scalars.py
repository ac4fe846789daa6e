"""Codegen pins of the voxel update's scalar side. An update wave issues at most
one instruction every ~4 cycles whatever its kind, so what the loop does beside the update itself
lengthens the launch's critical path: a kernel argument re-loaded inside the loop is a scalar memory
round trip per record (waited for in the middle of pass 2), and a scalar register spilled to a VGPR lane
is read back with v_readlane_b32 plus hazard s_nops. Round 9 collects the update's constants once
before the record loop (UpdConst, each through uniform_reg) and reads the kernels' arguments in place
(kernel_args), so that no part's arguments are live across another part's loop.

The loops are recognised as tests/test_isa.py recognises them (a backward branch whose body, fewer than
4,000 instructions, has three 16-B pool loads and the reciprocal estimate); the helpers are copies of
that file's. CPU only (llvm-objdump on the built library)."""
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

KERNELS = ("_ZN4tsdf7k_frame", "_ZN4tsdf9k_frame_g", "_ZN4tsdf13k_integrate_t", "_ZN4tsdf14k_integrate_vg")


def _disassemble(lib):
    if not os.path.exists(lib) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("library or llvm tools absent")
    tmp = tempfile.mkdtemp()
    try:
        fb = os.path.join(tmp, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", lib,
                               os.path.join(tmp, "copy.so")])
        data = open(fb, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        text = []
        for i, st in enumerate(starts):
            part = os.path.join(tmp, f"b{i}")
            with open(part, "wb") as f:
                f.write(data[st:starts[i + 1] if i + 1 < len(starts) else len(data)])
            co = part + ".co"
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                                   f"--input={part}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   f"--output={co}"])
            text.append(subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True))
        return "\n".join(text)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _functions(asm):
    funcs, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            name = m.group(1)
            funcs[name] = []
        elif name and line.startswith("\t"):
            funcs[name].append(line.strip())
    return funcs


def _loops(body):
    """(first, last) instruction indices of every backward branch's loop body."""
    addrs = []
    for x in body:
        m = re.search(r"// ([0-9A-F]+):", x)
        addrs.append(int(m.group(1), 16) if m else None)
    base = addrs[0]
    idx = {a: i for i, a in enumerate(addrs) if a is not None}
    for i, x in enumerate(body):
        if re.match(r"s_cbranch_\w+|s_branch", x):
            t = re.search(r"<\S+\+0x([0-9a-f]+)>", x)
            j = idx.get(base + int(t.group(1), 16)) if t and base is not None else None
            if j is not None and j < i:
                yield j, i


def update_loops(lib=LIB):
    """{function name: [the opcodes of each of its update loops]} for the frame kernels of lib."""
    out = {}
    for name, body in _functions(_disassemble(lib)).items():
        if not name.startswith(KERNELS):
            continue
        for j, i in _loops(body):
            ops = [x.split()[0] for x in body[j:i + 1]]
            if i - j < 4000 and ops.count("global_load_dwordx4") >= 3 and "v_rcp_f32_e32" in ops:
                out.setdefault(name, []).append(ops)
    return out


@pytest.fixture(scope="module")
def loops():
    found = update_loops()
    seen = {k for k in KERNELS for name in found if name.startswith(k)}
    assert seen == set(KERNELS), seen
    return found


def test_update_loops_load_no_kernel_arguments(loops):
    """No s_load_dword* inside any update loop of k_frame, k_frame_g, k_integrate_t (four forms) and
    k_integrate_vg -- the record loop itself and the loops around it (k_frame's collection, the pair
    loop's candidate path). The parent's k_frame re-loaded its arguments 4 times per record (two
    s_load_dwordx8, two s_load_dwordx16, each waited for with lgkmcnt(0)) and 6-7 times in the
    enclosing loops."""
    for name, bodies in loops.items():
        for ops in bodies:
            loads = [o for o in ops if o.startswith(("s_load_dword", "s_buffer_load_dword"))]
            assert not loads, (name, len(ops), loads)


# v_readlane_b32 per loop at most: the count this change reaches + 4 for compiler drift. Four of each
# count are wave_min_u's (the carve minimum's reduction), not spill reloads.
READLANE_CAP = (
    ("_ZN4tsdf7k_frame", 26),               # reached: 4 in the record loop, 22 with the collection around it
    ("_ZN4tsdf9k_frame_g", 26),             # 4 / 22
    ("_ZN4tsdf13k_integrate_tILb0ELb0", 16),  # 8 / 12
    ("_ZN4tsdf13k_integrate_tILb1ELb0", 16),  # 8 / 12
    ("_ZN4tsdf13k_integrate_tILb0ELb1", 34),  # the Raw (shard) forms: 26 / 30
    ("_ZN4tsdf13k_integrate_tILb1ELb1", 34),
    ("_ZN4tsdf14k_integrate_vg", 16),       # 8 / 12
)


def test_update_loops_reload_few_spilled_scalars(loops):
    """v_readlane_b32 in the update loops (SGPR-spill reloads plus wave_min_u's four), counted in the
    gfx950 code of the built library, smallest (the record loop) .. largest (with the enclosing loops)
    recognised loop of each kernel:

                              parent commit's library    this change
      k_frame                       15 .. 38                4 .. 22
      k_frame_g                     55 .. 99                4 .. 22
      k_integrate_t<., false>       44 .. 60                8 .. 12
      k_integrate_t<., true>        64 .. 81               26 .. 30
      k_integrate_vg                46 .. 62                8 .. 12

    (SGPR spills: k_frame 269 -> 154, k_frame_g 280 -> 160, k_integrate_t 76-94 -> 39-54.)"""
    for name, bodies in loops.items():
        cap = next(v for k, v in READLANE_CAP if name.startswith(k))
        for ops in bodies:
            assert ops.count("v_readlane_b32") <= cap, (name, len(ops), ops.count("v_readlane_b32"))
