"""The box calls' contract (csrc/tsdf_box.h) through the stand-alone box_host_main, against the same rules
written here: the limits, the block-range test with its grow, the counters, the rigid-pose rule and the
carve-up of a scratch buffer into sections. No GPU, no engine library."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "disinfect-slam_amd", "box_host_main")

MAX_DIM, MAX_VOXELS = 2048, 1 << 28


def run(lines):
    """One answer line per command line."""
    text = "".join(" ".join(str(v) for v in ln) + "\n" for ln in lines)
    r = subprocess.run([BIN], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def dims_ok(d):
    return all(1 <= v <= MAX_DIM for v in d) and d[0] * d[1] * d[2] <= MAX_VOXELS


def in_block_range(o, d, grow):
    return all((o[a] - grow) >> 3 >= -32768 and (o[a] + d[a] - 1 + grow) >> 3 <= 32767 for a in range(3))


def up16(b):
    return (b + 15) // 16 * 16


def test_limits_mirror_the_public_header_and_the_python_layer():
    text = open(os.path.join(ROOT, "include", "disinfect_tsdf.h")).read()
    assert "#define TSDF_BOX_MAX_DIM 2048\n" in text
    assert "#define TSDF_BOX_MAX_VOXELS ((int64_t)1 << 28)\n" in text
    from tsdf_amd import _lib
    assert (_lib.TSDF_BOX_MAX_DIM, _lib.TSDF_BOX_MAX_VOXELS) == (MAX_DIM, MAX_VOXELS)


def test_dims():
    cases = [(v, 3, 5)[k:] + (v, 3, 5)[:k] for v in (0, 1, 2048, 2049, -1, -2048) for k in range(3)]
    cases += [(2048, 2048, 64), (2048, 2048, 65), (64, 2048, 2048), (65, 2048, 2048), (1, 1, 1), (2048, 1, 1),
              (-2, -2, 4), (645, 645, 645), (646, 646, 644)]
    got = run([("dims", *d) for d in cases])
    for d, g in zip(cases, got):
        assert int(g) == int(dims_ok(d)), d
    assert dims_ok((2048, 2048, 64)) and not dims_ok((2048, 2048, 65))
    got = run([("voxels", *d) for d in ((1, 1, 1), (33, 9, 5), (2048, 2048, 64))])
    assert [int(g) for g in got] == [1, 33 * 9 * 5, 1 << 28]


def test_block_range_and_grow():
    lo, last = -32768 * 8, 32767 * 8 + 7
    cases = []
    for axis in range(3):
        def box(o, n):
            oo, dd = [0, 0, 0], [3, 4, 5]
            oo[axis], dd[axis] = o, n
            return oo, dd
        cases += [(*box(lo, 9), 0, True), (*box(lo, 9), 1, False), (*box(lo + 1, 9), 1, True),
                  (*box(last - 8, 9), 0, True), (*box(last - 8, 9), 1, False), (*box(last - 9, 9), 1, True),
                  (*box(lo - 1, 9), 0, False), (*box(last - 7, 9), 0, False), (*box(last, 1), 0, True),
                  (*box(last + 1, 1), 0, False), (*box(lo, 1), 0, True), (*box(-4, 9), 1, True)]
    got = run([("range", *o, *d, g) for o, d, g, _ in cases])
    for (o, d, g, want), ans in zip(cases, got):
        assert in_block_range(o, d, g) == want, (o, d, g)
        assert int(ans) == int(want), (o, d, g)


def test_words_and_tiles():
    for nx, wx in ((1, 1), (32, 1), (33, 2), (2048, 64)):
        a, b = run([("words", nx, 7, 3), ("words", nx, 1, 1)])
        assert (int(a), int(b)) == (3 * 7 * wx, wx)
    ns = (1, 7, 8, 9, 16, 17, 2048)
    got = run([("tiles", n, 3) for n in ns] + [("tiles", n, 5) for n in ns])
    assert [int(g) for g in got] == [-(-n // 8) for n in ns] + [-(-n // 32) for n in ns]


def test_rigid_pose():
    """|n^2 - 1| <= 2^-10 in double over the float components: just inside, just outside, and no pose at all."""
    def want(q):
        q = np.asarray(q, np.float32).astype(np.float64)
        return abs(float(q @ q) - 1.0) <= 2.0 ** -10
    qs = [(0, 0, 0, 1), (0, 0, 0, 0), (1, 0, 0, 0), (0.5, 0.5, 0.5, 0.5), (0, 0, 0, 2), (0, 0.6, 0, 0.8)]
    for s2, inside in ((1 + 2.0 ** -10, True), (1 - 2.0 ** -10, True), (1 + 2.0 ** -10 + 2.0 ** -20, False),
                       (1 - 2.0 ** -10 - 2.0 ** -20, False)):
        w = np.float32(np.sqrt(s2))
        # the float nearest the root may land on either side: step it until its square is on the side meant
        for _ in range(4):
            if want((0, 0, 0, w)) == inside:
                break
            w = np.nextafter(w, np.float32(1 if inside else (4 if s2 > 1 else 0)))
        assert want((0, 0, 0, w)) == inside
        qs += [(0, 0, 0, w), (w, 0, 0, 0)]
    qs += [(float("nan"), 0, 0, 1), (float("inf"), 0, 0, 0)]
    got = run([("rigid", *(float(np.float32(v)).hex() for v in q)) for q in qs])
    for q, g in zip(qs, got):
        assert int(g) == int(want(q)), q
    assert [int(g) for g in got[:3]] == [1, 0, 1]


def test_sections_refuse_one_too_many():
    """A section past kMax is refused: nothing is written, the total stays, and its handle resolves to null."""
    kmax, r, total, null = (int(v) for v in run([("full",)])[0].split())
    assert kmax >= 8 and r == -1 and total == 16 * kmax and null == 1


def test_sections():
    rng = np.random.default_rng(11)
    cases = []
    for i in range(400):
        k = int(rng.integers(1, 8))
        sizes = [int(v) for v in rng.integers(0, 4097, k)]
        for h in range(k):
            if rng.random() < 0.25:
                sizes[h] = 0
        m = int(rng.integers(0, k + 1))
        tail = [int(v) for v in rng.integers(0, 4097, m)]
        cases.append((sizes, tail))
    cases += [([0], []), ([0, 0, 0, 0, 0, 0, 0], [0, 5]), ([1] * 7, []), ([4096] * 7, [1]), ([15, 16, 17], [])]
    got = run([("sections", len(s), *s, len(t), *t) for s, t in cases])

    def check(words, sizes):
        total, rest = int(words[0]), [int(v) for v in words[1:]]
        offs, szs = rest[0::2], rest[1::2]
        assert len(offs) == len(sizes)
        assert offs[0] == 0
        assert all(o % 16 == 0 for o in offs)
        assert szs == [up16(b) for b in sizes]
        # contiguous in declaration order, so nothing overlaps; a zero-size section sits at the next one's offset
        ends = offs[1:] + [total]
        assert all(o + z == e for o, z, e in zip(offs, szs, ends))
        assert all(e == o for o, b, e in zip(offs, sizes, ends) if b == 0)
        assert total == sum(up16(b) for b in sizes)
        return offs

    for (sizes, tail), line in zip(cases, got):
        first, second = line.split("|")
        o1 = check(first.split(), sizes)
        keep = len(sizes) - len(tail)
        o2 = check(second.split(), sizes[:keep] + tail)
        # trailing sizes changed: the leading offsets stay, the first changed section's included
        assert o2[:keep + 1] == o1[:keep + 1]
