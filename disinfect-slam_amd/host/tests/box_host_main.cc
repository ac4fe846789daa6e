// box_host_main.cc -- the box calls' contract (csrc/tsdf_box.h) as a stand-alone program for
// tests/test_box_cpu.py: no GPU and no engine library. One command per input line, one answer line each:
//   dims     nx ny nz                  -> box_dims_ok: 0 or 1
//   range    ox oy oz nx ny nz grow    -> box_in_block_range: 0 or 1
//   words    nx ny nz                  -> box_words
//   voxels   nx ny nz                  -> box_voxels
//   tiles    n bits                    -> box_tiles
//   rigid    qx qy qz qw               -> pose_is_rigid of the four floats (hex floats are read): 0 or 1
//   sections k s0 .. s(k-1) [m t0 ..]  -> "total off0 size0 .. off(k-1) size(k-1)" of the k sections; with m
//                                         given, a second answer follows on the same line after "|": the
//                                         layout once the last m sections were declared again with sizes t
//   full                               -> "kMax r total null": add's answer r to one section more than kMax of
//                                         16 bytes each, the total after it, and whether at resolves r to null
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tsdf_box.h"

using namespace tsdf;

static void print_sections(const Sections& L) {
  std::printf("%zu", L.total());
  for (int h = 0; h < L.n; ++h) std::printf(" %zu %zu", L.offset(h), L.size(h));
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    if (!(in >> cmd)) continue;
    std::vector<std::string> a;
    while (in >> tok) a.push_back(tok);
    auto need = [&](size_t k) {
      if (a.size() >= k) return;
      std::fprintf(stderr, "box_host_main: %s needs %zu numbers\n", cmd.c_str(), k);
      std::exit(2);
    };
    auto i32 = [&](size_t k) { return (int32_t)std::strtoll(a[k].c_str(), nullptr, 10); };
    if (cmd == "dims" || cmd == "words" || cmd == "voxels") {
      need(3);
      const int32_t d[3] = {i32(0), i32(1), i32(2)};
      if (cmd == "dims")
        std::printf("%d", box_dims_ok(d) ? 1 : 0);
      else if (cmd == "words")
        std::printf("%lld", (long long)box_words(d));
      else
        std::printf("%zu", box_voxels(d));
    } else if (cmd == "range") {
      need(7);
      const int32_t o[3] = {i32(0), i32(1), i32(2)}, d[3] = {i32(3), i32(4), i32(5)};
      std::printf("%d", box_in_block_range(o, d, i32(6)) ? 1 : 0);
    } else if (cmd == "tiles") {
      need(2);
      std::printf("%d", box_tiles(i32(0), i32(1)));
    } else if (cmd == "rigid") {
      need(4);
      float q[4];
      for (int k = 0; k < 4; ++k) q[k] = std::strtof(a[(size_t)k].c_str(), nullptr);
      std::printf("%d", pose_is_rigid(q) ? 1 : 0);
    } else if (cmd == "full") {
      Sections L;
      for (int h = 0; h < Sections::kMax; ++h) {
        if (L.add(16) != h) return 3;
      }
      const int r = L.add(16);
      unsigned char base[1];
      std::printf("%d %d %zu %d", Sections::kMax, r, L.total(), L.at<uint32_t>(base, r) == nullptr ? 1 : 0);
    } else if (cmd == "sections") {
      need(1);
      const int k = i32(0);
      if (k < 1 || k > Sections::kMax) {
        std::fprintf(stderr, "box_host_main: sections takes 1..%d sizes\n", Sections::kMax);
        return 2;
      }
      need(1 + (size_t)k);
      Sections L;
      for (int h = 0; h < k; ++h) {
        if (L.add((size_t)std::strtoull(a[1 + (size_t)h].c_str(), nullptr, 10)) != h) return 3;
      }
      print_sections(L);
      if (a.size() > 1 + (size_t)k) {
        const int m = i32(1 + (size_t)k);
        if (m < 0 || m > k) return 2;
        need(2 + (size_t)k + (size_t)m);
        L.keep(k - m);
        for (int h = 0; h < m; ++h) L.add((size_t)std::strtoull(a[2 + (size_t)k + (size_t)h].c_str(), nullptr, 10));
        std::printf(" | ");
        print_sections(L);
      }
      // (at resolves a handle against a base: the offset, typed)
      std::vector<unsigned char> buf(L.total() + 1);
      if ((unsigned char*)L.at<uint32_t>(buf.data(), L.n - 1) != buf.data() + L.offset(L.n - 1)) return 3;
    } else {
      std::fprintf(stderr, "box_host_main: unknown command %s\n", cmd.c_str());
      return 2;
    }
    std::printf("\n");
  }
  return 0;
}
