// travel_host_main.cc -- drives the travel field's helpers of host/uv_dose.h for tests/test_travel_cpu.py: no
// GPU, no engine library. One command per input line, one answer line each:
//   voxel n voxel sample_offset <n coordinates>  ->  n nearest voxels
//   metres n voxel <n costs>  ->  n distances
//   reachable nx ny nz ox oy oz voxel max_travel sample_offset np <3 np coordinates> <nx ny nz costs>
//       ->  x y z travel of every kept position
// (max_travel "inf" for none)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "uv_dose.h"

using namespace disinfect;

static size_t count(std::istream& in, long most) {
  long n;
  if (!(in >> n) || n < 0 || n > most) throw std::invalid_argument("a count is missing or out of range");
  return (size_t)n;
}

static float number(std::istream& in) {
  std::string w;
  if (!(in >> w)) throw std::invalid_argument("a number is missing");
  return w == "inf" ? INFINITY : std::stof(w);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    try {
      if (cmd == "voxel") {
        const size_t n = count(in, 1000000);
        const float voxel = number(in), offset = number(in);
        for (size_t i = 0; i < n; ++i) std::printf("%d ", nearest_voxel(number(in), voxel, offset));
        std::printf("\n");
      } else if (cmd == "metres") {
        std::vector<uint32_t> cost(count(in, 1000000));
        const float voxel = number(in);
        for (auto& v : cost) in >> v;
        if (!in) throw std::invalid_argument("metres: too few values");
        for (float v : travel_metres(cost, voxel)) std::printf("%.9g ", v);
        std::printf("\n");
      } else if (cmd == "reachable") {
        int32_t dims[3], origin[3];
        if (!(in >> dims[0] >> dims[1] >> dims[2] >> origin[0] >> origin[1] >> origin[2]))
          throw std::invalid_argument("reachable: too few values");
        for (int a = 0; a < 3; ++a)
          if (dims[a] < 0 || dims[a] > 256) throw std::invalid_argument("reachable: dims");
        const float voxel = number(in), max_travel = number(in), offset = number(in);
        std::vector<float> pos(3 * count(in, 1000000));
        for (auto& v : pos) v = number(in);
        std::vector<uint32_t> cost((size_t)dims[0] * dims[1] * dims[2]);
        for (auto& v : cost) in >> v;
        if (!in) throw std::invalid_argument("reachable: too few values");
        std::vector<float> travel;
        const std::vector<float> kept = reachable_candidates(pos, cost, origin, dims, voxel, max_travel, offset, &travel);
        for (size_t k = 0; k < travel.size(); ++k)
          std::printf("%.9g %.9g %.9g %.9g ", kept[3 * k], kept[3 * k + 1], kept[3 * k + 2], travel[k]);
        std::printf("\n");
      } else {
        throw std::invalid_argument("unknown command " + cmd);
      }
    } catch (const std::exception& ex) {
      std::printf("error %s\n", ex.what());
    }
  }
  return 0;
}
