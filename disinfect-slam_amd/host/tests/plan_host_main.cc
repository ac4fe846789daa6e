// plan_host_main.cc -- drives the lamp-stop planner's helpers of host/uv_dose.h for tests/test_plan_cpu.py:
// no GPU, no engine library. One command per input line, one answer line each:
//   candidates nc <3 nc centres> ax ay az length power dwell segments
//       ->  x y z energy of every emitter, the word "first", the nc + 1 offsets
//   need n target prob_min <n doses> <n probabilities>  ->  n values
//   area nv nt <3 nv vertex coordinates> <3 nt indices>  ->  nv areas
//   standoff nx ny nz ox oy oz voxel lo hi stride <nx ny nz squared distances> <as many states>
//       ->  x y z of every position
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

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    try {
      if (cmd == "candidates") {
        std::vector<float> centres(3 * count(in, 100000));
        for (auto& v : centres) in >> v;
        float axis[3], length, power, dwell;
        int segments;
        if (!(in >> axis[0] >> axis[1] >> axis[2] >> length >> power >> dwell >> segments))
          throw std::invalid_argument("candidates: too few values");
        const LampCandidates c = tube_candidates(centres, axis, length, power, dwell, segments);
        for (const UVEmitter& e : c.emitters) std::printf("%.9g %.9g %.9g %.9g ", e.x, e.y, e.z, e.energy);
        std::printf("first");
        for (int32_t f : c.first) std::printf(" %d", f);
        std::printf("\n");
      } else if (cmd == "need") {
        const size_t n = count(in, 1000000);
        float target, prob_min;
        in >> target >> prob_min;
        std::vector<float> dose(n), prob(n);
        for (auto& v : dose) in >> v;
        for (auto& v : prob) in >> v;
        if (!in) throw std::invalid_argument("need: too few values");
        for (float v : plan_need(dose, prob, target, prob_min)) std::printf("%.9g ", v);
        std::printf("\n");
      } else if (cmd == "area") {
        const size_t nv = count(in, 1000000), nt = count(in, 1000000);
        std::vector<float> verts(3 * nv);
        std::vector<int32_t> tris(3 * nt);
        for (auto& v : verts) in >> v;
        for (auto& v : tris) in >> v;
        if (!in) throw std::invalid_argument("area: too few values");
        for (float v : vertex_area(verts, tris)) std::printf("%.9g ", v);
        std::printf("\n");
      } else if (cmd == "standoff") {
        int32_t dims[3], origin[3];
        float voxel, lo, hi;
        int stride;
        if (!(in >> dims[0] >> dims[1] >> dims[2] >> origin[0] >> origin[1] >> origin[2] >> voxel >> lo >> hi >> stride))
          throw std::invalid_argument("standoff: too few values");
        for (int a = 0; a < 3; ++a)
          if (dims[a] < 0 || dims[a] > 256) throw std::invalid_argument("standoff: dims");
        const size_t n = (size_t)dims[0] * dims[1] * dims[2];
        std::vector<uint16_t> d2(n);
        std::vector<uint8_t> state(n);
        for (auto& v : d2) in >> v;
        for (auto& v : state) {
          int s;
          in >> s;
          v = (uint8_t)s;
        }
        if (!in) throw std::invalid_argument("standoff: too few values");
        for (float v : standoff_candidates(d2, state, origin, dims, voxel, lo, hi, stride)) std::printf("%.9g ", v);
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
