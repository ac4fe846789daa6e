// uv_host_main.cc -- drives host/uv_dose.h for tests/test_uv_cpu.py: no GPU, no engine library.
// One command per input line, one answer line each:
//   tube x0 y0 z0 x1 y1 z1 power dwell segments  ->  x y z energy of every emitter
//   carry nold nnew <4 nold old keys> <nold old doses> <4 nnew new keys>  ->  nnew doses
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "uv_dose.h"

using namespace disinfect;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    try {
      if (cmd == "tube") {
        float p0[3], p1[3], power, dwell;
        int segments;
        if (!(in >> p0[0] >> p0[1] >> p0[2] >> p1[0] >> p1[1] >> p1[2] >> power >> dwell >> segments))
          throw std::invalid_argument("tube: 9 values");
        for (const UVEmitter& e : tube_emitters(p0, p1, power, dwell, segments))
          std::printf("%.9g %.9g %.9g %.9g ", e.x, e.y, e.z, e.energy);
        std::printf("\n");
      } else if (cmd == "carry") {
        long nold, nnew;
        if (!(in >> nold >> nnew) || nold < 0 || nnew < 0 || nold > 1000000 || nnew > 1000000)
          throw std::invalid_argument("carry: counts");
        std::vector<int32_t> ok((size_t)nold * 4), nk((size_t)nnew * 4);
        std::vector<float> od((size_t)nold);
        for (auto& v : ok) in >> v;
        for (auto& v : od) in >> v;
        for (auto& v : nk) in >> v;
        if (!in) throw std::invalid_argument("carry: too few values");
        for (float d : carry_dose(ok, od, nk)) std::printf("%.9g ", d);
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
