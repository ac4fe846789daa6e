// frontier_host_main.cc -- drives the frontier helper of host/uv_dose.h for tests/test_frontier_cpu.py: no GPU,
// no engine library. One command per input line, one answer line each:
//   goals nx ny nz ox oy oz voxel k <k clusters: label size sum_x sum_y sum_z goal goal_key>
//       ->  seven floats per cluster: goal x y z, centroid x y z, metres
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
      if (cmd == "goals") {
        int32_t dims[3], origin[3];
        float voxel;
        long k;
        if (!(in >> dims[0] >> dims[1] >> dims[2] >> origin[0] >> origin[1] >> origin[2] >> voxel >> k) || k < 0 ||
            k > 1000000)
          throw std::invalid_argument("goals: too few values");
        std::vector<tsdf_component> clusters((size_t)k);
        for (tsdf_component& c : clusters) {
          c = tsdf_component{};
          long long s[3];
          in >> c.label >> c.size >> s[0] >> s[1] >> s[2] >> c.goal >> c.goal_key;
          for (int a = 0; a < 3; ++a) c.sum[a] = s[a];
        }
        if (!in) throw std::invalid_argument("goals: too few values");
        for (float v : frontier_goals(clusters, origin, dims, voxel)) std::printf("%.9g ", v);
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
