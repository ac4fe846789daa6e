// view_host_main.cc -- drives the view helpers of host/uv_dose.h for tests/test_view_cpu.py: no GPU, no engine
// library. One command per input line, one answer line each:
//   look_at ex ey ez tx ty tz ux uy uz          ->  seven floats: the pose's qx qy qz qw tx ty tz
//   candidates nx ny nz ox oy oz voxel yaws pitch k <k clusters: label size sum_x sum_y sum_z goal goal_key>
//       ->  per pose eight values: the cluster's index, then qx qy qz qw tx ty tz
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "uv_dose.h"

using namespace disinfect;

static void print_pose(const SE3<float>& p) {
  const Quaternion<float> q = p.GetR();
  std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g ", q.x, q.y, q.z, q.w, p.GetT()[0], p.GetT()[1], p.GetT()[2]);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    try {
      if (cmd == "look_at") {
        double e[3], t[3], u[3];
        if (!(in >> e[0] >> e[1] >> e[2] >> t[0] >> t[1] >> t[2] >> u[0] >> u[1] >> u[2]))
          throw std::invalid_argument("look_at: too few values");
        print_pose(look_at_pose(e, t, u));
        std::printf("\n");
      } else if (cmd == "candidates") {
        int32_t dims[3], origin[3];
        float voxel, pitch;
        int yaws;
        long k;
        if (!(in >> dims[0] >> dims[1] >> dims[2] >> origin[0] >> origin[1] >> origin[2] >> voxel >> yaws >> pitch >> k) ||
            k < 0 || k > 1000000)
          throw std::invalid_argument("candidates: too few values");
        std::vector<tsdf_component> clusters((size_t)k);
        for (tsdf_component& c : clusters) {
          c = tsdf_component{};
          long long s[3];
          in >> c.label >> c.size >> s[0] >> s[1] >> s[2] >> c.goal >> c.goal_key;
          for (int a = 0; a < 3; ++a) c.sum[a] = s[a];
        }
        if (!in) throw std::invalid_argument("candidates: too few values");
        std::vector<int32_t> owner;
        const std::vector<SE3<float>> views = view_candidates(clusters, origin, dims, voxel, yaws, pitch, &owner);
        for (size_t i = 0; i < views.size(); ++i) {
          std::printf("%d ", owner[i]);
          print_pose(views[i]);
        }
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
