// track_solve_main.cc -- the tracker's host math (csrc/tsdf_track_host.h) as a stand-alone program
// for tests/test_track_host_cpu.py: no GPU and no engine library. One command per input line, one
// line of %.17g numbers per answer:
//   solve  u0 .. u20 r0 .. r5              -> "ok x0 .. x5" or "singular" (A x = r, A's upper triangle)
//   exp    w0 w1 w2                        -> the 9 entries of exp([w]x), row-major
//   update qx qy qz qw tx ty tz xi0 .. xi5 -> R_wc (9) p_wc (3) after the update, then the rounded
//                                             float pose qx qy qz qw tx ty tz
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "tsdf_track_host.h"

static void print(const double* v, int n) {
  for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    double a[27];
    const int need = cmd == "solve" ? 27 : cmd == "exp" ? 3 : cmd == "update" ? 13 : -1;
    if (need < 0) {
      std::fprintf(stderr, "track_solve_main: unknown command %s\n", cmd.c_str());
      return 2;
    }
    for (int i = 0; i < need; ++i) {  // (strtod: it reads "nan" and "inf", operator>> does not)
      std::string tok;
      char* end = nullptr;
      if (in >> tok) a[i] = std::strtod(tok.c_str(), &end);
      if (!end || end == tok.c_str() || *end) {
        std::fprintf(stderr, "track_solve_main: %s needs %d numbers\n", cmd.c_str(), need);
        return 2;
      }
    }
    if (cmd == "solve") {
      double x[6] = {};
      if (track_host::solve_spd6(a, a + 21, x)) {
        std::printf("ok");
        print(x, 6);
      } else {
        std::printf("singular");
      }
    } else if (cmd == "exp") {
      double R[9];
      track_host::so3_exp(a, R);
      print(R, 9);
    } else {
      float q[4], t[3], q2[4], t2[3];
      for (int i = 0; i < 4; ++i) q[i] = (float)a[i];
      for (int i = 0; i < 3; ++i) t[i] = (float)a[4 + i];
      double R_wc[9], p_wc[3];
      track_host::pose_to_world(q, t, R_wc, p_wc);
      track_host::apply_twist(a + 7, R_wc, p_wc);
      track_host::world_to_pose(R_wc, p_wc, q2, t2);
      print(R_wc, 9);
      print(p_wc, 3);
      for (float v : q2) std::printf(" %.9g", (double)v);
      for (float v : t2) std::printf(" %.9g", (double)v);
    }
    std::printf("\n");
  }
  return 0;
}
