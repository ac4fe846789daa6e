// view_main.cc -- drives DISINFSystem::query_next_views for the GPU tests (tests/test_gpu_view.py).
//   view_main <dir>
//   <dir>/meta.txt      : voxel trunc nb_bits max_depth W H fx fy cx cy frames
//                         cube (xmin xmax ymin ymax zmin zmax) max_dist clearance_m from_x from_y from_z min_size
//                         yaws pitch view_W view_H view_fx view_fy view_cx view_cy far k
//                         then per frame: qx qy qz qw tx ty tz (cam_T_world)
//   <dir>/depth_<i>.bin : W * H float32 [m], frame i
// The free layer over the cube is enabled before the first frame. Outputs: <dir>/out_views.bin (float32, seven per
// candidate: qx qy qz qw tx ty tz), out_cluster.bin (int32 per candidate), out_seen.bin (uint32, the layer of
// what the chosen views will observe) and on stdout one line: the number of candidates, the number chosen, then
// each chosen index and its gain.
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "disinfect_slam.h"
#include "uv_dose.h"

using namespace disinfect;

template <typename T>
static void write_file(const std::string& p, const std::vector<T>& v) {
  std::ofstream f(p, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  if (!f) throw std::runtime_error("cannot write " + p);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: view_main <dir>\n";
    return 2;
  }
  try {
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt");
    float voxel, trunc, max_depth, fx, fy, cx, cy, clearance_m, pitch, vfx, vfy, vcx, vcy, far;
    int nb_bits, W, H, frames, max_dist, min_size, yaws, vW, vH, k;
    BoundingCube<float> cube;
    std::vector<float> from(3);
    if (!(meta >> voxel >> trunc >> nb_bits >> max_depth >> W >> H >> fx >> fy >> cx >> cy >> frames >> cube.xmin >>
          cube.xmax >> cube.ymin >> cube.ymax >> cube.zmin >> cube.zmax >> max_dist >> clearance_m >> from[0] >> from[1] >>
          from[2] >> min_size >> yaws >> pitch >> vW >> vH >> vfx >> vfy >> vcx >> vcy >> far >> k) ||
        W < 1 || H < 1 || W > 4096 || H > 4096 || vW < 1 || vH < 1 || vW > W || vH > H || frames < 1 || frames > 100)
      throw std::runtime_error("bad meta.txt");
    tsdf_config cfg;
    tsdf_config_default(&cfg);
    cfg.max_width = W;
    cfg.max_height = H;
    cfg.num_block_bits = nb_bits;
    DISINFSystem sys(voxel, trunc, max_depth, CameraIntrinsics<float>(fx, fy, cx, cy), SE3<float>::Identity(), 1000.0f,
                     &cfg, 0);
    sys.enable_free_space(cube);
    Mat rgb(H, W, CV_8UC3);
    std::fill(rgb.data, rgb.data + (size_t)W * H * 3, (uint8_t)0);
    for (int i = 0; i < frames; ++i) {
      float p[7];
      if (!(meta >> p[0] >> p[1] >> p[2] >> p[3] >> p[4] >> p[5] >> p[6])) throw std::runtime_error("bad meta.txt: poses");
      Mat depth(H, W, CV_32FC1);
      std::ifstream df(dir + "/depth_" + std::to_string(i) + ".bin", std::ios::binary);
      df.read(reinterpret_cast<char*>(depth.data), (std::streamsize)((size_t)W * H * 4));
      if (!df) throw std::runtime_error("cannot read a depth file");
      sys.tsdf().Integrate(SE3<float>(p[0], p[1], p[2], p[3], p[4], p[5], p[6]), rgb, depth);
    }
    const CameraParams cam(CameraIntrinsics<float>(vfx, vfy, vcx, vcy), vH, vW);
    const NextViews nv = sys.query_next_views(k, cube, from, cam, far, clearance_m, min_size, yaws, pitch, max_dist);
    std::vector<float> poses;
    for (const SE3<float>& v : nv.views) {
      const Quaternion<float> q = v.GetR();
      for (float c : {q.x, q.y, q.z, q.w, v.GetT()[0], v.GetT()[1], v.GetT()[2]}) poses.push_back(c);
    }
    write_file(dir + "/out_views.bin", poses);
    write_file(dir + "/out_cluster.bin", nv.cluster);
    write_file(dir + "/out_seen.bin", nv.seen.bits);
    std::cout << nv.views.size() << " " << nv.chosen.size();
    for (size_t i = 0; i < nv.chosen.size(); ++i) std::cout << " " << nv.chosen[i] << " " << nv.gains[i];
    std::cout << "\n";
  } catch (const std::exception& ex) {
    std::cerr << "view_main: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
