// track_main.cc -- drives DISINFSystem::track_rgbd_frame for the GPU tests (tests/test_gpu_icp.py).
//   track_main <dir>
//   <dir>/meta.txt      : voxel trunc nb_bits max_depth depth_factor fx fy cx cy width height frames
//                         qx qy qz qw tx ty tz     (intrinsics of the half-size image; width x height
//                         the raw frames' size; the pose registered for the first frame)
//   <dir>/rgb_<i>.bin   : frame i, height x width x 3 u8
//   <dir>/depth_<i>.bin : frame i, height x width u16 (sensor units)
// Output: <dir>/out_poses.bin (7 floats per frame: qx qy qz qw tx ty tz of the registered pose) and
// out_info.txt (per frame: degenerate iterations inliers rmse).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "disinfect_slam.h"

using namespace disinfect;

static std::vector<uint8_t> read_file(const std::string& p, size_t bytes) {
  std::ifstream f(p, std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + p);
  std::vector<uint8_t> v((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (v.size() != bytes) throw std::runtime_error(p + ": unexpected size");
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: track_main <dir>\n";
    return 2;
  }
  try {
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt");
    float voxel, trunc, max_depth, depth_factor, fx, fy, cx, cy, p[7];
    int nb_bits, width, height, frames;
    if (!(meta >> voxel >> trunc >> nb_bits >> max_depth >> depth_factor >> fx >> fy >> cx >> cy >> width >> height >>
          frames))
      throw std::runtime_error("bad meta.txt");
    for (float& v : p)
      if (!(meta >> v)) throw std::runtime_error("bad meta.txt (pose)");
    tsdf_config cfg;
    tsdf_config_default(&cfg);
    cfg.max_width = width / 2;
    cfg.max_height = height / 2;
    cfg.num_block_bits = nb_bits;
    DISINFSystem sys(voxel, trunc, max_depth, CameraIntrinsics<float>(fx, fy, cx, cy), SE3<float>::Identity(),
                     depth_factor, &cfg, 0);
    sys.register_camera_pose(0, SE3<float>(p[0], p[1], p[2], p[3], p[4], p[5], p[6]));
    std::vector<float> poses;
    std::ofstream info(dir + "/out_info.txt");
    for (int i = 0; i < frames; ++i) {
      std::vector<uint8_t> rgb = read_file(dir + "/rgb_" + std::to_string(i) + ".bin", (size_t)width * height * 3);
      std::vector<uint8_t> depth = read_file(dir + "/depth_" + std::to_string(i) + ".bin", (size_t)width * height * 2);
      const TrackResult r = sys.track_rgbd_frame(Mat(height, width, CV_8UC3, rgb.data()),
                                                 Mat(height, width, CV_16UC1, depth.data()), i);
      const SE3<float> reg = sys.query_camera_pose(i);
      const Quaternion<float> q = reg.GetR();
      const float* t = reg.GetT();
      for (float v : {q.x, q.y, q.z, q.w, t[0], t[1], t[2]}) poses.push_back(v);
      info << (r.degenerate ? 1 : 0) << " " << r.iterations << " " << r.inliers << " " << r.rmse << "\n";
    }
    sys.tsdf().Flush();
    std::ofstream f(dir + "/out_poses.bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(poses.data()), (std::streamsize)(poses.size() * sizeof(float)));
    if (!f) throw std::runtime_error("cannot write out_poses.bin");
  } catch (const std::exception& ex) {
    std::cerr << "track_main: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
