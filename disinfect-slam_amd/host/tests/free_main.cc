// free_main.cc -- drives DISINFSystem::enable_free_space, frames, query_free_space and query_travel_field for
// the GPU tests (tests/test_gpu_free.py).
//   free_main <dir>
//   <dir>/meta.txt  : voxel trunc nb_bits max_depth W H fx fy cx cy frames
//                     layer cube (xmin xmax ymin ymax zmin zmax) field cube (the same six) max_dist
//                     clearance_m from_x from_y from_z
//   <dir>/depth.bin : W * H float32 [m], integrated `frames` times from the identity pose
// One frame goes in before enable_free_space and the rest after it, so the layer counts frames - 1.
// Outputs: <dir>/out_state.bin (uint8, the promoted state), out_cost.bin (uint32, the travel field with
// unknown_free = false over the promoted field), out_bits.bin (uint32, the layer's words), and on stdout one
// line: the field's origin and dims, layer frames, bits set, promoted, seeded without the layer, seeded and
// voxels reached with it.
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "disinfect_slam.h"

using namespace disinfect;

template <typename T>
static void write_file(const std::string& p, const std::vector<T>& v) {
  std::ofstream f(p, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  if (!f) throw std::runtime_error("cannot write " + p);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: free_main <dir>\n";
    return 2;
  }
  try {
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt");
    float voxel, trunc, max_depth, fx, fy, cx, cy, clearance_m;
    int nb_bits, W, H, frames, max_dist;
    BoundingCube<float> lc, fc;
    std::vector<float> from(3);
    if (!(meta >> voxel >> trunc >> nb_bits >> max_depth >> W >> H >> fx >> fy >> cx >> cy >> frames >> lc.xmin >>
          lc.xmax >> lc.ymin >> lc.ymax >> lc.zmin >> lc.zmax >> fc.xmin >> fc.xmax >> fc.ymin >> fc.ymax >> fc.zmin >>
          fc.zmax >> max_dist >> clearance_m >> from[0] >> from[1] >> from[2]) ||
        W < 1 || H < 1 || W > 4096 || H > 4096 || frames < 2 || frames > 100)
      throw std::runtime_error("bad meta.txt");
    Mat depth(H, W, CV_32FC1), rgb(H, W, CV_8UC3);
    std::ifstream df(dir + "/depth.bin", std::ios::binary);
    df.read(reinterpret_cast<char*>(depth.data), (std::streamsize)((size_t)W * H * 4));
    if (!df) throw std::runtime_error("cannot read depth.bin");
    std::fill(rgb.data, rgb.data + (size_t)W * H * 3, (uint8_t)0);
    tsdf_config cfg;
    tsdf_config_default(&cfg);
    cfg.max_width = W;
    cfg.max_height = H;
    cfg.num_block_bits = nb_bits;
    DISINFSystem sys(voxel, trunc, max_depth, CameraIntrinsics<float>(fx, fy, cx, cy), SE3<float>::Identity(), 1000.0f,
                     &cfg, 0);
    sys.tsdf().Integrate(SE3<float>::Identity(), rgb, depth);
    sys.enable_free_space(lc);
    for (int k = 1; k < frames; ++k) sys.tsdf().Integrate(SE3<float>::Identity(), rgb, depth);
    const DistanceField f = sys.query_distance_field(fc, max_dist);
    const TravelField before = sys.query_travel_field(f, from, clearance_m, false);
    int64_t promoted = -1;
    const DistanceField p = sys.query_free_space(f, &promoted);
    const TravelField t = sys.query_travel_field(p, from, clearance_m, false);
    const FreeLayer layer = sys.tsdf().FreeSpace();
    int64_t reached = 0;
    for (uint32_t c : t.cost) reached += c != TSDF_TRAVEL_UNREACHED;
    write_file(dir + "/out_state.bin", p.state);
    write_file(dir + "/out_cost.bin", t.cost);
    write_file(dir + "/out_bits.bin", layer.bits);
    std::cout << f.origin[0] << " " << f.origin[1] << " " << f.origin[2] << " " << f.dims[0] << " " << f.dims[1] << " "
              << f.dims[2] << " " << layer.frames << " " << layer.count() << " " << promoted << " " << before.seeded
              << " " << t.seeded << " " << reached << "\n";
  } catch (const std::exception& ex) {
    std::cerr << "free_main: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
