// travel_main.cc -- drives DISINFSystem::query_travel_field and TSDFSystem::TravelPaths for the GPU tests
// (tests/test_gpu_travel.py).
//   travel_main <dir>
//   <dir>/meta.txt   : voxel trunc nb_bits max_dist min_weight unknown xmin xmax ymin ymax zmin zmax
//                      clearance_m unknown_free from_x from_y from_z nt, then nt targets (global voxels x y z)
//   <dir>/blocks.bin : block records (tsdf_pack_blocks; TSDF_BLOCK_RECORD_BYTES each), imported into an
//                      empty volume
// Outputs: <dir>/out_cost.bin (uint32), out_box.txt (origin x y z, dims nx ny nz, seeded, rounds, then the
// cost at the box's first voxel through the accessor) and out_paths.txt (one line per target: its path's
// linear indices, target first).
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "disinfect_slam.h"

using namespace disinfect;

static std::vector<uint8_t> read_file(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + p);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

template <typename T>
static void write_file(const std::string& p, const std::vector<T>& v) {
  std::ofstream f(p, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  if (!f) throw std::runtime_error("cannot write " + p);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: travel_main <dir>\n";
    return 2;
  }
  try {
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt");
    float voxel, trunc, clearance_m;
    int nb_bits, max_dist, min_weight, unknown, unknown_free, nt;
    BoundingCube<float> cube;
    std::vector<float> from(3);
    if (!(meta >> voxel >> trunc >> nb_bits >> max_dist >> min_weight >> unknown >> cube.xmin >> cube.xmax >>
          cube.ymin >> cube.ymax >> cube.zmin >> cube.zmax >> clearance_m >> unknown_free >> from[0] >> from[1] >>
          from[2] >> nt) ||
        nt < 0 || nt > 100000)
      throw std::runtime_error("bad meta.txt");
    std::vector<int32_t> targets(3 * (size_t)nt);
    for (auto& v : targets)
      if (!(meta >> v)) throw std::runtime_error("bad meta.txt: targets");
    tsdf_config cfg;
    tsdf_config_default(&cfg);
    cfg.max_width = 64;
    cfg.max_height = 64;
    cfg.num_block_bits = nb_bits;
    const std::vector<uint8_t> recs = read_file(dir + "/blocks.bin");
    if (recs.size() % TSDF_BLOCK_RECORD_BYTES) throw std::runtime_error("blocks.bin: not whole records");
    DISINFSystem sys(voxel, trunc, 4.0f, CameraIntrinsics<float>(60.0f, 60.0f, 32.0f, 32.0f), SE3<float>::Identity(),
                     1000.0f, &cfg, 0);
    sys.tsdf().ImportBlocks(recs.data(), (int64_t)(recs.size() / TSDF_BLOCK_RECORD_BYTES), true);
    const DistanceField f = sys.query_distance_field(cube, max_dist, min_weight, unknown != 0);
    const TravelField t = sys.query_travel_field(f, from, clearance_m, unknown_free != 0);
    write_file(dir + "/out_cost.bin", t.cost);
    std::ofstream(dir + "/out_box.txt") << t.origin[0] << " " << t.origin[1] << " " << t.origin[2] << " " << t.dims[0]
                                        << " " << t.dims[1] << " " << t.dims[2] << " " << t.seeded << " " << t.rounds
                                        << " " << t.cost[t.at(0, 0, 0)] << "\n";
    std::ofstream paths(dir + "/out_paths.txt");
    for (const std::vector<int32_t>& p : sys.tsdf().TravelPaths(t, targets)) {
      for (int32_t v : p) paths << v << " ";
      paths << "\n";
    }
  } catch (const std::exception& ex) {
    std::cerr << "travel_main: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
