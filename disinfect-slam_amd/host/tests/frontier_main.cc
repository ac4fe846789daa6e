// frontier_main.cc -- drives DISINFSystem::query_frontiers for the GPU tests (tests/test_gpu_frontier.py).
//   frontier_main <dir>
//   <dir>/meta.txt   : voxel trunc nb_bits max_dist xmin xmax ymin ymax zmin zmax clearance_m unknown_free
//                      from_x from_y from_z min_size
//   <dir>/blocks.bin : block records (tsdf_pack_blocks; TSDF_BLOCK_RECORD_BYTES each), imported into an
//                      empty volume
// The distance field over the cube (surface sites), the travel field from `from`, then the frontiers reached
// by it. Outputs: <dir>/out_mask.bin (uint8), out_label.bin (uint32), out_clusters.bin (tsdf_component records),
// out_goals.bin (float32, seven per cluster: frontier_goals) and on stdout one line: the box's origin and dims,
// marked, total, the number of clusters.
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "disinfect_slam.h"
#include "uv_dose.h"

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
    std::cerr << "usage: frontier_main <dir>\n";
    return 2;
  }
  try {
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt");
    float voxel, trunc, clearance_m;
    int nb_bits, max_dist, unknown_free, min_size;
    BoundingCube<float> cube;
    std::vector<float> from(3);
    if (!(meta >> voxel >> trunc >> nb_bits >> max_dist >> cube.xmin >> cube.xmax >> cube.ymin >> cube.ymax >>
          cube.zmin >> cube.zmax >> clearance_m >> unknown_free >> from[0] >> from[1] >> from[2] >> min_size))
      throw std::runtime_error("bad meta.txt");
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
    const DistanceField f = sys.query_distance_field(cube, max_dist);
    const TravelField t = sys.query_travel_field(f, from, clearance_m, unknown_free != 0);
    const FrontierSet s = sys.query_frontiers(f, &t, min_size);
    write_file(dir + "/out_mask.bin", s.mask);
    write_file(dir + "/out_label.bin", s.label);
    write_file(dir + "/out_clusters.bin", s.clusters);
    write_file(dir + "/out_goals.bin", frontier_goals(s.clusters, s.origin, s.dims, voxel));
    std::cout << s.origin[0] << " " << s.origin[1] << " " << s.origin[2] << " " << s.dims[0] << " " << s.dims[1] << " "
              << s.dims[2] << " " << s.marked << " " << s.total << " " << s.clusters.size() << "\n";
  } catch (const std::exception& ex) {
    std::cerr << "frontier_main: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
