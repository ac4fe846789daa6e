// edt_main.cc -- drives DISINFSystem::query_distance_field for the GPU tests (tests/test_gpu_edt.py).
//   edt_main <dir>
//   <dir>/meta.txt   : voxel trunc nb_bits max_dist min_weight unknown xmin xmax ymin ymax zmin zmax
//   <dir>/blocks.bin : block records (tsdf_pack_blocks; TSDF_BLOCK_RECORD_BYTES each), imported into an
//                      empty volume
// Outputs: <dir>/out_d2.bin (uint16), out_state.bin (uint8) and out_box.txt (origin x y z, dims nx ny nz,
// max_dist, then d2 and the sign-carrying distance at the box's first voxel through the accessors).
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
    std::cerr << "usage: edt_main <dir>\n";
    return 2;
  }
  try {
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt");
    float voxel, trunc;
    int nb_bits, max_dist, min_weight, unknown;
    BoundingCube<float> cube;
    if (!(meta >> voxel >> trunc >> nb_bits >> max_dist >> min_weight >> unknown >> cube.xmin >> cube.xmax >>
          cube.ymin >> cube.ymax >> cube.zmin >> cube.zmax))
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
    const DistanceField f = sys.query_distance_field(cube, max_dist, min_weight, unknown != 0);
    write_file(dir + "/out_d2.bin", f.d2);
    write_file(dir + "/out_state.bin", f.state);
    std::ofstream(dir + "/out_box.txt") << f.origin[0] << " " << f.origin[1] << " " << f.origin[2] << " " << f.dims[0]
                                        << " " << f.dims[1] << " " << f.dims[2] << " " << f.max_dist << " "
                                        << f.d2[f.at(0, 0, 0)] << " " << f.signed_distance(0, 0, 0) << "\n";
  } catch (const std::exception& ex) {
    std::cerr << "edt_main: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
