// mesh_main.cc -- drives TSDFGrid::ExtractMesh for the GPU tests (tests/test_gpu_mesh_indexed.py).
//   mesh_main <dir>
//   <dir>/meta.txt   : voxel trunc nb_bits missing_tsdf min_weight
//   <dir>/blocks.bin : block records (tsdf_pack_blocks; TSDF_BLOCK_RECORD_BYTES each), imported into
//                      an empty volume
// Outputs: <dir>/out_verts.bin, out_tris.bin, out_rgba.bin, out_prob.bin (the four TriMesh arrays,
// raw) and out_counts.txt (vertices triangles).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "voxel_tsdf.h"

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
    std::cerr << "usage: mesh_main <dir>\n";
    return 2;
  }
  try {
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt");
    float voxel, trunc, missing;
    int nb_bits, min_weight;
    if (!(meta >> voxel >> trunc >> nb_bits >> missing >> min_weight)) throw std::runtime_error("bad meta.txt");
    tsdf_config cfg;
    tsdf_config_default(&cfg);
    cfg.voxel_size = voxel;
    cfg.truncation = trunc;
    cfg.max_width = 64;
    cfg.max_height = 64;
    cfg.num_block_bits = nb_bits;
    const std::vector<uint8_t> recs = read_file(dir + "/blocks.bin");
    if (recs.size() % TSDF_BLOCK_RECORD_BYTES) throw std::runtime_error("blocks.bin: not whole records");
    TSDFGrid grid(cfg, 0);
    check_tsdf(tsdf_import_blocks(grid.engine(), recs.data(), (int64_t)(recs.size() / TSDF_BLOCK_RECORD_BYTES),
                                  TSDF_MEM_HOST, 1),
               "tsdf_import_blocks");
    const TriMesh m = grid.ExtractMesh(nullptr, missing, min_weight);
    write_file(dir + "/out_verts.bin", m.verts);
    write_file(dir + "/out_tris.bin", m.tris);
    write_file(dir + "/out_rgba.bin", m.rgba);
    write_file(dir + "/out_prob.bin", m.prob);
    std::ofstream(dir + "/out_counts.txt") << m.prob.size() << " " << m.tris.size() / 3 << "\n";
  } catch (const std::exception& ex) {
    std::cerr << "mesh_main: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
