// dose_main.cc -- drives DISINFSystem::query_mesh + irradiate for the GPU tests (tests/test_gpu_uv_dose.py).
//   dose_main <dir>
//   <dir>/meta.txt     : voxel trunc nb_bits emitters
//   <dir>/blocks.bin   : block records (tsdf_pack_blocks; TSDF_BLOCK_RECORD_BYTES each), imported into
//                        an empty volume
//   <dir>/emitters.bin : 4 floats per emitter (x y z energy)
// Outputs: <dir>/out_verts.bin, out_normals.bin, out_dose.bin, out_keys.bin (raw TriMesh arrays) and
// out_counts.txt (vertices).
#include <cstdio>
#include <cstring>
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
    std::cerr << "usage: dose_main <dir>\n";
    return 2;
  }
  try {
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt");
    float voxel, trunc;
    int nb_bits, m;
    if (!(meta >> voxel >> trunc >> nb_bits >> m) || m < 0) throw std::runtime_error("bad meta.txt");
    tsdf_config cfg;
    tsdf_config_default(&cfg);
    cfg.max_width = 64;
    cfg.max_height = 64;
    cfg.num_block_bits = nb_bits;
    const std::vector<uint8_t> recs = read_file(dir + "/blocks.bin");
    if (recs.size() % TSDF_BLOCK_RECORD_BYTES) throw std::runtime_error("blocks.bin: not whole records");
    const std::vector<uint8_t> eb = read_file(dir + "/emitters.bin");
    if (eb.size() != (size_t)m * sizeof(UVEmitter)) throw std::runtime_error("emitters.bin: unexpected size");
    std::vector<UVEmitter> emitters((size_t)m);
    if (m) std::memcpy(emitters.data(), eb.data(), eb.size());
    DISINFSystem sys(voxel, trunc, 4.0f, CameraIntrinsics<float>(60.0f, 60.0f, 32.0f, 32.0f), SE3<float>::Identity(),
                     1000.0f, &cfg, 0);
    sys.tsdf().ImportBlocks(recs.data(), (int64_t)(recs.size() / TSDF_BLOCK_RECORD_BYTES), true);
    BoundingCube<float> all{-1e4f, 1e4f, -1e4f, 1e4f, -1e4f, 1e4f};
    TriMesh mesh = sys.query_mesh(all);
    sys.irradiate(mesh, emitters);
    write_file(dir + "/out_verts.bin", mesh.verts);
    write_file(dir + "/out_normals.bin", mesh.normals);
    write_file(dir + "/out_dose.bin", mesh.dose);
    write_file(dir + "/out_keys.bin", mesh.keys);
    std::ofstream(dir + "/out_counts.txt") << mesh.dose.size() << "\n";
  } catch (const std::exception& ex) {
    std::cerr << "dose_main: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
