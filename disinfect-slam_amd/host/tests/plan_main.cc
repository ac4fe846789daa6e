// plan_main.cc -- drives DISINFSystem::query_mesh + plan_irradiation for the GPU tests (tests/test_gpu_plan.py).
//   plan_main <dir>
//   <dir>/meta.txt     : voxel trunc nb_bits target max_stops
//   <dir>/blocks.bin   : block records (tsdf_pack_blocks; TSDF_BLOCK_RECORD_BYTES each), imported into
//                        an empty volume
//   <dir>/emitters.bin : 4 floats per emitter (x y z energy), every candidate's in turn
//   <dir>/first.bin    : int32 offsets into them, one more than there are candidates
// Outputs: <dir>/out_stops.bin (int32), out_gains.bin (double), out_need.bin (float, one per vertex) and
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
    std::cerr << "usage: plan_main <dir>\n";
    return 2;
  }
  try {
    const std::string dir = argv[1];
    std::ifstream meta(dir + "/meta.txt");
    float voxel, trunc, target;
    int nb_bits, max_stops;
    if (!(meta >> voxel >> trunc >> nb_bits >> target >> max_stops) || max_stops < 0)
      throw std::runtime_error("bad meta.txt");
    tsdf_config cfg;
    tsdf_config_default(&cfg);
    cfg.max_width = 64;
    cfg.max_height = 64;
    cfg.num_block_bits = nb_bits;
    const std::vector<uint8_t> recs = read_file(dir + "/blocks.bin");
    if (recs.size() % TSDF_BLOCK_RECORD_BYTES) throw std::runtime_error("blocks.bin: not whole records");
    const std::vector<uint8_t> eb = read_file(dir + "/emitters.bin"), fb = read_file(dir + "/first.bin");
    if (eb.size() % sizeof(UVEmitter) || fb.size() % 4 || fb.empty())
      throw std::runtime_error("emitters.bin / first.bin: unexpected size");
    LampCandidates cand;
    cand.emitters.resize(eb.size() / sizeof(UVEmitter));
    cand.first.resize(fb.size() / 4);
    if (!eb.empty()) std::memcpy(cand.emitters.data(), eb.data(), eb.size());
    std::memcpy(cand.first.data(), fb.data(), fb.size());
    DISINFSystem sys(voxel, trunc, 4.0f, CameraIntrinsics<float>(60.0f, 60.0f, 32.0f, 32.0f), SE3<float>::Identity(),
                     1000.0f, &cfg, 0);
    sys.tsdf().ImportBlocks(recs.data(), (int64_t)(recs.size() / TSDF_BLOCK_RECORD_BYTES), true);
    BoundingCube<float> all{-1e4f, 1e4f, -1e4f, 1e4f, -1e4f, 1e4f};
    TriMesh mesh = sys.query_mesh(all);
    const DISINFSystem::LampPlan plan = sys.plan_irradiation(mesh, {}, target, cand, max_stops);
    write_file(dir + "/out_stops.bin", plan.stops);
    write_file(dir + "/out_gains.bin", plan.gains);
    write_file(dir + "/out_need.bin", plan.need);
    std::ofstream(dir + "/out_counts.txt") << plan.need.size() << "\n";
  } catch (const std::exception& ex) {
    std::cerr << "plan_main: " << ex.what() << "\n";
    return 1;
  }
  return 0;
}
