// importance_device <cloud.f32> <idx.i32> <params.txt> <on_device 0|1> <min_inliers> <out.bin> [reps rounds samples]:
// ImportanceSampling::detectGraspPoses with setSampleOnDevice(on_device), 3 rounds of 40 samples (or as given);
// with reps, the call is repeated that many times more and the median host time per call is printed.
// out.bin: int64 initial count, int64 rounds, per round int64 s + 3 x s doubles, int64 hands, then per hand
// int32 slot, int32 orientation, 11 doubles (score, bottom, surface, axis, width).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "agile_grasp2/importance_sampling.h"

template <class T>
static std::vector<T> read_all(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> out(raw.size() / sizeof(T));
  std::memcpy(out.data(), raw.data(), out.size() * sizeof(T));
  return out;
}

template <class T>
static void put(std::ofstream& f, const T* p, size_t n) {
  f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv) {
  if (argc != 7 && argc != 10) {
    fprintf(stderr, "usage: %s cloud.f32 idx.i32 params.txt on_device min_inliers out.bin [reps rounds samples]\n",
            argv[0]);
    return 2;
  }
  const std::vector<float> xyz = read_all<float>(argv[1]);
  const std::vector<int32_t> idx = read_all<int32_t>(argv[2]);
  std::ifstream pf(argv[3]);
  const std::string ptext((std::istreambuf_iterator<char>(pf)), std::istreambuf_iterator<char>());
  GraspDetector::Params prm;
  std::string err;
  if (!GraspDetector::Params::fromKeyValueText(ptext, &prm, &err)) {
    fprintf(stderr, "params: %s\n", err.c_str());
    return 2;
  }
  PointCloudRGB::Ptr cloud(new PointCloudRGB);
  cloud->points.resize(xyz.size() / 3);
  for (size_t i = 0; i < cloud->size(); i++) {
    cloud->points[i].x = xyz[3 * i];
    cloud->points[i].y = xyz[3 * i + 1];
    cloud->points[i].z = xyz[3 * i + 2];
  }
  CloudCamera cc(cloud, (int)cloud->size());
  cc.setSampleIndices(std::vector<int>(idx.begin(), idx.end()));
  ImportanceSampling is(prm);
  is.setNumIterations(argc == 10 ? std::stoi(argv[8]) : 3);
  is.setNumSamplesPerIteration(argc == 10 ? std::stoi(argv[9]) : 40);
  is.setSampleOnDevice(std::string(argv[4]) == "1");
  is.getHandleSearch().setMinInliers(std::stoi(argv[5]));
  std::vector<GraspHypothesis> hands = is.detectGraspPoses(cc);
  hands = is.detectGraspPoses(cc);  // (a second call: on the device, the one-trip form)
  if (argc == 10) {
    std::vector<double> ms;
    for (int r = 0; r < std::stoi(argv[7]); r++) {
      const auto t0 = std::chrono::steady_clock::now();
      hands = is.detectGraspPoses(cc);
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    if (!ms.empty()) printf("median_ms %.4f over %zu calls\n", ms[ms.size() / 2], ms.size());
  }
  std::ofstream out(argv[6], std::ios::binary);
  const int64_t n0 = is.lastInitialCount(), nr = (int64_t)is.lastSampleRounds().size(), nh = (int64_t)hands.size();
  put(out, &n0, 1);
  put(out, &nr, 1);
  for (const ag2::Matrix3Xd& m : is.lastSampleRounds()) {
    const int64_t s = m.cols();
    put(out, &s, 1);
    put(out, m.data(), (size_t)(3 * s));
  }
  put(out, &nh, 1);
  for (const GraspHypothesis& h : hands) {
    const int32_t so[2] = {h.getSampleSlot(), h.getOrientation()};
    const double v[11] = {h.getScore(),         h.getGraspBottom()(0),  h.getGraspBottom()(1), h.getGraspBottom()(2),
                          h.getGraspSurface()(0), h.getGraspSurface()(1), h.getGraspSurface()(2), h.getAxis()(0),
                          h.getAxis()(1),       h.getAxis()(2),         h.getGraspWidth()};
    put(out, so, 2);
    put(out, v, 11);
  }
  printf("importance ok: %lld initial, %lld rounds, %lld hands\n", (long long)n0, (long long)nr, (long long)nh);
  return 0;
}
