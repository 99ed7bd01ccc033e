// sized_frames.cpp -- GraspDetector::detectGraspPosesInFrame(cloud, size_left_cloud), both record types, beside the
// three calls it stands for: CloudCamera(cloud, size_left_cloud) + setSampleIndices + detectGraspPoses
// (grasp_detection_node.cpp:123-143 with the index list of :278).  Records are compared as bytes.
//
//   sized_frames <cloud.f32> <normals.f32> <idx.i32> <params.txt> <size_left>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "agile_grasp2/cloud_camera.h"
#include "agile_grasp2/grasp_detector.h"

template <class T>
static std::vector<T> read_all(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> out(raw.size() / sizeof(T));
  std::memcpy(out.data(), raw.data(), out.size() * sizeof(T));
  return out;
}

static bool same_hands(const std::vector<GraspHypothesis>& a, const std::vector<GraspHypothesis>& b, const char* what) {
  if (a.size() != b.size()) {
    fprintf(stderr, "%s: %zu hands against %zu\n", what, a.size(), b.size());
    return false;
  }
  for (size_t i = 0; i < a.size(); i++) {
    const ag2_hypothesis ra = a[i].toRecord(), rb = b[i].toRecord();
    if (std::memcmp(&ra, &rb, sizeof(ra)) != 0) {
      fprintf(stderr, "%s: hand %zu differs (slot %d / %d, orientation %d / %d, score %.9g / %.9g)\n", what, i,
              ra.sample_slot, rb.sample_slot, ra.orientation, rb.orientation, ra.score, rb.score);
      return false;
    }
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s <cloud.f32> <normals.f32> <idx.i32> <params.txt> <size_left>\n", argv[0]);
    return 2;
  }
  const std::vector<float> xyz = read_all<float>(argv[1]);
  const std::vector<float> nrm = read_all<float>(argv[2]);
  const std::vector<int32_t> idx = read_all<int32_t>(argv[3]);
  std::ifstream pf(argv[4]);
  const std::string ptext((std::istreambuf_iterator<char>(pf)), std::istreambuf_iterator<char>());
  const int size_left = atoi(argv[5]);
  GraspDetector::Params prm;
  std::string err;
  if (!GraspDetector::Params::fromKeyValueText(ptext, &prm, &err)) {
    fprintf(stderr, "params: %s\n", err.c_str());
    return 2;
  }
  const size_t n = xyz.size() / 3;
  if (nrm.size() != xyz.size() || size_left < 0 || (size_t)size_left >= n) {
    fprintf(stderr, "bad input sizes\n");
    return 2;
  }
  PointCloudRGB::Ptr cloud(new PointCloudRGB);
  PointCloudNormal::Ptr cloud_n(new PointCloudNormal);
  cloud->points.resize(n);
  cloud_n->points.resize(n);
  for (size_t i = 0; i < n; i++) {
    ag2::PointXYZRGBA& p = cloud->points[i];
    ag2::PointXYZRGBNormal& q = cloud_n->points[i];
    p.x = q.x = xyz[3 * i];
    p.y = q.y = xyz[3 * i + 1];
    p.z = q.z = xyz[3 * i + 2];
    q.normal_x = nrm[3 * i];
    q.normal_y = nrm[3 * i + 1];
    q.normal_z = nrm[3 * i + 2];
  }
  agile_grasp2::CloudIndexed msg;
  msg.indices.resize(idx.size());
  for (size_t i = 0; i < idx.size(); i++) msg.indices[i].data = idx[i];
  const std::vector<int> indices(idx.begin(), idx.end());

  GraspDetector frames(prm), three(prm);
  // no index list: nothing, as the reference's topic path
  if (!frames.detectGraspPosesInFrame(cloud, size_left).empty() || !frames.detectGraspPosesInFrame(cloud_n, size_left).empty()) {
    fprintf(stderr, "hands without an index list\n");
    return 1;
  }
  frames.setIndicesFromMsg(msg);
  three.setIndicesFromMsg(msg);  // (with indices set detectGraspPoses skips the prune, grasp_detector.cpp:150-160)

  CloudCamera cc(cloud, size_left);
  cc.setSampleIndices(indices);
  const std::vector<GraspHypothesis> want = three.detectGraspPoses(cc);
  CloudCamera cc_n(cloud_n, size_left);
  cc_n.setSampleIndices(indices);
  const std::vector<GraspHypothesis> want_n = three.detectGraspPoses(cc_n);
  if (want.empty() || want_n.empty() || same_hands(want, want_n, "(the normals must matter)")) {
    fprintf(stderr, "the composition found no hands, or the given normals changed nothing\n");
    return 1;
  }
  // three frames each: step by step, at fixed shapes, replayed; then the other record type (normals come, go, come)
  for (int round = 0; round < 2; round++) {
    for (int k = 0; k < 3; k++)
      if (!same_hands(frames.detectGraspPosesInFrame(cloud, size_left), want, "PointXYZRGBA frame")) return 1;
    for (int k = 0; k < 3; k++)
      if (!same_hands(frames.detectGraspPosesInFrame(cloud_n, size_left), want_n, "PointXYZRGBNormal frame")) return 1;
  }
  if (!frames.lastError().empty()) {
    fprintf(stderr, "frames: %s\n", frames.lastError().c_str());
    return 1;
  }
  // size_left == size is the one-camera constructor (an all-zero camera matrix): the three calls, same hands
  {
    CloudCamera one(cloud, (int)n);
    one.setSampleIndices(indices);
    if (!same_hands(frames.detectGraspPosesInFrame(cloud, (int)n), three.detectGraspPoses(one), "size_left == size")) return 1;
  }
  printf("sized frames ok: %zu hands, %zu with the given normals\n", want.size(), want_n.size());
  return 0;
}
