// ag2_importance.hip -- C-ABI of ImportanceSampling::detectGraspPoses (importance_sampling.cpp:30-118) with the
// loop on the device: the initial detect, num_iterations rounds of (sampler -> detect on the round's xyz samples
// -> append the selected hands), then the clustering.  Orchestration only; the sampler is k_importance.hip.
//
// Two forms, same bytes:
//  * step by step (a context's first call, and any call whose shapes did not hold): ag2_detect on the indices,
//    then per round the sampler on the hands found so far (uploaded), its samples read back, ag2_detect on them;
//    ag2_find_clusters at the end.  This is literally the composition of existing calls, and it learns the shapes.
//  * one trip (from the second call on): every step is queued at once at the shapes the previous call left --
//    the detect tails as in ag2_detect's one-round-trip form (list lengths read on the device, top-k on the
//    device), the selected records appended to a device-resident hand list that the next round's sampler reads,
//    the sampler writing the round's query points straight where the frame kernel reads them -- and ONE
//    read-back brings every round's statistics, samples and counts and the hands.  If a round's statistics say
//    its shapes did not hold, the call runs again step by step.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "ag2_internal.h"

using namespace ag2;

namespace {

constexpr int kIsRedo = 1;

IsRound round_params(const ag2_importance_params& ip, uint64_t seed, int it) {
  IsRound r{};
  const int num_rand = (int)(ip.prob_rand_samples * ip.num_samples);
  r.method = ip.method;
  r.sigma = ip.radius;
  r.term = 1.0 / sqrt(pow(2.0 * M_PI, 3.0) * pow(ip.radius, 3.0));  // (host arithmetic, as the host loop)
  r.coef = -1.0 / (2.0 * ip.radius);
  r.seed = seed;
  r.stream = 0xFFFFFFFFFFFF0000ull + (uint64_t)it;
  r.num_samples = ip.num_samples;
  r.num_gauss = ip.num_samples - num_rand;
  return r;
}

// Layout of the device result block of a call (d_is): what the final read-back brings, then the top-k staging.
struct IsLayout {
  size_t fo, info, xyz, nh, hands, stage, total;
  size_t h_cap;
};
IsLayout is_layout(int R, int S, size_t h_cap, size_t stage_cap) {
  IsLayout L{};
  L.fo = 0;
  L.info = L.fo + (size_t)(R + 1) * sizeof(FrameOut);
  L.xyz = L.info + (size_t)std::max(R, 1) * 16;
  L.nh = L.xyz + (size_t)std::max(R, 1) * (size_t)S * 24;
  L.hands = ((L.nh + 16 + 255) / 256) * 256;
  L.stage = L.hands + (h_cap + 1) * sizeof(ag2_hypothesis);
  L.total = L.stage + std::max<size_t>(stage_cap, 1) * sizeof(ag2_hypothesis);
  L.h_cap = h_cap;
  return L;
}

void is_reset_info(ag2_ctx* c, const ag2_importance_params& ip) {
  memset(&c->is_info, 0, sizeof(c->is_info));
  c->is_info.num_samples = ip.num_samples;
  c->is_rounds.clear();
}

// One detect (slot_base 0) queued at fixed shapes: hypotheses -> prune -> images -> LeNet -> threshold -> top k_cap
// records into d_stage, statistics into *d_fo.  preset: the query points are already in d_sample_q (a round: the
// sampler wrote them); otherwise sample_idx, or with sample_idx == NULL the indices ag2_subsample_uniformly left.
// Stage events as ag2_detect's, so that ag2_get_stage_times describes the last detect queued.
int enqueue_detect(ag2_ctx* c, const int32_t* sample_idx, bool preset, size_t s, uint64_t seed, int do_prune,
                   size_t cap_img, int max_p, FrameOut* d_fo, ag2_hypothesis* d_stage) {
  AG2_HIP(c, stage_event(c, 8));
  c->queries_preset = preset;
  int rc = enqueue_hypotheses(c, preset ? nullptr : sample_idx, s, seed, do_prune);
  c->queries_preset = false;
  if (rc) return rc;
  if (c->desc_stride == 0) return kIsRedo;  // (no descriptors from the compaction)
  const ag2_hypothesis* d_res = nullptr;
  const unsigned* d_nres = nullptr;
  rc = enqueue_tail(c, cap_img, max_p, &c->d_stats.as<DevStats>()->n_list, c->desc_stride, /*cluster=*/false, &d_res,
                    &d_nres);
  if (rc) return rc;
  rc = launch_topk(c, d_res, d_nres, cap_img, k_cap_for(c, cap_img), d_stage, d_fo, nullptr);
  if (rc) return rc;
  AG2_HIP(c, stage_event(c, 7));
  return 0;
}

// the most hands the queued form can collect: the initial detect's and every round's top-k
size_t hand_bound(const ag2_ctx* c, const ag2_ctx::IsShapes& sh, const ag2_importance_params& ip) {
  return k_cap_for(c, sh.cap_img0) + (size_t)ip.num_iterations * k_cap_for(c, sh.cap_img_r);
}

// (the sweeps of these detects always run the long-list stage)
bool shapes_held(const FrameOut& fo, size_t cap_img, int max_p) {
  return shapes_missed(fo.st, fo.topk_overflow, tail_shapes(cap_img, max_p, false)) == 0;
}

int is_one_trip(ag2_ctx* c, const int32_t* sample_idx, size_t s, uint64_t seed, int do_prune,
                const ag2_importance_params& ip, std::vector<ag2_hypothesis>* out) {
  const ag2_ctx::IsShapes& sh = c->is_shapes;
  const int R = ip.num_iterations, S = ip.num_samples;
  const size_t k0 = k_cap_for(c, sh.cap_img0), kr = k_cap_for(c, sh.cap_img_r);
  const size_t h_cap = k0 + (size_t)R * kr;
  const IsLayout L = is_layout(R, S, h_cap, std::max(k0, kr));
  const size_t clu_bytes = c->min_inliers > 0 ? h_cap * sizeof(ag2_hypothesis) + 16 : 0;  // (+ count trailer)
  const size_t back = L.stage + clu_bytes;
  // Everything that may reallocate comes first (a grown page-locked block would move the indices staged in it).
  int rc = pin_reserve(c, std::max(back, s * 4));
  if (rc) return rc;
  if (!c->h_pin_dev) return kIsRedo;
  AG2_HIP(c, c->d_is.reserve(L.total));
  AG2_HIP(c, c->d_sample_q.reserve(std::max<size_t>(std::max(s, (size_t)S), 1) * 16));
  const size_t cap_img = std::max(sh.cap_img0, sh.cap_img_r);
  AG2_HIP(c, c->d_images.reserve(cap_img * 10800));
  AG2_HIP(c, c->d_logits.reserve(cap_img * 8));
  char* base = (char*)c->d_is.p;
  FrameOut* d_fo = (FrameOut*)(base + L.fo);
  long long* d_info = (long long*)(base + L.info);
  double* d_xyz = (double*)(base + L.xyz);
  unsigned* d_nh = (unsigned*)(base + L.nh);
  ag2_hypothesis* d_hands = (ag2_hypothesis*)(base + L.hands);
  ag2_hypothesis* d_stage = (ag2_hypothesis*)(base + L.stage);
  AG2_HIP(c, hipMemsetAsync(d_nh, 0, 16, c->stream));
  rc = enqueue_detect(c, sample_idx, /*preset=*/false, s, seed, do_prune, sh.cap_img0, sh.max_p, d_fo, d_stage);
  if (rc) return rc;
  rc = launch_is_append(c, d_fo, d_stage, d_hands, d_nh, (unsigned)h_cap);
  if (rc) return rc;
  for (int it = 0; it < R; it++) {
    rc = launch_is_sample(c, (const double*)((const char*)d_hands + offsetof(ag2_hypothesis, surface)),
                          (int)(sizeof(ag2_hypothesis) / sizeof(double)), d_nh, round_params(ip, seed, it),
                          d_xyz + (size_t)it * 3 * S, c->d_sample_q.as<float4>(), d_info + 2 * it);
    if (rc) return rc;
    rc = enqueue_detect(c, nullptr, /*preset=*/true, (size_t)S, seed, do_prune, sh.cap_img_r, sh.max_p, d_fo + 1 + it,
                        d_stage);
    if (rc) return rc;
    rc = launch_is_append(c, d_fo + 1 + it, d_stage, d_hands, d_nh, (unsigned)h_cap);
    if (rc) return rc;
  }
  if (c->min_inliers > 0) {  // HandleSearch::findClusters over every hand found (importance_sampling.cpp:104-108)
    rc = cluster_async(c, d_hands, h_cap, d_nh, c->min_inliers, d_nh + 1);
    if (rc) return rc;
  }
  // the one read-back
  AG2_HIP(c, hipMemcpyAsync(pin_bulk(c), base, L.stage, hipMemcpyDeviceToHost, c->stream));
  if (clu_bytes)
    AG2_HIP(c, hipMemcpyAsync(pin_bulk(c) + L.stage, c->d_cluster.p, clu_bytes, hipMemcpyDeviceToHost, c->stream));
  AG2_HIP(c, ag2::stream_sync(c));
  const char* h = pin_bulk(c);
  std::vector<FrameOut> fo((size_t)R + 1);
  memcpy(fo.data(), h + L.fo, fo.size() * sizeof(FrameOut));
  const size_t n0 = fo[0].n_out;
  const int rounds = n0 ? R : 0;  // no hand from the initial detect: the rounds that were queued do not count
  if (!shapes_held(fo[0], sh.cap_img0, sh.max_p)) return kIsRedo;
  for (int it = 0; it < rounds; it++)
    if (!shapes_held(fo[1 + it], sh.cap_img_r, sh.max_p)) return kIsRedo;
  unsigned nh[2];
  memcpy(nh, h + L.nh, 8);
  c->is_info.n_initial = (int64_t)n0;
  c->is_info.rounds = rounds;
  c->is_info.n_hands = n0 ? nh[0] : 0;
  const long long* info = (const long long*)(h + L.info);
  for (int it = 0; it < rounds; it++) {
    c->is_info.tried[it] = info[2 * it];
    c->is_info.accepted[it] = info[2 * it + 1];
  }
  c->is_rounds.assign((const double*)(h + L.xyz), (const double*)(h + L.xyz) + (size_t)rounds * 3 * S);
  out->clear();
  if (n0) {
    if (c->min_inliers > 0) {
      const ag2_hypothesis* rec = (const ag2_hypothesis*)(h + L.stage);
      out->assign(rec, rec + nh[1]);
    } else {
      const ag2_hypothesis* rec = (const ag2_hypothesis*)(h + L.hands);
      out->assign(rec, rec + nh[0]);
    }
  }
  // the shapes follow the workload (never below what just ran)
  size_t n_img_r = 0;
  int max_p = (int)fo[0].st.max_p;
  for (int it = 0; it < rounds; it++) {
    n_img_r = std::max<size_t>(n_img_r, fo[1 + it].st.n_list);
    max_p = std::max(max_p, (int)fo[1 + it].st.max_p);
  }
  c->is_shapes.cap_img0 = std::max(c->is_shapes.cap_img0, grown_cap_img(fo[0].st.n_list));
  c->is_shapes.cap_img_r = std::max(c->is_shapes.cap_img_r, grown_cap_img(n_img_r));
  c->is_shapes.max_p = std::max(c->is_shapes.max_p, max_p);
  // counters and stage times: those of the last detect queued, as ag2_detect leaves them
  const FrameOut& last = fo[(size_t)R];
  note_detect_stats(c, R ? (size_t)S : s, last.st, last.n_out);
  return 0;
}

int is_stepwise(ag2_ctx* c, const int32_t* sample_idx, size_t s, uint64_t seed, int do_prune,
                const ag2_importance_params& ip, std::vector<ag2_hypothesis>* out) {
  const int R = ip.num_iterations, S = ip.num_samples, R_or = c->p.num_orientations;
  const int min_inliers = c->min_inliers;
  c->min_inliers = 0;  // the detects do not cluster; the loop clusters all hands at its end
  std::vector<ag2_hypothesis> hands(std::max<size_t>(1, s * (size_t)R_or)), recs(std::max(1, S * R_or));
  size_t n = 0;
  int rc = ag2_detect(c, sample_idx, nullptr, s, 0, seed, do_prune, hands.data(), hands.size(), &n, nullptr, 0,
                      nullptr);
  const size_t n_img0 = (size_t)c->cnt.n_pruned;
  int max_p = c->max_p;
  size_t n_img_r = 0;
  hands.resize(n);
  c->is_info.n_initial = (int64_t)n;
  if (!rc && n) {
    c->is_info.rounds = R;
    std::vector<double> srf, xyz((size_t)3 * S);
    for (int it = 0; it < R && !rc; it++) {
      srf.resize(3 * hands.size());
      for (size_t h = 0; h < hands.size(); h++)
        for (int k = 0; k < 3; k++) srf[3 * h + k] = hands[h].surface[k];
      int64_t tried = 0, accepted = 0;
      rc = ag2_importance_sample(c, srf.data(), hands.size(), &ip, it, seed, xyz.data(), &tried, &accepted);
      if (rc) break;
      c->is_info.tried[it] = tried;
      c->is_info.accepted[it] = accepted;
      c->is_rounds.insert(c->is_rounds.end(), xyz.begin(), xyz.end());
      size_t m = 0;
      rc = ag2_detect(c, nullptr, xyz.data(), (size_t)S, 0, seed, do_prune, recs.data(), recs.size(), &m, nullptr, 0,
                      nullptr);
      n_img_r = std::max<size_t>(n_img_r, (size_t)c->cnt.n_pruned);
      max_p = std::max(max_p, c->max_p);
      hands.insert(hands.end(), recs.begin(), recs.begin() + m);
    }
  }
  c->min_inliers = min_inliers;
  if (rc) return rc;
  c->is_info.n_hands = (int64_t)hands.size();
  if (min_inliers > 0 && !hands.empty()) {
    out->resize(hands.size());
    size_t k = 0;
    rc = ag2_find_clusters(c, hands.data(), hands.size(), min_inliers, out->data(), out->size(), &k);
    if (rc) return rc;
    out->resize(k);
  } else {
    out->swap(hands);
  }
  // shapes for the one-trip form of the next call
  ag2_ctx::IsShapes& sh = c->is_shapes;
  sh.valid = true;
  sh.s = s;
  sh.num_samples = S;
  sh.rounds = R;
  sh.prune = do_prune ? 1 : 0;
  sh.cap_img0 = grown_cap_img(n_img0);
  sh.cap_img_r = grown_cap_img(n_img_r);
  sh.max_p = max_p;
  return 0;
}

// Grows every buffer the queued form uses to the shapes just learned, through the same launchers at those shapes
// over zero items (*d_n = 0), so that the next call reallocates nothing -- hipFree waits for the device.
int is_presize(ag2_ctx* c, size_t s, const ag2_importance_params& ip) {
  const ag2_ctx::IsShapes& sh = c->is_shapes;
  const int R = ip.num_iterations, S = ip.num_samples;
  const size_t k0 = k_cap_for(c, sh.cap_img0), kr = k_cap_for(c, sh.cap_img_r);
  const size_t h_cap = k0 + (size_t)R * kr;
  const IsLayout L = is_layout(R, S, h_cap, std::max(k0, kr));
  const size_t clu_bytes = c->min_inliers > 0 ? h_cap * sizeof(ag2_hypothesis) + 16 : 0;
  int rc = pin_reserve(c, std::max(L.stage + clu_bytes, s * 4));
  if (rc) return rc;
  AG2_HIP(c, c->d_is.reserve(L.total));
  AG2_HIP(c, c->d_sample_q.reserve(std::max<size_t>(std::max(s, (size_t)S), 1) * 16));
  const size_t cap_img = std::max(sh.cap_img0, sh.cap_img_r);
  AG2_HIP(c, c->d_images.reserve(cap_img * 10800));
  AG2_HIP(c, c->d_logits.reserve(cap_img * 8));
  unsigned* d_zero = (unsigned*)((char*)c->d_is.p + L.nh);  // {0, count out}
  AG2_HIP(c, hipMemsetAsync(d_zero, 0, 16, c->stream));
  rc = launch_render(c, c->d_arena.as<double>(), c->d_desc.as<long long>(), (const int*)c->d_desc.as<long long>(),
                     cap_img, c->d_images.as<uint8_t>(), sh.max_p, d_zero);
  if (rc) return rc;
  rc = launch_lenet(c, c->d_images.as<uint8_t>(), cap_img, c->d_logits.as<float>(), -1, d_zero);
  if (rc) return rc;
  rc = score_and_select_async(c, c->d_list2.as<int>(), cap_img, d_zero + 1, d_zero);
  if (rc) return rc;
  if (c->min_inliers > 0) {
    AG2_HIP(c, hipMemsetAsync(d_zero + 1, 0, 4, c->stream));
    rc = cluster_async(c, (const ag2_hypothesis*)((char*)c->d_is.p + L.hands), h_cap, d_zero, c->min_inliers,
                       d_zero + 1);
  }
  return rc;
}

}  // namespace

extern "C" {

int ag2_importance_sample(ag2_ctx* c, const double* surfaces, size_t n_hands, const ag2_importance_params* ip,
                          int round, uint64_t seed, double* xyz, int64_t* tried, int64_t* accepted) {
  if (!c || !ip || !xyz || (n_hands && !surfaces)) return AG2_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (ip->num_samples < 1 || ip->num_samples > (1 << 20) ||
      !(ip->prob_rand_samples >= 0.0 && ip->prob_rand_samples <= 1.0) || !(ip->radius > 0.0) ||
      (ip->method != AG2_IS_SUM && ip->method != AG2_IS_MAX) || round < 0)
    return set_err(c, AG2_ERR_ARG, "importance sampling: bad parameters");
  if (!c->has_cloud || c->n == 0) return set_err(c, AG2_ERR_STATE, "no cloud set");
  if (n_hands == 0 || n_hands > ((size_t)1 << 24))
    return set_err(c, AG2_ERR_ARG, "importance sampling: 1 .. 2^24 hands");
  if (ip->method == AG2_IS_MAX && n_hands > (size_t)AG2_IMPORTANCE_MAX_HANDS)
    return set_err(c, AG2_ERR_CAPACITY, "importance sampling: MAX over more than AG2_IMPORTANCE_MAX_HANDS (" +
                                           std::to_string(AG2_IMPORTANCE_MAX_HANDS) + ") hands");
  const size_t S = (size_t)ip->num_samples;
  const size_t off_xyz = 256, off_q = off_xyz + S * 24, off_srf = off_q + S * 16;
  AG2_HIP(c, c->d_is_samp.reserve(off_srf + n_hands * 24));
  char* base = (char*)c->d_is_samp.p;
  const unsigned nh = (unsigned)n_hands;
  AG2_HIP(c, hipMemcpyAsync(base + off_srf, surfaces, n_hands * 24, hipMemcpyHostToDevice, c->stream));
  AG2_HIP(c, hipMemcpyAsync(base, &nh, 4, hipMemcpyHostToDevice, c->stream));
  int rc = launch_is_sample(c, (const double*)(base + off_srf), 3, (const unsigned*)base, round_params(*ip, seed, round),
                            (double*)(base + off_xyz), (float4*)(base + off_q), (long long*)(base + 16));
  if (rc) return rc;
  long long info[2] = {0, 0};
  AG2_HIP(c, hipMemcpyAsync(xyz, base + off_xyz, S * 24, hipMemcpyDeviceToHost, c->stream));
  AG2_HIP(c, hipMemcpyAsync(info, base + 16, 16, hipMemcpyDeviceToHost, c->stream));
  AG2_HIP(c, ag2::stream_sync(c));
  if (tried) *tried = info[0];
  if (accepted) *accepted = info[1];
  return 0;
}

void ag2_default_importance_params(ag2_importance_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->num_iterations = 5;       // importance_sampling.cpp:9-15
  p->num_samples = 50;
  p->prob_rand_samples = 0.3;
  p->radius = 0.02;
  p->method = AG2_IS_MAX;
}

int ag2_detect_importance(ag2_ctx* c, const int32_t* sample_idx, size_t s, uint64_t seed, int do_prune,
                          const ag2_importance_params* ip, ag2_hypothesis* out, size_t cap, size_t* n_out) {
  if (!c || !ip || !n_out) return AG2_ERR_ARG;
  (void)hipSetDevice(c->device);
  *n_out = 0;
  if (ip->num_iterations < 0 || ip->num_iterations > AG2_IMPORTANCE_MAX_ROUNDS || ip->num_samples < 1 ||
      ip->num_samples > (1 << 20) || !(ip->prob_rand_samples >= 0.0 && ip->prob_rand_samples <= 1.0) ||
      !(ip->radius > 0.0) || (ip->method != AG2_IS_SUM && ip->method != AG2_IS_MAX))
    return set_err(c, AG2_ERR_ARG, "importance sampling: bad parameters");
  if (!c->has_cloud) return set_err(c, AG2_ERR_STATE, "no cloud set");
  if (!c->has_normals) return set_err(c, AG2_ERR_STATE, "normals missing: call ag2_compute_normals or pass normals");
  if (!c->net.loaded) return set_err(c, AG2_ERR_STATE, "lenet weights not loaded");
  if (!sample_idx && s > c->n_resident_samples)
    return set_err(c, AG2_ERR_ARG, "no sample_idx given and fewer than s indices left by ag2_subsample_uniformly");
  int rc = rank_spec_retire(c);
  if (rc) return rc;
  is_reset_info(c, *ip);
  // host waits of this call, measured: every synchronisation the library makes on this context and every hipFree
  // (which waits for the device) -- process-wide, so another thread's reallocation would be counted here too
  const unsigned long long waits0 = c->host_waits, frees0 = g_buffer_frees.load();
  struct SyncCount {
    ag2_ctx* c;
    unsigned long long w0, f0;
    ~SyncCount() { c->is_info.host_syncs = (int64_t)((c->host_waits - w0) + (g_buffer_frees.load() - f0)); }
  } sync_count{c, waits0, frees0};
  static const bool stepwise_only = getenv("AG2_DETECT_STEPWISE") != nullptr;
  const ag2_ctx::IsShapes& sh = c->is_shapes;
  const ag2_ctx::IsShapes before = sh;
  const size_t R_or = (size_t)c->p.num_orientations;
  const bool one_trip = !stepwise_only && sh.valid && sh.s == s && sh.num_samples == ip->num_samples &&
                        sh.rounds == ip->num_iterations && sh.prune == (do_prune ? 1 : 0) &&
                        !c->fm_on && s > 0 && s * R_or <= 65536 && (size_t)ip->num_samples * R_or <= 65536 &&
                        (ip->method != AG2_IS_MAX || hand_bound(c, sh, *ip) <= (size_t)AG2_IMPORTANCE_MAX_HANDS);
  std::vector<ag2_hypothesis> res;
  if (one_trip) {
    rc = is_one_trip(c, sample_idx, s, seed, do_prune, *ip, &res);
    if (rc == 0) c->is_info.one_trip = 1;
    if (rc != kIsRedo && rc != 0) return rc;
    if (rc == kIsRedo) {
      is_reset_info(c, *ip);
      c->is_info.redone = 1;
    }
  }
  if (!one_trip || rc == kIsRedo) {
    rc = is_stepwise(c, sample_idx, s, seed, do_prune, *ip, &res);
    if (rc) return rc;
  }
  if (sh.cap_img0 != before.cap_img0 || sh.cap_img_r != before.cap_img_r || sh.max_p != before.max_p ||
      sh.s != before.s || sh.num_samples != before.num_samples || sh.rounds != before.rounds || !before.valid) {
    if (!c->fm_on && s > 0 && s * R_or <= 65536 && (size_t)ip->num_samples * R_or <= 65536 &&
        (ip->method != AG2_IS_MAX || hand_bound(c, sh, *ip) <= (size_t)AG2_IMPORTANCE_MAX_HANDS)) {
      rc = is_presize(c, s, *ip);  // (the shapes changed: the next call runs queued at them)
      if (rc) return rc;
    }
  }
  c->is_info.n_out = (int64_t)res.size();
  *n_out = res.size();
  if (res.size() > cap) return set_err(c, AG2_ERR_CAPACITY, "detect_importance: output capacity too small");
  if (!res.empty()) {
    if (!out) return set_err(c, AG2_ERR_ARG, "detect_importance: out is NULL");
    memcpy(out, res.data(), res.size() * sizeof(ag2_hypothesis));
  }
  return 0;
}

int ag2_get_importance_rounds(ag2_ctx* c, double* xyz, size_t cap, size_t* n) {
  if (!c || !n) return AG2_ERR_ARG;
  *n = c->is_rounds.size();
  if (!xyz && cap == 0) return 0;  // (a size query)
  if (cap < c->is_rounds.size()) return set_err(c, AG2_ERR_CAPACITY, "importance rounds: buffer too small");
  if (!c->is_rounds.empty()) {
    if (!xyz) return set_err(c, AG2_ERR_ARG, "importance rounds: xyz is NULL");
    memcpy(xyz, c->is_rounds.data(), c->is_rounds.size() * sizeof(double));
  }
  return 0;
}

int ag2_get_importance_info(ag2_ctx* c, ag2_importance_info* out) {
  if (!c || !out) return AG2_ERR_ARG;
  *out = c->is_info;
  return 0;
}

}  // extern "C"
