// k_importance.hip -- the sampler of ImportanceSampling (importance_sampling.cpp:50-90): one round's xyz
// samples, drawn around the hands found so far, on the device.  Also the append of a round's selected
// records to the hand list the next round draws from.
//
// The host loop (agile_grasp2_amd/host/ag2_host.cpp, ImportanceSampling::detectGraspPoses) gives candidate c of
// round `it` the counter draws 7c .. 7c+6 of stream 0xFFFFFFFFFFFF0000 + it -- one pick, then three Box-Muller
// pairs -- whether it is accepted or not.  Candidates are therefore independent: a workgroup evaluates a batch of
// them at once and keeps the accepted ones in candidate order (ballot + popcount, as k_select.hip compacts slots),
// until num_gauss are kept or the host's guard of 10^6 candidates is reached.  The random samples that follow take
// the counters after the last candidate tried.
#include <math.h>

#include "ag2_internal.h"

namespace ag2 {

namespace {

constexpr int kIsThreads = 256;         // candidates per batch (4 waves)
constexpr int kIsHandChunk = 1024;      // hand surfaces staged in LDS at a time (24 KB)
constexpr long long kIsGuard = 1000000; // candidates per round at most, as the host loop

__device__ __forceinline__ double u53_open(uint64_t r) {  // (0, 1]: log(u1) is finite
  return (double)((r >> 11) + 1ull) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ double u53(uint64_t r) { return (double)(r >> 11) * (1.0 / 9007199254740992.0); }

// One workgroup.  The surface of hand h is srf[h * stride + 0 .. 2], *d_nh hands.  out_xyz: 3 x S doubles
// (column-major), out_q: S query points as upload_samples writes them (float xyz, finite flag), info: {tried,
// accepted}.
__global__ void __launch_bounds__(kIsThreads)
k_is_sample(const double* __restrict__ srf0, int stride, const unsigned* __restrict__ d_nh, int method,
            double sigma, double term, double coef, uint64_t seed, uint64_t stream, int S, int num_gauss,
            const float4* __restrict__ cloud, long long n_cloud, double* __restrict__ out_xyz,
            float4* __restrict__ out_q, long long* __restrict__ info) {
  __shared__ double sx[kIsHandChunk], sy[kIsHandChunk], sz[kIsHandChunk];
  __shared__ unsigned wave_acc[kIsThreads / 64];
  __shared__ long long s_tried;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned nh = *d_nh;
  if (nh == 0u || n_cloud <= 0) {  // no hand: the round does not run -- invalid query points, an empty detect
    for (int q = tid; q < S; q += kIsThreads) {
      out_xyz[3 * q] = out_xyz[3 * q + 1] = out_xyz[3 * q + 2] = 0.0;
      out_q[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (tid == 0) info[0] = info[1] = 0;
    return;
  }
  int j = 0;             // accepted so far (the same in every thread)
  long long tried = 0;
  if (num_gauss > 0) {
    if (tid == 0) s_tried = -1;
    for (long long base = 0;; base += kIsThreads) {
      const long long cand = base + tid;
      const bool active = cand < kIsGuard;
      uint64_t ctr = 7ull * (uint64_t)cand;
      unsigned idx = 0;
      double x[3] = {0.0, 0.0, 0.0};
      if (active) {
        idx = (unsigned)(draw_u64(seed, stream, ctr++) % (uint64_t)nh);
        const double* srf = srf0 + (size_t)idx * stride;
        for (int k = 0; k < 3; k++) {
          const double u1 = u53_open(draw_u64(seed, stream, ctr++));
          const double u2 = u53(draw_u64(seed, stream, ctr++));
          const double g = sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
          x[k] = srf[k] + g * sigma;
        }
      }
      bool accept = active;
      if (method == 2) {  // MAX: own density >= the maximum over all hands (rejection sampling)
        double maxp = 0.0;
        for (unsigned h0 = 0; h0 < nh; h0 += kIsHandChunk) {
          const unsigned m = min(nh - h0, (unsigned)kIsHandChunk);
          __syncthreads();
          for (unsigned h = tid; h < m; h += kIsThreads) {
            const double* srf = srf0 + (size_t)(h0 + h) * stride;
            sx[h] = srf[0];
            sy[h] = srf[1];
            sz[h] = srf[2];
          }
          __syncthreads();
          if (active)
            for (unsigned h = 0; h < m; h++) {
              const double d0 = x[0] - sx[h], d1 = x[1] - sy[h], d2 = x[2] - sz[h];
              const double p = term * exp(coef * ((d0 * d0 + d1 * d1) + d2 * d2));
              maxp = (maxp < p) ? p : maxp;  // std::max
            }
        }
        if (active) {
          const double* srf = srf0 + (size_t)idx * stride;
          const double d0 = x[0] - srf[0], d1 = x[1] - srf[1], d2 = x[2] - srf[2];
          accept = term * exp(coef * ((d0 * d0 + d1 * d1) + d2 * d2)) >= maxp;
        }
      }
      // rank of this candidate among the batch's accepted ones, in candidate order
      const unsigned long long mask = __ballot(accept);
      const unsigned below = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
      if (lane == 0) wave_acc[wave] = (unsigned)__popcll(mask);
      __syncthreads();
      unsigned before = 0, total = 0;
      for (int w = 0; w < kIsThreads / 64; w++) {
        before += (w < wave) ? wave_acc[w] : 0u;
        total += wave_acc[w];
      }
      const int rank = j + (int)(before + below);
      if (accept && rank < num_gauss) {
        out_xyz[3 * rank] = x[0];
        out_xyz[3 * rank + 1] = x[1];
        out_xyz[3 * rank + 2] = x[2];
        if (rank == num_gauss - 1) s_tried = cand + 1;  // the candidate that filled the last slot
      }
      __syncthreads();  // (wave_acc and s_tried are read below / rewritten by the next batch)
      j += (int)total;
      if (j >= num_gauss) {
        tried = s_tried;
        j = num_gauss;
        break;
      }
      if (base + kIsThreads >= kIsGuard) {  // the guard: slots left unfilled stay (0, 0, 0) as in the host matrix
        tried = kIsGuard;
        for (int q = j + tid; q < num_gauss; q += kIsThreads)
          out_xyz[3 * q] = out_xyz[3 * q + 1] = out_xyz[3 * q + 2] = 0.0;
        break;
      }
    }
    __syncthreads();  // (the Gaussian samples are written: the query points below read them)
  }
  // random samples: cloud points, counters 7 * tried + (q - num_gauss)
  for (int q = num_gauss + tid; q < S; q += kIsThreads) {
    const uint64_t ctr = 7ull * (uint64_t)tried + (uint64_t)(q - num_gauss);
    const float4 p = cloud[draw_u64(seed, stream, ctr) % (uint64_t)n_cloud];
    out_xyz[3 * q] = (double)p.x;
    out_xyz[3 * q + 1] = (double)p.y;
    out_xyz[3 * q + 2] = (double)p.z;
  }
  __syncthreads();
  // the query points of the round's detect (upload_samples: double -> float, valid = all finite)
  for (int q = tid; q < S; q += kIsThreads) {
    const float fx = (float)out_xyz[3 * q], fy = (float)out_xyz[3 * q + 1], fz = (float)out_xyz[3 * q + 2];
    const bool ok = isfinite(fx) && isfinite(fy) && isfinite(fz);
    out_q[q] = make_float4(fx, fy, fz, ok ? 1.f : 0.f);
  }
  if (tid == 0) {
    info[0] = tried;
    info[1] = j;
  }
}

// hands[*d_nh ..] += fo->n_out records of rec (one workgroup); *d_nh grows by as many, at most to cap
__global__ void k_is_append(const FrameOut* __restrict__ fo, const ag2_hypothesis* __restrict__ rec,
                            ag2_hypothesis* __restrict__ hands, unsigned* __restrict__ d_nh, unsigned cap) {
  const unsigned base = *d_nh;
  const unsigned n = min(fo->n_out, cap - min(base, cap));
  constexpr int kPer = (int)(sizeof(ag2_hypothesis) / 16);
  const uint4* src = reinterpret_cast<const uint4*>(rec);
  uint4* dst = reinterpret_cast<uint4*>(hands + base);
  for (unsigned i = threadIdx.x; i < n * kPer; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
  if (threadIdx.x == 0) *d_nh = base + n;
}

}  // namespace

int launch_is_sample(ag2_ctx* c, const double* d_srf, int stride, const unsigned* d_nh, const IsRound& r,
                     double* d_xyz, float4* d_q, long long* d_info) {
  hipLaunchKernelGGL(k_is_sample, dim3(1), dim3(kIsThreads), 0, c->stream, d_srf, stride, d_nh, r.method, r.sigma,
                     r.term, r.coef, r.seed, r.stream, r.num_samples, r.num_gauss, c->d_xyz_in.as<float4>(),
                     (long long)c->n, d_xyz, d_q, d_info);
  AG2_HIP(c, hipGetLastError());
  return 0;
}

int launch_is_append(ag2_ctx* c, const FrameOut* d_fo, const ag2_hypothesis* d_rec, ag2_hypothesis* d_hands,
                     unsigned* d_nh, unsigned cap) {
  hipLaunchKernelGGL(k_is_append, dim3(1), dim3(256), 0, c->stream, d_fo, d_rec, d_hands, d_nh, cap);
  AG2_HIP(c, hipGetLastError());
  return 0;
}

}  // namespace ag2
