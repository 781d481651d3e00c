// The label site with an environment on BOTH sides (tnml_set_any_position):
//   f[l][s] = sum_{a, d, c} Lenv[a][s] * x[s][d] * A[a][d][c][l] * Renv[c][s]
// A is the label core of an intermediate site, [ml][D][mr][L] as it lies in memory; both environments are [bond][b_pad], so the
// lanes of a wave read consecutive floats.  D is a runtime argument (2 .. kMaxD).
//
// One lane per sample, one wave per workgroup (64 samples): the b_pad / 64 workgroups of a C3 batch (313) are spread over the
// chip and no lane ever talks to another one.  LDS holds
//   * the right environment of the workgroup's samples, [mr][64]: lane s reads word c * 64 + s -- consecutive lanes, consecutive
//     banks, no conflict; it is read ml * D times, the left environment and the features once (registers);
//   * a chunk of whole a-rows of the label core ([D][mr][L] each), copied as it lies in memory.  Every lane reads the SAME core
//     element at the same time: a broadcast, conflict-free whatever the strides.
// The chunk is as many rows as fit beside the environment tile under the 160 KB limit (launch_label_meet); bond 50 with ten labels
// (200 KB) takes two chunks.  Measured: 0.18 ms beside a 1.5 ms chain at C3 (313 workgroups), 2.2 ms beside a
// 5.5 ms chain at C5, where 79 one-wave workgroups leave most of the chip idle: several waves per sample tile are the next step there.
//
// The sum runs in float32 in ONE order -- a outermost, then d, then c, one fused multiply-add per label -- and the chunk
// boundaries fall between two values of a: the result does not depend on the chunk size.  Labels are taken kMeetLT at a time
// (accumulators in registers); for L <= kMeetLT that is one pass.  Samples b .. b_pad - 1 produce 0.
#include "tnml_internal.h"

namespace tnml {

constexpr int kMeetTS = 64;      // samples (= lanes) per workgroup
constexpr int kMeetLT = 16;      // labels per pass

__global__ __launch_bounds__(kMeetTS) void label_meet_kernel(MeetParams p) {
  extern __shared__ __attribute__((aligned(16))) float meet_smem[];
  float *sR = meet_smem;                                   // [mr][64]
  float *sA = meet_smem + (size_t)p.mr * kMeetTS;          // [rows_per_chunk][D][mr][L]
  const int lane = threadIdx.x;
  const int s = blockIdx.x * kMeetTS + lane;               // < b_pad (grid = b_pad / 64)
  const int D = p.D, L = p.L, ml = p.ml, mr = p.mr;
  const int row = D * mr * L;                              // floats of one a-row
  for (int c = 0; c < mr; ++c) sR[c * kMeetTS + lane] = p.Renv[(size_t)c * p.b_pad + s];
  float x[kMaxD];
#pragma unroll
  for (int d = 0; d < kMaxD; ++d) x[d] = d < D ? p.x[(size_t)s * D + d] : 0.f;
  const bool live = s < p.b;
  for (int l0 = 0; l0 < L; l0 += kMeetLT) {
    const int nl = min(kMeetLT, L - l0);
    float acc[kMeetLT];
#pragma unroll
    for (int j = 0; j < kMeetLT; ++j) acc[j] = 0.f;
    for (int a0 = 0; a0 < ml; a0 += p.rows_per_chunk) {
      const int na = min(p.rows_per_chunk, ml - a0);
      __syncthreads();                                     // the previous chunk has been read (first pass: sR is complete)
      const float *src = p.core + (size_t)a0 * row;
      for (int e = lane; e < na * row; e += kMeetTS) sA[e] = src[e];
      __syncthreads();
      for (int a = 0; a < na; ++a) {
        const float la = p.Lenv[(size_t)(a0 + a) * p.b_pad + s];
        for (int d = 0; d < D; ++d) {
          const float w = la * x[d];
          const float *arow = sA + ((size_t)a * D + d) * mr * L + l0;
          for (int c = 0; c < mr; ++c) {
            const float wr = w * sR[c * kMeetTS + lane];
            const float *ap = arow + (size_t)c * L;
#pragma unroll
            for (int j = 0; j < kMeetLT; ++j)
              if (j < nl) acc[j] = fmaf(wr, ap[j], acc[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kMeetLT; ++j)
      if (j < nl) p.f[(size_t)(l0 + j) * p.b_pad + s] = live ? acc[j] : 0.f;
  }
}

// rows of the label core per chunk at these dimensions: all of them, or as many as fit beside the environment tile; 0: not even one
int label_meet_chunk_rows(int ml, int mr, int D, int L) {
  const size_t budget = 160 * 1024, tile = (size_t)mr * kMeetTS * sizeof(float), row = (size_t)D * mr * L * sizeof(float);
  if (tile + row > budget) return 0;
  return (int)std::min<size_t>((size_t)ml, (budget - tile) / row);
}

size_t label_meet_lds_bytes(int rows_per_chunk, int mr, int D, int L) {
  return ((size_t)mr * kMeetTS + (size_t)rows_per_chunk * D * mr * L) * sizeof(float);
}

bool launch_label_meet(MeetParams p, hipStream_t st) {
  if (p.D < 2 || p.D > kMaxD || p.b_pad % kMeetTS || p.b < 1 || p.b > p.b_pad || p.ml < 1 || p.mr < 1 || p.L < 1) return false;
  if (p.rows_per_chunk <= 0) p.rows_per_chunk = label_meet_chunk_rows(p.ml, p.mr, p.D, p.L);
  if (p.rows_per_chunk < 1) return false;
  p.rows_per_chunk = std::min(p.rows_per_chunk, p.ml);
  const size_t lds = label_meet_lds_bytes(p.rows_per_chunk, p.mr, p.D, p.L);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(label_meet_kernel, dim3(p.b_pad / kMeetTS), dim3(kMeetTS), lds, st, p);
  return true;
}

}  // namespace tnml
