// Kernels of the device-resident dataset (tnml_dataset_attach / tnml_select_indices / tnml_eval_indices):
//   * gather / embed / re-tile: sample rows picked by an index list -> the site-major layout x[site][b_pad][D] the chain and step
//     kernels read, padding samples zeroed, labels gathered by the same launch;
//   * metrics over f [L][b_pad]: activation, argmax, |onehot - act(f)|, reduced per wave and per workgroup, then summed in a fixed
//     order by a one-thread kernel (so that the same samples in the same 256-sample blocks always give the same sums).
//
// The dataset is stored sample-major ("contiguous along sites"): features [n][N][D] or pixels [n][N].  The batch layout is
// "contiguous along samples".  Both kernels go through an LDS tile of 32 samples x 32 sites so that the reads (along sites of one
// sample row) and the writes (along samples of one site) are both coalesced, as transpose_input_kernel does for a dense batch.
#include "tnml_internal.h"
#include "act_device.h"

namespace tnml {

// psi of one pixel (data_generator.psi): float64 throughout, one rounding to float32 per component -- what the host does when it
// embeds in float64 and converts the result to float32.
//   D = 2:  [sin(pi x / 2), cos(pi x / 2)]
//   D > 2:  sqrt(C(D-1, s)) sin^(D-1-s) cos^s,  s = 0 .. D-1   (coef[s] = sqrt(C(D-1, s)) comes from the host)
__device__ inline double ds_powi(double v, int k) {
  double r = 1.0;                       // v^0 == 1 also at v == 0, as NumPy's power
  for (int i = 0; i < k; ++i) r *= v;
  return r;
}
__device__ inline void ds_sincos(float px, double &sn, double &cs) {
  const double a = 3.141592653589793 * (double)px / 2;       // the host's order of operations: (pi * x) / 2
  sn = sin(a);
  cs = cos(a);
}

// ------------------------------------------------------------------------------------------
// D == 2: one float2 per (sample, site); grid (b_pad / 32, ceil(N / 32)), 256 threads
// ------------------------------------------------------------------------------------------
template <bool PIXELS>
__global__ void dataset_gather_d2_kernel(DatasetGather p) {
  __shared__ float2 tile[32][33];
  __shared__ int rows[32];
  const int s0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  if (threadIdx.x < 32) {
    const int s = s0 + threadIdx.x;
    const int row = s < p.b ? p.idx[s] : -1;
    rows[threadIdx.x] = row;
    if (blockIdx.y == 0 && p.y_out && s < p.b_pad) p.y_out[s] = row >= 0 ? p.labels[row] : 0;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int row = rows[r], n = n0 + tx;
    float2 v = make_float2(0.f, 0.f);
    if (row >= 0 && n < p.N) {
      if (PIXELS) {
        double sn, cs;
        ds_sincos(p.data[(size_t)row * p.N + n], sn, cs);
        v = make_float2((float)sn, (float)cs);
      } else {
        v = ((const float2 *)p.data)[(size_t)row * p.N + n];
      }
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  float2 *out = (float2 *)p.out;
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r, s = s0 + tx;
    if (n < p.N && s < p.b_pad) out[(size_t)n * p.b_pad + s] = tile[tx][r];
  }
}

// ------------------------------------------------------------------------------------------
// general D: the tile holds 32 samples x (32 sites x D) floats; same grid
// ------------------------------------------------------------------------------------------
template <bool PIXELS>
__global__ void dataset_gather_anyd_kernel(DatasetGather p) {
  __shared__ float tile[32][32 * kMaxD + 1];
  __shared__ int rows[32];
  const int D = p.D, W = 32 * D;
  const int s0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  if (threadIdx.x < 32) {
    const int s = s0 + threadIdx.x;
    const int row = s < p.b ? p.idx[s] : -1;
    rows[threadIdx.x] = row;
    if (blockIdx.y == 0 && p.y_out && s < p.b_pad) p.y_out[s] = row >= 0 ? p.labels[row] : 0;
  }
  __syncthreads();
  if (PIXELS) {
    for (int q = threadIdx.x; q < 32 * 32; q += blockDim.x) {
      const int r = q >> 5, nl = q & 31, row = rows[r], n = n0 + nl;
      const bool live = row >= 0 && n < p.N;
      double sn = 0.0, cs = 0.0;
      if (live) ds_sincos(p.data[(size_t)row * p.N + n], sn, cs);
      for (int d = 0; d < D; ++d)
        tile[r][nl * D + d] = live ? (float)(p.coef[d] * ds_powi(sn, D - 1 - d) * ds_powi(cs, d)) : 0.f;
    }
  } else {
    for (int q = threadIdx.x; q < 32 * W; q += blockDim.x) {
      const int r = q / W, e = q - r * W, row = rows[r], n = n0 + e / D;
      tile[r][e] = (row >= 0 && n < p.N) ? p.data[((size_t)row * p.N + n0) * D + e] : 0.f;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < 32 * W; q += blockDim.x) {
    const int nl = q / W, j = q - nl * W, sl = j / D, d = j - sl * D;
    const int n = n0 + nl, s = s0 + sl;
    if (n < p.N && s < p.b_pad) p.out[((size_t)n * p.b_pad + s0) * D + j] = tile[sl][nl * D + d];
  }
}

bool launch_dataset_gather(const DatasetGather &p, hipStream_t st) {
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64 || p.N < 1 || p.D < 2 || p.D > kMaxD) return false;
  const dim3 grid(p.b_pad / 32, (p.N + 31) / 32);
  if (p.D == kD) {
    if (p.pixels) hipLaunchKernelGGL(dataset_gather_d2_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(dataset_gather_d2_kernel<false>, grid, dim3(256), 0, st, p);
  } else {
    if (p.pixels) hipLaunchKernelGGL(dataset_gather_anyd_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(dataset_gather_anyd_kernel<false>, grid, dim3(256), 0, st, p);
  }
  return true;
}

// ------------------------------------------------------------------------------------------
// metrics of f [L][b_pad] against y [b_pad], samples [0, b): one thread per sample runs act_and_lossder (act_device.h: the
// arithmetic of the per-step metrics of a sweep), a workgroup reduces its 256 samples (the absolute error in float64) and stores
//   part[block] = {correct, sum |onehot - act(f)|, non-finite samples, samples}
// ------------------------------------------------------------------------------------------
__global__ void dataset_metrics_kernel(const float *__restrict__ f, const int *__restrict__ y, int L, int b, int b_pad, int act_fn, float T,
                                       double *__restrict__ part) {
  extern __shared__ float sh[];                     // [2][L][kDsMetricThreads]: activated f and (unused) loss derivative
  __shared__ double wsum[kDsMetricThreads / 64][4];
  const int tid = threadIdx.x, s = blockIdx.x * kDsMetricThreads + tid;
  float sa = 0.f;
  int correct = 0, nf = 0;
  if (s < b)
    act_and_lossder(f + s, b_pad, sh + tid, sh + (size_t)L * kDsMetricThreads + tid, kDsMetricThreads, L, y[s], act_fn, TNML_LOSS_MSE, T, sa,
                    correct, nf);
  double v[4] = {(double)correct, (double)sa, (double)nf, s < b ? 1.0 : 0.0};
  for (int k = 0; k < 4; ++k)
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
  if ((tid & 63) == 0)
    for (int k = 0; k < 4; ++k) wsum[tid >> 6][k] = v[k];
  __syncthreads();
  if (tid < 4) {
    double t = 0.0;
    for (int w = 0; w < kDsMetricThreads / 64; ++w) t += wsum[w][tid];
    part[(size_t)blockIdx.x * 4 + tid] = t;
  }
}

// acc[0..4) (+)= part[0..nblk) in block order; reset != 0 starts from zero
__global__ void dataset_metrics_sum_kernel(const double *__restrict__ part, int nblk, int reset, double *__restrict__ acc) {
  const int k = threadIdx.x;
  if (k >= 4) return;
  double t = reset ? 0.0 : acc[k];
  for (int i = 0; i < nblk; ++i) t += part[(size_t)i * 4 + k];
  acc[k] = t;
}

size_t dataset_metrics_lds_bytes(int L) { return (size_t)2 * L * kDsMetricThreads * sizeof(float); }

bool launch_dataset_metrics(const float *f, const int *y, int L, int b, int b_pad, int act_fn, float T, double *part, int reset, double *acc,
                            hipStream_t st) {
  const size_t lds = dataset_metrics_lds_bytes(L);
  if (b < 1 || b > b_pad || lds > 64 * 1024) return false;
  const int nblk = (b + kDsMetricThreads - 1) / kDsMetricThreads;
  hipLaunchKernelGGL(dataset_metrics_kernel, dim3(nblk), dim3(kDsMetricThreads), lds, st, f, y, L, b, b_pad, act_fn, T, part);
  hipLaunchKernelGGL(dataset_metrics_sum_kernel, dim3(1), dim3(64), 0, st, (const double *)part, nblk, reset, acc);
  return true;
}

}  // namespace tnml
