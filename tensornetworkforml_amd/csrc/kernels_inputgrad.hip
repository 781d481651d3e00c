// Input gradients (tnml_input_grad / tnml_input_grad_indices):
//   g[s][i][d] = sum_l' cot[l'][s] d f[l'][s] / d x[s][i][d]     for every sample s, site i and feature d
// f is linear in every x[s][i][:] separately, so with P_i[a] the contraction of sites 0 .. i-1, Q_i[c] that of sites i+1 .. N-1
// and T[a][d] = sum_c A_i[a][d][c] Q_i[c] (grad_chain_device.h: the two passes, their tiles, the LDS image and its bank argument):
//   g[i][d] = sum_a P_i[a] T[a][d]
// input_grad_kernel is that body with two hooks: pass B reads P_i back from the stack of pass A, and forms g from T, written
// straight into [b][N][D].
#include "tnml_internal.h"
#include "grad_chain_device.h"

namespace tnml {

__global__ __launch_bounds__(256) void input_grad_kernel(InputGradParams p) {
  const GradChainView v{p.bond, p.cores, p.labcore, p.X, p.cot, p.stack, p.cf, p.core_stride, p.b, p.b_pad, p.x_bpad, p.N, p.D, p.L, p.l_pos, p.cap, p.mb};
  const int tid = threadIdx.x, part = (tid & 63) >> 4;
  grad_chain_body(
      v,
      [&](int i, int ml, int, float *sP, const float *, int s0) {          // P_i from the stack
        if (i == 0) {
          if (tid < kGcTS) sP[tid] = 1.f;
        } else {
          const float *src = p.stack + (size_t)i * p.cap * p.b_pad + s0;
          for (int e = tid; e < ml * kGcTS; e += 256) sP[(e / kGcTS) * kGcLd + e % kGcTS] = src[(size_t)(e / kGcTS) * p.b_pad + e % kGcTS];
        }
      },
      [&](int i, int ml, int s, const float *Ts, const float *sP, int s0) {   // g[i][:] of sample s
        for (int d = 0; d < p.D; ++d) {
          float v = 0.f;
          for (int a = part; a < ml; a += 4) v = fmaf(sP[a * kGcLd + s], Ts[a * p.D + d], v);
          v += __shfl_xor(v, 16);
          v += __shfl_xor(v, 32);
          if (part == 0 && s0 + s < p.b) p.g[((size_t)(s0 + s) * p.N + i) * p.D + d] = v;
        }
      });
}

bool launch_input_grad(const InputGradParams &p, hipStream_t st) {
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % kGcTS || p.x_bpad < p.b_pad || p.mb < 1 || p.mb > p.cap || p.D < 2 || p.D > kMaxD ||
      p.l_pos < 0 || p.l_pos >= p.N)
    return false;
  const size_t lds = grad_chain_lds_bytes(p.mb, p.D, p.L, p.N);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(input_grad_kernel, dim3((p.b + kGcTS - 1) / kGcTS), dim3(256), lds, st, p);
  return true;
}

// The range-safe form: P_i and Q_i are mantissas with the exponents eP_i (the exponent stack) and eQ_i (LDS),
// and g = ldexpf(sum_a P T, eP_i + eQ_i).
__global__ __launch_bounds__(256) void input_grad_scaled_kernel(InputGradScaledParams ps) {
  const InputGradParams &p = ps.base;
  const GradChainView v{p.bond, p.cores, p.labcore, p.X, p.cot, p.stack, p.cf, p.core_stride, p.b, p.b_pad, p.x_bpad, p.N, p.D, p.L, p.l_pos, p.cap, p.mb};
  const int tid = threadIdx.x, part = (tid & 63) >> 4;
  grad_chain_body<true>(
      v,
      [&](int i, int ml, int, float *sP, const float *, int s0, const int *) {          // P_i from the stack
        if (i == 0) {
          if (tid < kGcTS) sP[tid] = 1.f;
        } else {
          const float *src = p.stack + (size_t)i * p.cap * p.b_pad + s0;
          for (int e = tid; e < ml * kGcTS; e += 256) sP[(e / kGcTS) * kGcLd + e % kGcTS] = src[(size_t)(e / kGcTS) * p.b_pad + e % kGcTS];
        }
      },
      [&](int i, int ml, int s, const float *Ts, const float *sP, int s0, const int *sEQ) {   // g[i][:] of sample s
        const int ex = (i == 0 ? 0 : ps.estack[(size_t)i * p.b_pad + s0 + s]) + sEQ[s];
        for (int d = 0; d < p.D; ++d) {
          float v = 0.f;
          for (int a = part; a < ml; a += 4) v = fmaf(sP[a * kGcLd + s], Ts[a * p.D + d], v);
          v += __shfl_xor(v, 16);
          v += __shfl_xor(v, 32);
          if (part == 0 && s0 + s < p.b) p.g[((size_t)(s0 + s) * p.N + i) * p.D + d] = ldexpf(v, ex);
        }
      },
      ps.estack);
}

bool launch_input_grad_scaled(const InputGradScaledParams &ps, hipStream_t st) {
  const InputGradParams &p = ps.base;
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % kGcTS || p.x_bpad < p.b_pad || p.mb < 1 || p.mb > p.cap || p.D < 2 || p.D > kMaxD ||
      p.l_pos < 0 || p.l_pos >= p.N || !ps.estack)
    return false;
  const size_t lds = grad_chain_lds_bytes(p.mb, p.D, p.L, p.N, true);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(input_grad_scaled_kernel, dim3((p.b + kGcTS - 1) / kGcTS), dim3(256), lds, st, ps);
  return true;
}

// ------------------------------------------------------------------------------------------
// cot[l'][s] = (l' == first maximum of f[:, s]) for s < b, 0 beyond: the rule of act_and_lossder (act_device.h)
// ------------------------------------------------------------------------------------------
__global__ void input_grad_onehot_kernel(const float *__restrict__ f, int f_bpad, int L, int b, float *__restrict__ cot, int b_pad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= b_pad) return;
  int am = -1;
  if (s < b) {
    am = 0;
    float best = f[s];
    for (int l = 0; l < L; ++l) {
      const float fv = f[(size_t)l * f_bpad + s];
      if (fv > best) { best = fv; am = l; }
    }
  }
  for (int l = 0; l < L; ++l) cot[(size_t)l * b_pad + s] = l == am ? 1.f : 0.f;
}

bool launch_input_grad_onehot(const float *f, int f_bpad, int L, int b, float *cot, int b_pad, hipStream_t st) {
  if (b < 1 || b > b_pad || b_pad > f_bpad || L < 1) return false;
  hipLaunchKernelGGL(input_grad_onehot_kernel, dim3((b_pad + 255) / 256), dim3(256), 0, st, f, f_bpad, L, b, cot, b_pad);
  return true;
}

// ------------------------------------------------------------------------------------------
// chain rule through the pixel feature map (kernels_dataset.hip): out[s][i] = sum_k g[s][i][k] dpsi_k / dp at the pixel of
// sample idx[s], site i;  psi_k(p) = coef_k sin^(D-1-k)(pi p / 2) cos^k(pi p / 2),
//   dpsi_k / dp = (pi / 2) coef_k [(D-1-k) sin^(D-2-k) cos^(k+1) - k sin^(D-k) cos^(k-1)]
// in float64 with one rounding of the sum; a term whose integer factor is 0 is dropped, not evaluated
// ------------------------------------------------------------------------------------------
__device__ inline double ig_powi(double v, int k) {
  double r = 1.0;
  for (int i = 0; i < k; ++i) r *= v;
  return r;
}

__global__ void input_grad_pixels_kernel(InputGradPixels p) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)p.b * p.N) return;
  const int s = (int)(e / p.N), i = (int)(e - (size_t)s * p.N), D = p.D;
  const double a = 3.141592653589793 * (double)p.data[(size_t)p.idx[s] * p.N + i] / 2;
  const double sn = sin(a), cs = cos(a);
  double acc = 0.0;
  for (int k = 0; k < D; ++k) {
    double t = 0.0;
    if (D - 1 - k > 0) t += (double)(D - 1 - k) * ig_powi(sn, D - 2 - k) * ig_powi(cs, k + 1);
    if (k > 0) t -= (double)k * ig_powi(sn, D - k) * ig_powi(cs, k - 1);
    acc += (double)p.g[e * D + k] * (1.5707963267948966 * p.coef[k] * t);
  }
  p.out[e] = (float)acc;
}

bool launch_input_grad_pixels(const InputGradPixels &p, hipStream_t st) {
  if (p.b < 1 || p.N < 1 || p.D < 2 || p.D > kMaxD) return false;
  const size_t n = (size_t)p.b * p.N;
  hipLaunchKernelGGL(input_grad_pixels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
  return true;
}

}  // namespace tnml
