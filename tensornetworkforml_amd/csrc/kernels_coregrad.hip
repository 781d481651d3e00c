// Core gradients (tnml_core_grad / tnml_core_grad_indices): the derivative of sum_s cf[s],
// cf[s] = sum_l' cot[l'][s] f[l'][s], with respect to every core at once.  With P_i[s][a] the contraction of sites 0 .. i-1 and
// Q_i[s][c] that of sites i+1 .. N-1 of sample s (P_0 = Q_{N-1} = 1; the chain that has passed the label site l carries cot):
//   G_i[a][d][c]     = sum_s P_i[s][a] x_i[s][d] Q_i[s][c]                    i != l
//   G_l[a][d][c][l'] = sum_s cot[l'][s] P_l[s][a] x_l[s][d] Q_l[s][c]         (P_l and Q_l are free of cot)
// Two kernels per chunk of samples:
//   core_grad_chain_kernel   the two-pass body of grad_chain_device.h (tiles, LDS image and bank argument are there), which
//                            input_grad_kernel runs too: pass A stores P_1 .. P_{N-1} to one HBM stack [N][cap][b_pad], this
//                            kernel's hook in pass B stores Q_{N-2} .. Q_0 to a second one; the body leaves cf.
//   core_grad_reduce_kernel  the sum over samples, parallel over sites: for a site one GEMM with K = samples,
//                            (P_i (x) x_i)^T [ml D x samples] . Q_i^T [samples x mr], at the label site one per label slice with
//                            cot[l'][s] folded into x.  Grid (site, block of output tiles, label slice).  A wave owns two
//                            16 x 16 output tiles side by side (one A operand, two B operands, v_mfma_f32_16x16x4_f32) and walks
//                            ALL samples of the chunk in ascending order, 64 at a time through LDS; the accumulators of a chunk
//                            after the first start from G, so that every element is one fixed left-to-right sum whatever the
//                            chunk size.  No atomics, no split of the sample axis.
//
// LDS of the reduction (floats): P tile mb x 65, Q tile mb x 65, x tile 64 x D.  The stacks are sample-contiguous, so the tiles are
// filled by coalesced loads (a thread's element e -> row e / 64, sample e % 64: 64 consecutive banks per row, conflict-free
// writes).  ds_read_b32 banks over 32 dwords per 32-lane half (lanes 0-31 = k-quarters 0 and 1 of an operand fetch):
//   P tile, row stride 65: a lane reads row a = (row of the output tile) / D at sample k: bank (a + k) mod 32.  The 16 lanes of a
//     k-quarter touch at most 16 consecutive a (lanes with the same a read one address: broadcast), the second quarter the same
//     rows one sample on: at most 2-way.  At a row stride of 64 all rows of a quarter would share one bank.
//   Q tile, row stride 65: 16 consecutive rows c at sample k, bank (c + k) mod 32: the same argument, at most 2-way.
//   x tile: a half reads two samples x D features, at most 2 D <= 16 distinct addresses with 2 D consecutive banks: conflict-free.
#include "tnml_internal.h"
#include "grad_chain_device.h"

namespace tnml {

typedef float cg_f4 __attribute__((ext_vector_type(4)));

constexpr int kCgTS = kGcTS;       // samples per LDS tile of the reduction: the chain kernel's 64 per workgroup
constexpr int kCgLdR = 65;         // reduction: row stride of the P and Q tiles

// ------------------------------------------------------------------------------------------
// chain kernel: the shared body; pass B stores Q_{N-2} .. Q_0 to the second stack, and T has no other use
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void core_grad_chain_kernel(CoreGradParams p) {
  const GradChainView v{p.tab, p.cores, p.labcore, p.X, p.cot, p.stackP, p.cf, p.core_stride, p.b, p.b_pad, p.x_bpad, p.N, p.D, p.L, p.l_pos, p.cap, p.mb};
  const int tid = threadIdx.x;
  grad_chain_body(
      v,
      [&](int i, int, int mr, const float *, const float *sQ, int s0) {     // Q_i to the second stack
        if (i < p.N - 1) {
          float *dst = p.stackQ + (size_t)i * p.cap * p.b_pad + s0;
          for (int e = tid; e < mr * kGcTS; e += 256) dst[(size_t)(e / kGcTS) * p.b_pad + e % kGcTS] = sQ[(e / kGcTS) * kGcLd + e % kGcTS];
        }
      },
      [](int, int, int, const float *, const float *, int) {});
}

// The range-safe form: stackP keeps the mantissas of P_i, the second stack receives ldexpf(Q_i, eP_i + eQ_i), so
// that the reduction kernel below, unchanged, sums the true P_i x_i Q_i wherever that is representable.
__global__ __launch_bounds__(256) void core_grad_chain_scaled_kernel(CoreGradScaledParams ps) {
  const CoreGradParams &p = ps.base;
  const GradChainView v{p.tab, p.cores, p.labcore, p.X, p.cot, p.stackP, p.cf, p.core_stride, p.b, p.b_pad, p.x_bpad, p.N, p.D, p.L, p.l_pos, p.cap, p.mb};
  const int tid = threadIdx.x;
  grad_chain_body<true>(
      v,
      [&](int i, int ml, int mr, const float *, const float *sQ, int s0, const int *sEQ) {     // Q_i to the second stack
        if (i == p.N - 1) {
          // the reduction takes Q_{N-1} as the scalar 1 and not from the second stack: the last site's exponent goes into P_{N-1},
          // which no later step of this kernel reads (this workgroup wrote the slot and the exponents in pass A)
          float *slot = p.stackP + (size_t)i * p.cap * p.b_pad + s0;
          const int *eP = ps.estack + (size_t)i * p.b_pad + s0;
          for (int e = tid; e < ml * kGcTS; e += 256) {
            float *v = slot + (size_t)(e / kGcTS) * p.b_pad + e % kGcTS;
            *v = ldexpf(*v, eP[e % kGcTS]);
          }
        }
        if (i < p.N - 1) {
          float *dst = p.stackQ + (size_t)i * p.cap * p.b_pad + s0;
          const int *eP = ps.estack + (size_t)i * p.b_pad + s0;
          for (int e = tid; e < mr * kGcTS; e += 256) {
            const int s = e % kGcTS;
            dst[(size_t)(e / kGcTS) * p.b_pad + s] = ldexpf(sQ[(e / kGcTS) * kGcLd + s], (i == 0 ? 0 : eP[s]) + sEQ[s]);
          }
        }
      },
      [](int, int, int, const float *, const float *, int, const int *) {}, ps.estack);
}

static bool core_grad_geometry_ok(const CoreGradParams &p) {
  return p.b >= 1 && p.b <= p.b_pad && p.b_pad % kCgTS == 0 && p.x_bpad >= p.b_pad && p.mb >= 1 && p.mb <= p.cap && p.D >= 2 && p.D <= kMaxD &&
         p.N >= 2 && p.L >= 1 && p.l_pos >= 0 && p.l_pos < p.N;
}

bool launch_core_grad_chain_scaled(const CoreGradScaledParams &ps, hipStream_t st) {
  const CoreGradParams &p = ps.base;
  if (!core_grad_geometry_ok(p) || !ps.estack) return false;
  const size_t lds = grad_chain_lds_bytes(p.mb, p.D, p.L, p.N, true);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(core_grad_chain_scaled_kernel, dim3((p.b + kCgTS - 1) / kCgTS), dim3(256), lds, st, ps);
  return true;
}

bool launch_core_grad_chain(const CoreGradParams &p, hipStream_t st) {
  if (!core_grad_geometry_ok(p)) return false;
  const size_t lds = grad_chain_lds_bytes(p.mb, p.D, p.L, p.N);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(core_grad_chain_kernel, dim3((p.b + kCgTS - 1) / kCgTS), dim3(256), lds, st, p);
  return true;
}

// ------------------------------------------------------------------------------------------
// reduction kernel: G_i (+)= (P_i (x) x_i [cot])^T . Q_i^T over the samples of the chunk
// ------------------------------------------------------------------------------------------
size_t core_grad_reduce_lds_bytes(int mb, int D) { return (2 * (size_t)mb * kCgLdR + (size_t)kCgTS * D) * sizeof(float); }

int core_grad_reduce_blocks(int mb, int D) {
  const int pairs = ((mb * D + 15) / 16) * (((mb + 15) / 16 + 1) / 2);
  return (pairs + 3) / 4;
}

__global__ __launch_bounds__(256) void core_grad_reduce_kernel(CoreGradParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int i = blockIdx.x, sl = blockIdx.z, D = p.D, N = p.N;
  const bool label = i == p.l_pos;
  if (sl > 0 && !label) return;                              // only the label site has more than one slice
  const int ml = i == 0 ? 1 : p.tab[i - 1], mr = i == N - 1 ? 1 : p.tab[i];
  const int J = ml * D, CP = ((mr + 15) / 16 + 1) / 2, npairs = ((J + 15) / 16) * CP;
  if ((int)blockIdx.y * 4 >= npairs) return;                 // (the grid is sized for the largest bond)
  float *sP = (float *)smem_raw;                             // [ml][kCgLdR]
  float *sQ = sP + (size_t)p.mb * kCgLdR;                    // [mr][kCgLdR]
  float *sX = sQ + (size_t)p.mb * kCgLdR;                    // [64][D]: x, at the label site x cot[sl]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, part = lane >> 4;
  const int q = blockIdx.y * 4 + wave;                       // this wave's pair of tiles: row tile q / CP, column tiles 2 (q % CP) + {0, 1}
  const bool active = q < npairs;
  const int row0 = (q / CP) * 16, c0 = (q % CP) * 32 + r16, c1 = c0 + 16;
  const int j = row0 + r16, ja = j / D, jd = j - ja * D;     // the row of the A operand this lane supplies: (a, d)
  const int nL = label ? p.L : 1;
  float *Gi = p.G + (size_t)p.tab[N + i] + sl;
  cg_f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};   // acc[r]: row row0 + 4 part + r, column c0 / c1
  if (active && !p.first) {
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * part + r;
      if (row < J && c0 < mr) acc0[r] = Gi[((size_t)row * mr + c0) * nL];
      if (row < J && c1 < mr) acc1[r] = Gi[((size_t)row * mr + c1) * nL];
    }
  }
  const float *srcP = p.stackP + (size_t)i * p.cap * p.b_pad, *srcQ = p.stackQ + (size_t)i * p.cap * p.b_pad;
  const float *srcX = p.X + (size_t)i * p.x_bpad * D, *cot = p.cot + (size_t)sl * p.b_pad;
  for (int s0 = 0; s0 < p.b; s0 += kCgTS) {
    __syncthreads();                                         // the tiles of the previous 64 samples are free
    if (i == 0) { if (tid < kCgTS) sP[tid] = 1.f; }
    else for (int e = tid; e < ml * kCgTS; e += 256) sP[(e / kCgTS) * kCgLdR + e % kCgTS] = srcP[(size_t)(e / kCgTS) * p.b_pad + s0 + e % kCgTS];
    if (i == N - 1) { if (tid < kCgTS) sQ[tid] = 1.f; }
    else for (int e = tid; e < mr * kCgTS; e += 256) sQ[(e / kCgTS) * kCgLdR + e % kCgTS] = srcQ[(size_t)(e / kCgTS) * p.b_pad + s0 + e % kCgTS];
    for (int e = tid; e < kCgTS * D; e += 256) {
      const float xv = srcX[(size_t)s0 * D + e];
      sX[e] = label ? xv * cot[s0 + e / D] : xv;
    }
    __syncthreads();
    if (!active) continue;
    for (int k = part; k < kCgTS; k += 4) {
      const float av = j < J ? sP[ja * kCgLdR + k] * sX[k * D + jd] : 0.f;
      const float b0 = c0 < mr ? sQ[c0 * kCgLdR + k] : 0.f, b1 = c1 < mr ? sQ[c1 * kCgLdR + k] : 0.f;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc1, 0, 0, 0);
    }
  }
  if (!active) return;
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * part + r;
    if (row < J && c0 < mr) Gi[((size_t)row * mr + c0) * nL] = acc0[r];
    if (row < J && c1 < mr) Gi[((size_t)row * mr + c1) * nL] = acc1[r];
  }
}

bool launch_core_grad_reduce(const CoreGradParams &p, hipStream_t st) {
  if (!core_grad_geometry_ok(p)) return false;
  const size_t lds = core_grad_reduce_lds_bytes(p.mb, p.D);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(core_grad_reduce_kernel, dim3(p.N, core_grad_reduce_blocks(p.mb, p.D), p.L), dim3(256), lds, st, p);
  return true;
}

}  // namespace tnml
