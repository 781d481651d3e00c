// Orthogonal form about the label, compression and bond spectra (tnml_orthogonalize / tnml_compress / tnml_bond_spectra,
// DESIGN.md section 18).  Three kernels:
//   orth_load_kernel    one workgroup per site: the first core_elems floats of the site's slot -> the float64 work copy W (same slot
//                       layout), with the input check (a float that is not finite, or whose square is not a float32) on the way.
//   orth_chain_kernel   ONE workgroup walks the list of operations of a call (OrthOp): site i+1 needs the carried factor of site i,
//                       so there is nothing to spread over CUs.  Per decomposed site, everything in float64:
//                         1  M = C . A        the carried r x n factor of the previous operation is absorbed into the site (Mbuf);
//                         2  G = T^T T / tr   Gram of the side that is cut (n = the bond), T the site as a tall R x n matrix;
//                         3  cyclic Jacobi    two-sided, round-robin pairs, G and V in LDS, two LDS barriers per round;
//                         4  sort, rank rule, (compression) the cut, spectrum / discarded weight / rank of the bond;
//                         5  Q = T B          B = V_r Sigma_r^-1 in LDS, Q into the site's slot of W;
//                         6  E = Q^T Q - 1    a second Gram; B <- B (1 - E/2 + 3/8 E^2), carry <- (1 + E/2 - E^2/8) carry, and 5 again
//                                             (the CholeskyQR2 idea with the inverse square root as its series); three products at the most, each
//                                             followed by its Gram: a defect above 1e-9 after the third fails the call;
//                         7  carry = Sigma_r V_r^T / |.|_F to global memory, log |.|_F added to the running log-norm.
//                       Global hand-overs inside the workgroup are behind __syncthreads() (the full fence), LDS-only ones behind
//                       lds_barrier().  Every sum has a fixed order; there is no atomic.
//   orth_store_kernel   one workgroup per site: g W -> the float32 scratch copy of the slots, zero behind core_elems.
#include "tnml_internal.h"
#include "jacobi_device.h"

namespace tnml {

constexpr int kOrthThreads = 1024;
constexpr int kOrthLoadThreads = 256;
constexpr int kOrthMaxSweeps = 40;
constexpr int kOrthReorth = 3;              // Q products per site at the most; every one is followed by its Gram
constexpr double kOrthBig2 = 1e-18;         // a sweep without a rotation of g^2 / (a b) above this ends the iteration
constexpr double kOrthTol2 = 1e-30;         // g^2 / (a b) below which a pair is left alone
constexpr double kOrthAbs2 = kJacobiAbs * kJacobiAbs;
constexpr double kOrthReorthStop = 1e-14;   // max |Q^T Q - 1| below which Q stands
constexpr double kOrthReorthAccept = 1e-9;  // what the last product may leave (a kept ratio near the floor limits Q = T B itself to about
                                            // 1e-16 sigma_1 / sigma_r); above it the call fails with status 2
constexpr double kOrthSigmaFloor = 3e-8;      // sqrt of the Gram's own rounding: no direction below this share of sigma_1 is resolved
constexpr float kOrthInputMax = 1.8e19f;    // sqrt(FLT_MAX): the square of a larger float is not a float32

static int orth_npad(int mb) { return (mb + 1) & ~1; }
static int orth_ld(int mb) { return orth_npad(mb) | 1; }
size_t orth_chain_lds_bytes(int mb) {
  const size_t npad = (size_t)orth_npad(mb), ld = (size_t)orth_ld(mb);
  return (2 * npad * ld + kOrthThreads + 4 * npad) * sizeof(double) + 16 * sizeof(int);
}

// The rotation of jacobi_rot (jacobi_device.h) evaluated in float64 throughout, with a float64-level threshold: that helper leaves
// pairs with g^2 <= 1e-14 a b alone, which is right for a truncated float32 product and leaves |Q^T Q - 1| at 1e-7 here (measured),
// a first-order error of the carried factor's norm.  This kernel is not on the sweep's critical path: the float64 divisions stay.
__device__ inline Rot orth_rot(double a, double b, double g) {
  Rot r; r.c = 1.0; r.s = 0.0; r.t = 0.0; r.level = 0;
  const double g2 = g * g, sc = fabs(a * b);
  if (!(g2 > fmax(kOrthTol2 * sc, kOrthAbs2))) return r;        // false for g == 0 and NaN
  const double d = b - a, hyp = sqrt(fma(d, d, 4.0 * g2));
  const double t = 2.0 * g / (d + copysign(hyp, d));
  r.c = 1.0 / sqrt(fma(t, t, 1.0));
  r.s = r.c * t;
  r.t = t;
  r.level = g2 > kOrthBig2 * sc ? 2 : 1;
  return r;
}

__device__ inline int orth_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the site as a tall matrix: element (rho, kappa) at (rho / q) * sA + kappa * sK + rho % q
struct OrthView { int R, n, q, sA, sK; };
__device__ inline size_t orth_addr(const OrthView &v, int rho, int kappa) {
  return (size_t)(rho / v.q) * v.sA + (size_t)kappa * v.sK + (size_t)(rho % v.q);
}
// dir 0: the site becomes a left isometry, its right bond is cut; dir 1: right isometry, left bond
__device__ inline OrthView orth_view(int dir, int ml, int D, int mr, int Lx) {
  OrthView v;
  if (dir == 0) { v.R = ml * D * Lx; v.n = mr; v.q = Lx; v.sA = mr * Lx; v.sK = Lx; }
  else { v.R = D * mr * Lx; v.n = ml; v.q = v.R; v.sA = 0; v.sK = v.R; }
  return v;
}

// dst[i * ld + j] = scale * sum_rho T(rho, i) T(rho, j) (- 1 on the diagonal when minus_one), i, j < n.  Every element is the sum
// of P partial sums over rho = part, part + P, ... added in ascending order of part: the order depends on (n, R) alone.
__device__ void orth_gram(const double *T, const OrthView &v, double *dst, int ld, double *red, double scale, bool minus_one) {
  const int tid = threadIdx.x, n = v.n, nn = n * n;
  int P = kOrthThreads / nn;
  P = P < 1 ? 1 : (P > 16 ? 16 : P);
  if (P > v.R) P = v.R;
  if (P > 1) {
    if (tid < nn * P) {
      const int e = tid % nn, part = tid / nn, i = e / n, j = e % n;
      double s = 0.0;
      for (int rho = part; rho < v.R; rho += P) s = fma(T[orth_addr(v, rho, i)], T[orth_addr(v, rho, j)], s);
      red[tid] = s;
    }
    lds_barrier();
    if (tid < nn) {
      double s = 0.0;
      for (int part = 0; part < P; ++part) s += red[part * nn + tid];
      const int i = tid / n, j = tid % n;
      dst[i * ld + j] = s * scale - (minus_one && i == j ? 1.0 : 0.0);
    }
  } else {
    for (int e = tid; e < nn; e += kOrthThreads) {
      const int i = e / n, j = e % n;
      double s = 0.0;
      for (int rho = 0; rho < v.R; ++rho) s = fma(T[orth_addr(v, rho, i)], T[orth_addr(v, rho, j)], s);
      dst[i * ld + j] = s * scale - (minus_one && i == j ? 1.0 : 0.0);
    }
  }
  lds_barrier();
}

// sum (or maximum) of one value per thread in a fixed tree; every thread receives it
__device__ double orth_block_reduce(double x, double *red, bool want_max) {
  const int tid = threadIdx.x;
  red[tid] = x;
  lds_barrier();
  for (int w = kOrthThreads / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] = want_max ? fmax(red[tid], red[tid + w]) : red[tid] + red[tid + w];
    lds_barrier();
  }
  const double r = red[0];
  lds_barrier();
  return r;
}

__global__ __launch_bounds__(kOrthLoadThreads) void orth_load_kernel(OrthParams p) {
  const int i = blockIdx.x, tid = threadIdx.x, N = p.N;
  const int ml = i == 0 ? 1 : p.bond[i - 1], mr = i == N - 1 ? 1 : p.bond[i];
  const bool lab = i == p.l_pos;
  const size_t n = (size_t)ml * p.D * mr * (lab ? p.L : 1);
  const float *src = lab ? p.labcore : p.cores + (size_t)i * p.core_stride;
  double *dst = lab ? p.W + (size_t)N * p.core_stride : p.W + (size_t)i * p.core_stride;
  bool bad = false;
  for (size_t e = tid; e < n; e += kOrthLoadThreads) {
    const float a = src[e];
    if (!(fabsf(a) <= kOrthInputMax)) bad = true;                // NaN and infinity fail the comparison too
    dst[e] = (double)a;
  }
  if (bad) p.status[0] = 1;                                      // (every writer stores the same word)
}

__global__ __launch_bounds__(kOrthLoadThreads) void orth_store_kernel(OrthParams p) {
  const int i = blockIdx.x, tid = threadIdx.x, N = p.N;
  const int ml = i == 0 ? 1 : p.bond[i - 1], mr = i == N - 1 ? 1 : p.bond[i];
  const bool lab = i == p.l_pos;
  const size_t n = (size_t)ml * p.D * mr * (lab ? p.L : 1), cap = lab ? p.lab_elems : p.core_stride;
  const double *src = lab ? p.W + (size_t)N * p.core_stride : p.W + (size_t)i * p.core_stride;
  float *dst = lab ? p.out_lab : p.out_cores + (size_t)i * p.core_stride;
  const double g = p.result[1];
  bool bad = false;
  for (size_t e = tid; e < cap; e += kOrthLoadThreads) {
    const float a = e < n ? (float)(g * src[e]) : 0.f;
    if (!(fabsf(a) <= 3.0e38f)) bad = true;
    dst[e] = a;
  }
  if (bad) p.status[0] = 1;
}

__global__ __launch_bounds__(kOrthThreads) void orth_chain_kernel(OrthParams p) {
  extern __shared__ double orth_sh[];
  const int tid = threadIdx.x, ld = p.ld, npad = p.npad, N = p.N, D = p.D;
  double *SA = orth_sh, *SB = SA + (size_t)npad * ld, *red = SB + (size_t)npad * ld;
  double *lam = red + kOrthThreads, *sig = lam + npad, *rot = sig + npad;      // rot: (c, s) of the npad / 2 pairs of a round
  int *ord = (int *)(rot + npad);                                              // [npad] position -> column, then [npad] pairs
  int *pq = ord + npad;
  int *flags = pq + npad;                                                      // [0..2] "a large rotation" of sweep s % 3
  double *Cc = p.aux, *Cn = p.aux + p.aux_stride, *Pm = p.aux + 2 * p.aux_stride, *Pinv = p.aux + 3 * p.aux_stride;
  double *Wlab = p.W + (size_t)N * p.core_stride;

  double logn = 0.0;
  int have = 0, cr = 0, cn = 0, cdir = 0, bad = 0;

  for (int o = 0; o < p.n_ops && !bad; ++o) {
    const OrthOp op = p.ops[o];
    const int site = orth_uni(op.site), kind = orth_uni(op.kind), cut = orth_uni(op.cut);
    const bool is_lab = site == p.l_pos;
    const int Lx = is_lab ? p.L : 1;
    const int ml = site == 0 ? 1 : orth_uni(p.bond[site - 1]), mr = site == N - 1 ? 1 : orth_uni(p.bond[site]);
    double *slot = is_lab ? Wlab : p.W + (size_t)site * p.core_stride;
    const int elems = ml * D * mr * Lx;

    // 1  absorb the carried factor (cr x cn) into the index it belongs to, or copy: the site -> Mbuf with its new dimensions
    if (have) {
      const int lo = cdir == 0 ? D * mr * Lx : Lx;
      for (int e = tid; e < elems; e += kOrthThreads) {
        const int l_ = e % lo, j = (e / lo) % cr, h = e / (lo * cr);
        const double *a = slot + ((size_t)h * cn) * lo + l_, *c = Cc + (size_t)j * cn;
        double s = 0.0;
        for (int k = 0; k < cn; ++k) s = fma(c[k], a[(size_t)k * lo], s);
        p.Mbuf[e] = s;
      }
      have = 0;
    } else {
      for (int e = tid; e < elems; e += kOrthThreads) p.Mbuf[e] = slot[e];
    }
    __syncthreads();

    if (kind == kOrthCentre) {
      double s = 0.0;
      for (int e = tid; e < elems; e += kOrthThreads) s = fma(p.Mbuf[e], p.Mbuf[e], s);
      const double nrm2 = orth_block_reduce(s, red, false);
      if (!(nrm2 > 0.0) || !(nrm2 < 1e300)) { bad = 1; break; }
      const double inv = 1.0 / sqrt(nrm2);
      logn += 0.5 * log(nrm2);
      for (int e = tid; e < elems; e += kOrthThreads) slot[e] = p.Mbuf[e] * inv;
      __syncthreads();
      continue;
    }

    const int dir = kind == kOrthRight ? 0 : 1;
    const OrthView v = orth_view(dir, ml, D, mr, Lx);
    const int n = v.n, bi = dir == 0 ? site : site - 1;

    // 2  Gram of the cut side, scaled to trace 1
    for (int e = tid; e < npad * ld; e += kOrthThreads) { SA[e] = 0.0; SB[e] = 0.0; }
    if (tid < 3) flags[tid] = 0;
    lds_barrier();
    orth_gram(p.Mbuf, v, SA, ld, red, 1.0, false);
    double tr = 0.0;
    for (int j = 0; j < n; ++j) tr += SA[j * ld + j];
    if (!(tr > 0.0) || !(tr < 1e300)) { bad = 1; break; }
    lds_barrier();
    {
      const double itr = 1.0 / tr;
      for (int e = tid; e < n * n; e += kOrthThreads) SA[(e / n) * ld + e % n] *= itr;
      for (int j = tid; j < n; j += kOrthThreads) SB[j * ld + j] = 1.0;
    }
    lds_barrier();

    // 3  cyclic Jacobi: round t pairs (p, q) of the round-robin tournament; a thread owns the 2 x 2 block of G that two pairs
    //    select (J1^T . block . J2) or the two columns of one row of V, so a round needs the rotations and nothing else
    const int ne = (n + 1) & ~1, np = ne / 2;
    int sweep = 0, converged = n < 2;
    for (; sweep < kOrthMaxSweeps && !converged; ++sweep) {
      if (tid == 0) flags[(sweep + 1) % 3] = 0;
      for (int t = 0; t < ne - 1; ++t) {
        if (tid < np) {
          int a, b;
          if (tid == 0) { a = ne - 1; b = t; }
          else { a = (t + tid) % (ne - 1); b = (t - tid + (ne - 1)) % (ne - 1); }
          const int pp = a < b ? a : b, qq = a < b ? b : a;
          Rot r; r.c = 1.0; r.s = 0.0; r.level = 0;
          if (qq < n) r = orth_rot(SA[pp * ld + pp], SA[qq * ld + qq], SA[pp * ld + qq]);
          rot[2 * tid] = r.c;
          rot[2 * tid + 1] = r.s;
          pq[tid] = pp | (qq << 16);
          if (r.level == 2) flags[sweep % 3] = 1;
        }
        lds_barrier();
        for (int it = tid; it < np * np + n * np; it += kOrthThreads) {
          if (it < np * np) {
            const int k1 = it / np, k2 = it % np;
            if (k1 > k2) continue;                               // written by the thread of (k2, k1)
            const int p1 = pq[k1] & 0xffff, q1 = pq[k1] >> 16, p2 = pq[k2] & 0xffff, q2 = pq[k2] >> 16;
            const double c1 = rot[2 * k1], s1 = rot[2 * k1 + 1], c2 = rot[2 * k2], s2 = rot[2 * k2 + 1];
            const double b00 = SA[p1 * ld + p2], b01 = SA[p1 * ld + q2], b10 = SA[q1 * ld + p2], b11 = SA[q1 * ld + q2];
            // rows: p' = c p - s q, q' = s p + c q (J1^T from the left), then the same on the columns with J2
            const double r00 = c1 * b00 - s1 * b10, r01 = c1 * b01 - s1 * b11, r10 = s1 * b00 + c1 * b10, r11 = s1 * b01 + c1 * b11;
            const double n00 = c2 * r00 - s2 * r01, n01 = s2 * r00 + c2 * r01, n10 = c2 * r10 - s2 * r11, n11 = s2 * r10 + c2 * r11;
            SA[p1 * ld + p2] = n00; SA[p1 * ld + q2] = n01; SA[q1 * ld + p2] = n10; SA[q1 * ld + q2] = n11;
            if (k1 != k2) { SA[p2 * ld + p1] = n00; SA[q2 * ld + p1] = n01; SA[p2 * ld + q1] = n10; SA[q2 * ld + q1] = n11; }   // G stays symmetric bit for bit
          } else {
            const int w = it - np * np, i = w / np, k = w % np;
            const int pp = pq[k] & 0xffff, qq = pq[k] >> 16;
            const double c = rot[2 * k], s = rot[2 * k + 1];
            const double x = SB[i * ld + pp], y = SB[i * ld + qq];
            SB[i * ld + pp] = c * x - s * y;
            SB[i * ld + qq] = s * x + c * y;
          }
        }
        lds_barrier();
      }
      converged = orth_uni(flags[sweep % 3]) == 0;
    }
    if (!converged) { bad = 2; break; }

    // 4  eigenvalues in descending order (ties by column), rank rule, cut
    for (int j = tid; j < n; j += kOrthThreads) lam[j] = fmax(SA[j * ld + j], 0.0);
    lds_barrier();
    for (int j = tid; j < n; j += kOrthThreads) {
      int rank = 0;
      const double x = lam[j];
      for (int i = 0; i < n; ++i) rank += (lam[i] > x || (lam[i] == x && i < j)) ? 1 : 0;
      ord[rank] = j;
    }
    lds_barrier();
    for (int j = tid; j < n; j += kOrthThreads) sig[j] = sqrt(lam[ord[j]]);
    lds_barrier();
    const double tol = fmax(p.rank_tol, kOrthSigmaFloor) * sig[0];
    int r0 = 0;
    for (int j = 0; j < n; ++j) r0 += sig[j] > tol ? 1 : 0;
    r0 = r0 < 1 ? 1 : r0;
    r0 = r0 > v.R ? v.R : r0;
    double w0 = 0.0, s1sum = 0.0;
    for (int j = 0; j < r0; ++j) { w0 += sig[j] * sig[j]; s1sum += sig[j]; }
    int m = r0;
    if (cut == 2) {
      if (p.threshold < 1.0) {
        int idx = 0, found = 0;
        double cum = 0.0;
        for (int j = 0; j < r0; ++j) {
          cum += sig[j];
          if (!found && cum / s1sum > p.threshold) { idx = j; found = 1; }
        }
        m = idx + 1 < m ? idx + 1 : m;
      }
      m = p.m_max < m ? p.m_max : m;
    }
    m = orth_uni(m);
    r0 = orth_uni(r0);
    double wk = 0.0;
    for (int j = 0; j < m; ++j) wk += sig[j] * sig[j];
    double wd = 0.0;
    for (int j = m; j < r0; ++j) wd += sig[j] * sig[j];
    if (cut >= 1) {
      const double inw = 1.0 / sqrt(w0);
      for (int j = tid; j < p.sigma_ld; j += kOrthThreads) p.sigma_out[(size_t)bi * p.sigma_ld + j] = j < r0 ? sig[j] * inw : 0.0;
      if (tid == 0) p.discarded_out[bi] = wd / w0;
    }
    if (tid == 0) { p.bond[bi] = m; p.rank_out[bi] = r0; }
    const double nk = sqrt(wk), str = sqrt(tr);
    logn += 0.5 * log(tr) + log(nk);

    // 7 (first form)  carry[j][kappa] = sigma_j V[kappa][ord j] / nk;  5  B[kappa][j] = V[kappa][ord j] / (sigma_j sqrt(tr))
    for (int e = tid; e < m * n; e += kOrthThreads) {
      const int j = e / n, k = e % n;
      const double x = SB[k * ld + ord[j]];
      Cc[(size_t)j * n + k] = sig[j] * x / nk;
      SA[k * ld + j] = x / (sig[j] * str);
    }
    __syncthreads();
    double *B = SA, *Bo = SB;
    OrthView vq = v;                                             // Q in the slot: the cut index has m entries
    vq.n = m;
    if (dir == 0) vq.sA = m * Lx;
    for (int pass = 0;; ++pass) {
      for (int e = tid; e < v.R * m; e += kOrthThreads) {
        const int rho = e / m, j = e % m;
        double s = 0.0;
        for (int k = 0; k < n; ++k) s = fma(p.Mbuf[orth_addr(v, rho, k)], B[k * ld + j], s);
        slot[orth_addr(vq, rho, j)] = s;
      }
      __syncthreads();
      // 6  E = Q^T Q - 1 into the other LDS area
      orth_gram(slot, vq, Bo, ld, red, 1.0, true);
      double mx = 0.0;
      for (int e = tid; e < m * m; e += kOrthThreads) mx = fmax(mx, fabs(Bo[(e / m) * ld + e % m]));
      mx = orth_block_reduce(mx, red, true);
      if (!(mx <= 0.5)) { bad = 2; break; }
      if (mx <= kOrthReorthStop) break;
      if (pass == kOrthReorth - 1) {                             // no further correction: the defect stands or the call fails
        if (mx > kOrthReorthAccept) bad = 2;
        break;
      }
      // P = 1 - E/2 + 3/8 E^2, Pinv = 1 + E/2 - E^2/8 to global memory
      for (int e = tid; e < m * m; e += kOrthThreads) {
        const int i = e / m, j = e % m;
        double e2 = 0.0;
        for (int k = 0; k < m; ++k) e2 = fma(Bo[i * ld + k], Bo[k * ld + j], e2);
        const double ee = Bo[i * ld + j], id = i == j ? 1.0 : 0.0;
        Pm[e] = id - 0.5 * ee + 0.375 * e2;
        Pinv[e] = id + 0.5 * ee - 0.125 * e2;
      }
      __syncthreads();
      // B <- B P (into the other area), carry <- Pinv carry (into the other buffer)
      for (int e = tid; e < n * m; e += kOrthThreads) {
        const int k = e / m, j = e % m;
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = fma(B[k * ld + i], Pm[i * m + j], s);
        Bo[k * ld + j] = s;                                      // (E was consumed before the fence above)
      }
      for (int e = tid; e < m * n; e += kOrthThreads) {
        const int j = e / n, k = e % n;
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = fma(Pinv[j * m + i], Cc[(size_t)i * n + k], s);
        Cn[(size_t)j * n + k] = s;
      }
      __syncthreads();
      { double *t_ = B; B = Bo; Bo = t_; }
      { double *t_ = Cc; Cc = Cn; Cn = t_; }
    }
    if (bad) break;
    have = 1; cr = m; cn = n; cdir = dir == 0 ? 0 : 1;
  }

  if (tid == 0) {
    if (bad) p.status[0] = bad == 1 ? 1 : 2;
    p.result[0] = logn;
    p.result[1] = exp(logn / (double)N);
  }
}

bool launch_orth(const OrthParams &p, int mb, hipStream_t st) {
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N || mb < 1 || p.n_ops < 1) return false;
  const size_t lds = orth_chain_lds_bytes(mb);
  if (lds > 160 * 1024 || mb > 0x7fff) return false;
  OrthParams q = p;
  q.npad = orth_npad(mb);
  q.ld = orth_ld(mb);
  if ((size_t)mb * mb > q.aux_stride) return false;
  hipLaunchKernelGGL(orth_load_kernel, dim3(q.N), dim3(kOrthLoadThreads), 0, st, q);
  hipLaunchKernelGGL(orth_chain_kernel, dim3(1), dim3(kOrthThreads), lds, st, q);
  hipLaunchKernelGGL(orth_store_kernel, dim3(q.N), dim3(kOrthLoadThreads), 0, st, q);
  return true;
}

}  // namespace tnml
