// CPU stand-in for the HIP runtime and RCCL, for ONE purpose: running the HOST side of this library (tnml_api.hip, the api_*.hip files and the launch
// wrappers of kernels_*.hip, compiled `--cuda-host-only -fsanitize=address,undefined`) on a machine without a GPU, so that the
// planning of whole sweeps -- strides, slot offsets, buffer sizing, the pipelined / classic / persistent state machine -- runs under
// AddressSanitizer and UBSan (GPU sanitizers are not available on this pool).  Nothing here computes: kernels are never executed.
// What it does instead:
//   * "device memory" comes from one reserved address range with unmapped gaps between allocations; every copy / memset the host
//     code issues is checked against the allocation registry;
//   * every launch is checked: grid, block and dynamic LDS against the gfx950 limits, and -- for the kernels that carry the sweep
//     (typed decoders below) -- every pointer of their argument blocks together with the extent the kernel will touch;
//   * with TNML_SAN_TRACE=<file>, every runtime call is written there as one line of text, in call order: launches with every argument
//     (the planners' structs field by field, record arrays and site tables on continuation lines), copies, memsets, all-reduces, event
//     and stream calls; device pointers as offsets from the arena base, streams and events by their order of creation.
//   * san_stub_fail_alloc(n) makes the n-th allocation call from now on fail once: the mains fail every allocation of a call in turn
//     (san/fail_each.h) and the final "live allocations" count, with LeakSanitizer behind it, shows what a failed call left behind.
// A violation prints what and where and aborts.  Test infrastructure only; never linked into libtnml_hip.so.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <sys/mman.h>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <cxxabi.h>
#include "../tnml_internal.h"
#include "../wide_pipe_device.h"
#include "../grad_chain_device.h"

using namespace tnml;

namespace san {
static char *g_base = nullptr;
static size_t g_used = 0;
static constexpr size_t kArena = (size_t)1 << 38, kGap = (size_t)1 << 20;
// (function-local: kernels register themselves from static constructors that may run before this file's)
static std::map<uintptr_t, size_t> &alloc_map() { static auto *m = new std::map<uintptr_t, size_t>; return *m; }          // base -> bytes (live)
static std::map<const void *, std::string> &kernel_map() { static auto *m = new std::map<const void *, std::string>; return *m; }
static std::map<std::string, long> &launch_map() { static auto *m = new std::map<std::string, long>; return *m; }
#define g_alloc alloc_map()
#define g_kernels kernel_map()
#define g_launches launch_map()
static long g_checked_ptrs = 0, g_allreduces = 0;
static const PersistStep *g_last_persist = nullptr;      // records and step count of the last persistent launch (san_stub_last_persist)
static int g_last_persist_n = 0;
// injected failure: the allocation call (hipMalloc / hipHostMalloc) with this number returns hipErrorOutOfMemory, once (0: none)
static long g_alloc_calls = 0, g_fail_call = 0;
static bool alloc_fails() {
  if (++g_alloc_calls != g_fail_call) return false;
  g_fail_call = 0;
  return true;
}
static const char *g_ctx = "";

[[noreturn]] static void die(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "san-stub VIOLATION [%s]: ", g_ctx);
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  abort();
}
static bool in_arena(const void *p) { return g_base && (const char *)p >= g_base && (const char *)p < g_base + kArena; }
// [p, p + bytes) inside ONE live allocation
static void need(const void *p, size_t bytes, const char *what) {
  ++g_checked_ptrs;
  if (!p) die("%s: null pointer (%zu bytes wanted)", what, bytes);
  if (!in_arena(p)) die("%s: %p is not device memory", what, p);
  auto it = g_alloc.upper_bound((uintptr_t)p);
  if (it == g_alloc.begin()) die("%s: %p below every allocation", what, p);
  --it;
  const uintptr_t lo = it->first, hi = lo + it->second;
  if ((uintptr_t)p + bytes > hi) die("%s: [%p, +%zu) leaves its allocation [%p, +%zu) by %zu bytes", what, p, bytes, (void *)lo, it->second, (uintptr_t)p + bytes - hi);
}
static void opt(const void *p, size_t bytes, const char *what) { if (p) need(p, bytes, what); }
// every 8-byte word of an argument block that points into the device range must point into a live allocation
static void scan(const void *blk, size_t bytes, const char *what) {
  for (size_t o = 0; o + 8 <= bytes; o += 8) {
    void *v;
    memcpy(&v, (const char *)blk + o, 8);
    if (in_arena(v)) need(v, 1, what);
  }
}
static size_t view_extent(const CoreView &v, int tail) {     // elements reached through the strides (+ tail for the label index)
  return (size_t)(v.n_in - 1) * v.s_in + (size_t)(kD - 1) * v.s_d + (size_t)(v.n_out - 1) * v.s_out + tail;
}

static void check_wide(const WideParams &p, int nblk, bool f_only = false) {
  const size_t bp = p.b_pad;
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64) die("WideParams: b %d b_pad %d", p.b, p.b_pad);
  scan(&p, sizeof p, "WideParams");
  if (f_only) {                            // f from the previous step's updated tensor: the "previous" operands only
    opt(p.Hprev, (size_t)p.hp * bp * 4, "WideParams.Hprev"); opt(p.Gprev, (size_t)p.gp * bp * 4, "WideParams.Gprev");
    need(p.x_km1, bp * kD * 4, "WideParams.x_km1"); need(p.x_k, bp * kD * 4, "WideParams.x_k");
    need(p.Bprev, (size_t)p.hp * kD * kD * p.gp * p.L * 4, "WideParams.Bprev"); need(p.f, (size_t)p.L * bp * 4, "WideParams.f");
    if ((size_t)nblk * kTS != bp) die("f_only grid %d x %d samples != b_pad %zu", nblk, kTS, bp);
    return;
  }
  opt(p.x_km1, bp * kD * 4, "WideParams.x_km1"); need(p.x_k, bp * kD * 4, "WideParams.x_k"); need(p.x_kp1, bp * kD * 4, "WideParams.x_kp1");
  if (p.do_ext && !p.first_ext) need(p.Hprev, (size_t)p.hp * bp * 4, "WideParams.Hprev");
  opt(p.Hcur, (size_t)p.h * bp * 4, "WideParams.Hcur");
  if (p.do_f) { opt(p.Gprev, (size_t)p.gp * bp * 4, "WideParams.Gprev"); need(p.Bprev, (size_t)p.hp * kD * kD * p.gp * p.L * 4, "WideParams.Bprev"); }
  opt(p.Gcur, (size_t)p.g * bp * 4, "WideParams.Gcur");
  if (p.do_ext) need(p.ext_core.base, view_extent(p.ext_core, 1) * 4, "WideParams.ext_core");
  need(p.y, bp * 4, "WideParams.y"); need(p.f, (size_t)p.L * bp * 4, "WideParams.f");
  if (p.slabs) {
    if (p.bsize != p.h * kD * kD * p.g * p.L) die("WideParams.bsize %d != h D D g L", p.bsize);
    if (p.slab_stride < p.bsize + kMetricSlots) die("WideParams.slab_stride %d < bsize + tail %d", p.slab_stride, p.bsize + kMetricSlots);
    need(p.slabs, (size_t)nblk * p.slab_stride * 4, "WideParams.slabs");
  }
}
struct BigExtArgs { const float *Eprev, *x_km1, *x_k; CoreView A; int b_pad; float *Ecur, *Pk; };     // kernels_big.hip
static void check_big_ext(const BigExtArgs &a, size_t shm) {
  const CoreView &A = a.A;
  const size_t bp = (size_t)a.b_pad;
  need(a.Eprev, (size_t)A.n_in * bp * 4, "big_ext: E_{k-1}");
  need(a.x_km1, bp * kD * 4, "big_ext: x_{k-1}"); need(a.x_k, bp * kD * 4, "big_ext: x_k");
  need(A.base, view_extent(A, 1) * 4, "big_ext: core");
  need(a.Ecur, (size_t)A.n_out * bp * 4, "big_ext: E_k"); need(a.Pk, (size_t)kD * A.n_out * bp * 4, "big_ext: P'_k");
  if (shm < (size_t)A.n_in * kD * ((A.n_out + 3) & ~3) * 4) die("big_ext: %zu bytes of LDS for a %d x %d x %d core", shm, A.n_in, kD, A.n_out);
}
static void check_narrow(const NarrowParams &p) {
  scan(&p, sizeof p, "NarrowParams");
  if (p.bsize != p.h * kD * kD * p.g * p.L) die("NarrowParams.bsize %d != h D D g L (%d %d %d)", p.bsize, p.h, p.g, p.L);
  const int rows = p.h * kD, cols = kD * p.g * p.L;     // (right sweep orientation; the kept rank bound is symmetric)
  if (p.m < 1 || p.m > (rows < cols ? rows : cols) * p.L) die("NarrowParams.m %d for a %d x %d tensor", p.m, rows, cols);
  if (!p.pipe) opt(p.red, (size_t)(p.bsize + kMetricSlots) * 4, "NarrowParams.red");
  if (!p.Bdirect) { need(p.lab.base, view_extent(p.lab, p.L) * 4, "NarrowParams.lab"); need(p.pl.base, view_extent(p.pl, 1) * 4, "NarrowParams.pl"); }
  else need(p.Bdirect, (size_t)p.bsize * 4, "NarrowParams.Bdirect");
  opt(p.Nh, (size_t)p.h * p.h * 8, "NarrowParams.Nh"); opt(p.Ng, (size_t)p.g * p.g * 8, "NarrowParams.Ng");
  need(p.Bnew, (size_t)p.bsize * 4, "NarrowParams.Bnew");
  if (!p.stop_after_update) {
    need(p.out_behind, ((size_t)(p.h - 1) * p.ob_s_h + (size_t)(kD - 1) * p.ob_s_d + (size_t)(p.m - 1) * p.ob_s_m + 1) * 4, "NarrowParams.out_behind");
    need(p.out_ahead, ((size_t)(p.m - 1) * p.oa_s_m + (size_t)(kD - 1) * p.oa_s_d + (size_t)(p.g - 1) * p.oa_s_g + p.L) * 4, "NarrowParams.out_ahead");
    opt(p.Nh_new, (size_t)p.m * p.m * 8, "NarrowParams.Nh_new");
  }
  if (p.zpoll_flag) need(p.zpoll_flag, 4, "NarrowParams.zpoll_flag");
  if (p.done_flag) need(p.done_flag, 4, "NarrowParams.done_flag");
  if (p.m_out) { need(p.m_out, 4, "NarrowParams.m_out"); memcpy(p.m_out, &p.m, 4); }     // the adaptive rank the kernel would decide: the cap
  opt(p.metrics, 2 * 4, "NarrowParams.metrics"); opt(p.counters, 4 * 8, "NarrowParams.counters") /* null in compute_L2_reg alone: the kernel tests it */; need(p.status, 4, "NarrowParams.status");
  if (p.pipe) {
    need(p.zred, (size_t)(p.zsize + kMetricSlots) * 4, "NarrowParams.zred");
    // (persistent sweep: the helper workgroups contract Z with the published behind core; the update workgroup reads the metric tail)
    if (!p.z_first && !p.persist) need(p.zcore.base, view_extent(p.zcore, 1) * 4, "NarrowParams.zcore");
    opt(p.flag, 4, "NarrowParams.flag");
  }
  if (p.fused) {
    opt(p.slabs, (size_t)p.nslabs * p.slab_stride * 4, "NarrowParams.slabs");
    opt(p.prepB, (size_t)p.bsize * 4, "NarrowParams.prepB"); opt(p.prepG, (size_t)p.bsize * 8, "NarrowParams.prepG");
    need(p.sync, 4, "NarrowParams.sync");
  }
  if (p.persist) {
    need(p.prepB, (size_t)p.bsize * 4, "NarrowParams.prepB (persistent)"); need(p.prepG, (size_t)p.bsize * 8, "NarrowParams.prepG (persistent)");
    need(p.pready, 4, "NarrowParams.pready"); need(p.aflag, 4, "NarrowParams.aflag"); need(p.coreflag, 4, "NarrowParams.coreflag"); need(p.abort_flag, 4, "NarrowParams.abort_flag");
    need(p.Apub, persist_pub_doubles(kD * p.h * p.m, p.m) * 8, "NarrowParams.Apub");
  }
}
static void check_pipe(const WidePipeParams &w) {
  scan(&w, sizeof w, "WidePipeParams");
  const size_t bp = w.b_pad;
  if (w.b < 1 || w.b > w.b_pad || w.b_pad % 64 || w.ntiles != w.b_pad / kTS) die("WidePipeParams: b %d b_pad %d ntiles %d", w.b, w.b_pad, w.ntiles);
  if (!w.first) {
    need(w.x_j, bp * kD * 4, "WidePipeParams.x_j");
    if (w.do_ext) {
      need(w.Ecur, (size_t)w.hj * bp * 4, "WidePipeParams.Ecur (written)");
      need(w.x_jm1, bp * kD * 4, "WidePipeParams.x_jm1");
      if (!w.first_ext) need(w.Eprev, (size_t)w.hprev * bp * 4, "WidePipeParams.Eprev");
      need(w.ext_core.base, view_extent(w.ext_core, 1) * 4, "WidePipeParams.ext_core");
    } else opt(w.Ecur, (size_t)w.hj * bp * 4, "WidePipeParams.Ecur (read)");
    if (w.do_f) { opt(w.Gj, (size_t)w.gj * bp * 4, "WidePipeParams.Gj"); need(w.Bnew, (size_t)w.hj * kD * kD * w.gj * w.L * 4, "WidePipeParams.Bnew"); }
  }
  need(w.x_jp1, bp * kD * 4, "WidePipeParams.x_jp1");
  need(w.y, bp * 4, "WidePipeParams.y"); need(w.f, (size_t)w.L * bp * 4, "WidePipeParams.f"); need(w.status, 4, "WidePipeParams.status");
  if (w.do_z) {
    need(w.x_jp2, bp * kD * 4, "WidePipeParams.x_jp2");
    opt(w.Gn, (size_t)w.gn * bp * 4, "WidePipeParams.Gn");
    const int nI = w.first ? 1 : w.hj * kD;
    if (w.zsize != nI * kD * kD * w.gn * w.L) die("WidePipeParams.zsize %d != nI D D gn L (%d %d %d)", w.zsize, nI, w.gn, w.L);
    if (w.slab_stride < w.zsize + kMetricSlots) die("WidePipeParams.slab_stride %d < zsize + tail", w.slab_stride);
    need(w.slabs, (size_t)w.nwide * w.slab_stride * 4, "WidePipeParams.slabs");
    if (!w.one_level && !w.slice_red) need(w.gslabs, (size_t)w.ngroups * w.slab_stride * 4, "WidePipeParams.gslabs");
    if (w.slice_red) {
      // the slice plan of a persistent record: whole 128-byte lines per run, every 16-byte element in exactly one run, no more
      // reducers than workgroups, the group sums of a run inside the workgroup's LDS, both words inside the step's counter block
      const int n4 = (w.zsize + kMetricSlots + 3) / 4;
      if (!w.persist || w.one_level) die("WidePipeParams: slice reduction on a record with persist %d one_level %d", w.persist, w.one_level);
      if (w.slice_S < 8 || w.slice_S % 8) die("WidePipeParams.slice_S %d is no multiple of 8", w.slice_S);
      if (w.slice_R < 1 || w.slice_R > w.nwide || w.slice_R > (n4 + w.slice_S - 1) / w.slice_S) die("WidePipeParams.slice_R %d for %d workgroups, %d elements", w.slice_R, w.nwide, n4);
      if (w.slice_R < w.nwide && w.slice_R * w.slice_S < n4) die("WidePipeParams: %d reducers x %d elements < %d and not capped", w.slice_R, w.slice_S, n4);
      if (w.ngroups < 1 || w.ngroups > kPipeGroupMax || w.gsz * w.ngroups < w.nwide) die("WidePipeParams: %d groups of %d for %d workgroups", w.ngroups, w.gsz, w.nwide);
      if ((size_t)w.ngroups * w.slice_S * 16 > wide_pipe_lds_bytes(w) - 16) die("WidePipeParams: group sums of a run beyond the workgroup's LDS");
      if ((size_t)w.nwide * w.slab_stride * 4 >= ((size_t)1 << 31)) die("WidePipeParams: the partials of %d workgroups beyond a 31-bit offset", w.nwide);
      if ((size_t)n4 * 4 > (size_t)w.slab_stride) die("WidePipeParams: %d 16-byte elements beyond the slab stride %d", n4, w.slab_stride);
      need(w.sarrive, 4, "WidePipeParams.sarrive"); need(w.sdone, 4, "WidePipeParams.sdone");
      if (w.sarrive != w.gcnt + kPstArriveWord || w.sdone != w.gcnt + kPstDoneWord) die("WidePipeParams: slice words outside the step's counter block");
    }
    need(w.zred, (size_t)(w.zsize + kMetricSlots) * 4, "WidePipeParams.zred");
    need(w.gcnt, (size_t)(w.ngroups > 0 ? w.ngroups : 1) * 4, "WidePipeParams.gcnt"); need(w.tcnt, 4, "WidePipeParams.tcnt");
    if (w.nwide * w.tiles_per_wg < w.ntiles) die("WidePipeParams: %d workgroups x %d tiles < %d tiles", w.nwide, w.tiles_per_wg, w.ntiles);
  }
  if (w.wait_flag) need(w.flag, 4, "WidePipeParams.flag");
}
static void check_chain(const ChainSite *sites, int n, const float *cores, const float *lab, const float *X, float *env, float *f, int b_pad, int L) {
  need(sites, (size_t)n * sizeof(ChainSite), "chain table");
  for (int i = 0; i < n; ++i) {
    const ChainSite &c = sites[i];
    const size_t ext = (size_t)(c.n_in - 1) * c.s_in + (size_t)(kD - 1) * c.s_d + (size_t)(c.n_out - 1) * c.s_out + 1;
    need((c.is_label ? lab : cores) + c.core_off, ext * 4, "chain core");
    need(X + (size_t)c.x_site * b_pad * kD, (size_t)b_pad * kD * 4, "chain features");
    if (c.env_out_off >= 0) { if (env) need(env + c.env_out_off, (size_t)c.n_out * b_pad * 4, "chain environment slot"); }
    else need(f, (size_t)(c.is_label ? L : c.n_out) * b_pad * 4, c.is_label ? "chain f" : "chain: last environment of a half-chain");
    if (i + 1 < n && sites[i + 1].n_in != c.n_out) die("chain: site %d produces %d, site %d takes %d", i, c.n_out, i + 1, sites[i + 1].n_in);
  }
}

// the label site between two environments (kernels_meet.hip): every operand with the extent the kernel touches
static void check_meet(const MeetParams &p, dim3 g, dim3 b, size_t shm) {
  scan(&p, sizeof p, "MeetParams");
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64) die("MeetParams: b %d b_pad %d", p.b, p.b_pad);
  if (p.D < 2 || p.D > kMaxD || p.L < 1 || p.ml < 1 || p.mr < 1) die("MeetParams: D %d L %d ml %d mr %d", p.D, p.L, p.ml, p.mr);
  if (b.x != 64 || (size_t)g.x * 64 != (size_t)p.b_pad) die("label_meet_kernel: grid %u x %u lanes != b_pad %d", g.x, b.x, p.b_pad);
  if (p.rows_per_chunk < 1 || p.rows_per_chunk > p.ml) die("MeetParams.rows_per_chunk %d for %d rows", p.rows_per_chunk, p.ml);
  const size_t bp = p.b_pad;
  if (shm < ((size_t)p.mr * 64 + (size_t)p.rows_per_chunk * p.D * p.mr * p.L) * 4) die("label_meet_kernel: %zu bytes of LDS for %d rows of %d x %d x %d and a tile of %d", shm, p.rows_per_chunk, p.D, p.mr, p.L, p.mr);
  need(p.Lenv, (size_t)p.ml * bp * 4, "MeetParams.Lenv"); need(p.Renv, (size_t)p.mr * bp * 4, "MeetParams.Renv");
  need(p.x, bp * p.D * 4, "MeetParams.x"); need(p.core, (size_t)p.ml * p.D * p.mr * p.L * 4, "MeetParams.core");
  need(p.f, (size_t)p.L * bp * 4, "MeetParams.f");
}

// What InputGradParams and CoreGradParams share, as the view either kernel fills (grad_chain_device.h), under the name `blk` of the
// block: the geometry, the extents of X, cot and cf and, for a launch of the two-pass chain (`kernel` names it;
// nullptr: the reduction), its grid, block and LDS.
static void check_grad_geometry(const GradChainView &p, const char *blk, const char *kernel, dim3 g, dim3 b, size_t shm) {
  const std::string B(blk);
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64 || p.x_bpad < p.b_pad) die("%s: b %d b_pad %d x_bpad %d", blk, p.b, p.b_pad, p.x_bpad);
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N) die("%s: N %d D %d L %d l_pos %d", blk, p.N, p.D, p.L, p.l_pos);
  if (p.mb < 1 || p.mb > p.cap) die("%s: largest bond %d, capacity %d", blk, p.mb, p.cap);
  if (kernel) {
    if (b.x != 256 || g.x != (unsigned)((p.b + 63) / 64) || g.y != 1 || g.z != 1) die("%s: grid %u block %u for b %d", kernel, g.x, b.x, p.b);
    if (shm < grad_chain_lds_bytes(p.mb, p.D, p.L, p.N)) die("%s: %zu bytes of LDS, %zu wanted (bond %d, D %d, L %d)", kernel, shm, grad_chain_lds_bytes(p.mb, p.D, p.L, p.N), p.mb, p.D, p.L);
  }
  const size_t bp = p.b_pad;
  need(p.X, (size_t)p.N * p.x_bpad * p.D * 4, (B + ".X").c_str());
  need(p.cot, (size_t)p.L * bp * 4, (B + ".cot").c_str());
  opt(p.cf, (size_t)p.b * 4, (B + ".cf").c_str());
}
// every site's bonds through the table the host uploaded (the stand-in's device memory is host memory; the caller has checked its
// extent) and, for the two-pass chain, the extent of every core
static void check_grad_sites(const GradChainView &p, const char *blk, bool chain) {
  const std::string B(blk);
  for (int i = 0; i < p.N; ++i) {
    const int ml = i == 0 ? 1 : p.bond[i - 1], mr = i == p.N - 1 ? 1 : p.bond[i];
    if (ml < 1 || ml > p.mb || mr < 1 || mr > p.mb) die("%s: site %d is %d x %d, largest bond %d", blk, i, ml, mr, p.mb);
    if (!chain) continue;
    if (i == p.l_pos) need(p.labcore, (size_t)ml * p.D * mr * p.L * 4, (B + ".labcore").c_str());
    else need(p.cores + (size_t)i * p.core_stride, (size_t)ml * p.D * mr * 4, (B + ".cores").c_str());
  }
}

// input gradients (kernels_inputgrad.hip): every operand with the extent the kernel touches
static void check_input_grad(const InputGradParams &p, dim3 g, dim3 b, size_t shm) {
  scan(&p, sizeof p, "InputGradParams");
  const GradChainView v{p.bond, p.cores, p.labcore, p.X, p.cot, p.stack, p.cf, p.core_stride, p.b, p.b_pad, p.x_bpad, p.N, p.D, p.L, p.l_pos, p.cap, p.mb};
  check_grad_geometry(v, "InputGradParams", "input_grad_kernel", g, b, shm);
  need(p.bond, (size_t)(p.N - 1) * 4, "InputGradParams.bond");
  need(p.stack, (size_t)p.N * p.cap * p.b_pad * 4, "InputGradParams.stack");
  need(p.g, (size_t)p.b * p.N * p.D * 4, "InputGradParams.g");
  check_grad_sites(v, "InputGradParams", true);
}

// core gradients (kernels_coregrad.hip): one block for both kernels.  The chain kernel touches every core, X, cot, both stacks and cf;
// the reduction both stacks, X, cot and every core's extent of G through the offset half of the table.
static void check_core_grad(const CoreGradParams &p, dim3 g, dim3 b, size_t shm, bool reduce) {
  scan(&p, sizeof p, "CoreGradParams");
  const GradChainView v{p.tab, p.cores, p.labcore, p.X, p.cot, p.stackP, p.cf, p.core_stride, p.b, p.b_pad, p.x_bpad, p.N, p.D, p.L, p.l_pos, p.cap, p.mb};
  check_grad_geometry(v, "CoreGradParams", reduce ? nullptr : "core_grad_chain_kernel", g, b, shm);
  if (p.first != 0 && p.first != 1) die("CoreGradParams: first %d", p.first);
  const size_t bp = p.b_pad, tiles = (size_t)(p.b + 63) / 64 * 64;       // both kernels work on whole tiles of 64 samples
  if (tiles > bp) die("CoreGradParams: %zu samples in tiles, b_pad %zu", tiles, bp);
  if (reduce) {
    if (b.x != 256 || g.x != (unsigned)p.N || g.y != (unsigned)core_grad_reduce_blocks(p.mb, p.D) || g.z != (unsigned)p.L)
      die("core_grad_reduce_kernel: grid (%u, %u, %u) block %u for N %d bond %d D %d L %d", g.x, g.y, g.z, b.x, p.N, p.mb, p.D, p.L);
    if (shm < core_grad_reduce_lds_bytes(p.mb, p.D)) die("core_grad_reduce_kernel: %zu bytes of LDS, %zu wanted", shm, core_grad_reduce_lds_bytes(p.mb, p.D));
  }
  need(p.tab, (size_t)2 * p.N * 4, "CoreGradParams.tab");
  need(p.stackP, (size_t)p.N * p.cap * bp * 4, "CoreGradParams.stackP");
  need(p.stackQ, (size_t)p.N * p.cap * bp * 4, "CoreGradParams.stackQ");
  check_grad_sites(v, "CoreGradParams", !reduce);
  size_t off = 0;
  for (int i = 0; i < p.N; ++i) {
    const int ml = i == 0 ? 1 : p.tab[i - 1], mr = i == p.N - 1 ? 1 : p.tab[i];
    // the reduction covers a site's output with ceil(ml D / 16) x ceil(ceil(mr / 16) / 2) wave pairs, four to a workgroup
    if (reduce && (size_t)((ml * p.D + 15) / 16) * (((mr + 15) / 16 + 1) / 2) > (size_t)4 * g.y) die("core_grad_reduce_kernel: site %d (%d x %d) is not covered by %u workgroups", i, ml, mr, g.y);
    const size_t ne = (size_t)ml * p.D * mr * (i == p.l_pos ? p.L : 1);
    if ((size_t)p.tab[p.N + i] != off) die("CoreGradParams: core %d at offset %d, the flat layout has it at %zu", i, p.tab[p.N + i], off);
    if (reduce) need(p.G + off, ne * 4, "CoreGradParams.G");
    off += ne;
  }
}

// range-safe chains.  The two scaled gradient kernels: the plain block with the scaled form's LDS, and the
// exponent stack [N][b_pad] ints beside the stack of pass A.
static void check_scaled_lds(const char *kernel, size_t shm, int mb, int D, int L, int N) {
  const size_t want = grad_chain_lds_bytes(mb, D, L, N, true);
  if (shm < want) die("%s: %zu bytes of LDS, %zu wanted (bond %d, D %d, L %d)", kernel, shm, want, mb, D, L);
}
static void check_input_grad_scaled(const InputGradScaledParams &ps, dim3 g, dim3 b, size_t shm) {
  scan(&ps, sizeof ps, "InputGradScaledParams");
  check_input_grad(ps.base, g, b, shm);
  check_scaled_lds("input_grad_scaled_kernel", shm, ps.base.mb, ps.base.D, ps.base.L, ps.base.N);
  need(ps.estack, (size_t)ps.base.N * ps.base.b_pad * 4, "InputGradScaledParams.estack");
}
static void check_core_grad_scaled(const CoreGradScaledParams &ps, dim3 g, dim3 b, size_t shm) {
  scan(&ps, sizeof ps, "CoreGradScaledParams");
  check_core_grad(ps.base, g, b, shm, false);
  check_scaled_lds("core_grad_chain_scaled_kernel", shm, ps.base.mb, ps.base.D, ps.base.L, ps.base.N);
  need(ps.estack, (size_t)ps.base.N * ps.base.b_pad * 4, "CoreGradScaledParams.estack");
}
// scaled_pred_kernel (kernels_scaled.hip): whole tiles of 64 samples of X, mant, expo and f; every core through the bond table
static void check_scaled_pred(const ScaledPredParams &p, dim3 g, dim3 b, size_t shm) {
  scan(&p, sizeof p, "ScaledPredParams");
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64) die("ScaledPredParams: b %d b_pad %d", p.b, p.b_pad);
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N || p.mb < 1) die("ScaledPredParams: N %d D %d L %d l_pos %d mb %d", p.N, p.D, p.L, p.l_pos, p.mb);
  if (b.x != 256 || g.x != (unsigned)((p.b + 63) / 64) || g.y != 1 || g.z != 1) die("scaled_pred_kernel: grid %u block %u for b %d", g.x, b.x, p.b);
  check_scaled_lds("scaled_pred_kernel", shm, p.mb, p.D, p.L, p.N);
  const size_t bp = p.b_pad;
  need(p.bond, (size_t)(p.N - 1) * 4, "ScaledPredParams.bond");
  need(p.X, (size_t)p.N * bp * p.D * 4, "ScaledPredParams.X");
  need(p.mant, (size_t)p.L * bp * 4, "ScaledPredParams.mant");
  need(p.expo, bp * 4, "ScaledPredParams.expo");
  need(p.f, (size_t)p.L * bp * 4, "ScaledPredParams.f");
  for (int i = 0; i < p.N; ++i) {
    const int ml = i == 0 ? 1 : p.bond[i - 1], mr = i == p.N - 1 ? 1 : p.bond[i];
    if (ml < 1 || ml > p.mb || mr < 1 || mr > p.mb) die("ScaledPredParams: site %d is %d x %d, largest bond %d", i, ml, mr, p.mb);
    if (i == p.l_pos) need(p.labcore, (size_t)ml * p.D * mr * p.L * 4, "ScaledPredParams.labcore");
    else need(p.cores + (size_t)i * p.core_stride, (size_t)ml * p.D * mr * 4, "ScaledPredParams.cores");
  }
}

// orthogonal form / compression / bond spectra (kernels_orth.hip): one parameter block for the load, chain and store kernels.  The
// operation list is walked the way the chain kernel walks it: every decomposition hands its carried factor to the neighbouring site,
// which the next operation must name; the list ends with the centre on the label site.  Every slot of the context, of the float64
// work copy and of the float32 result, the absorbed site, the carried factors and the outputs with their extents.
static void check_orth(const OrthParams &p, dim3 g, dim3 b, size_t shm, int which) {       // which: 0 load, 1 chain, 2 store
  scan(&p, sizeof p, "OrthParams");
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N) die("OrthParams: N %d D %d L %d l_pos %d", p.N, p.D, p.L, p.l_pos);
  need(p.bond, (size_t)(p.N - 1) * 4, "OrthParams.bond");
  int mb = 1;
  for (int i = 0; i < p.N - 1; ++i) {
    if (p.bond[i] < 1) die("OrthParams: bond %d is %d", i, p.bond[i]);
    mb = p.bond[i] > mb ? p.bond[i] : mb;
  }
  if (which == 1) {
    if (g.x != 1 || g.y != 1 || g.z != 1 || b.x != 1024) die("orth_chain_kernel: grid %u block %u", g.x, b.x);
    if (shm < orth_chain_lds_bytes(mb)) die("orth_chain_kernel: %zu bytes of LDS for bond %d", shm, mb);
    if (p.npad < mb || p.npad % 2 || p.ld <= p.npad || shm < ((size_t)2 * p.npad * p.ld + 1024 + 4 * (size_t)p.npad) * 8 + 64)
      die("orth_chain_kernel: npad %d ld %d lds %zu for bond %d", p.npad, p.ld, shm, mb);
  } else if (g.x != (unsigned)p.N || g.y != 1 || g.z != 1 || b.x != 256) die("orth load / store kernel: grid %u block %u for N %d", g.x, b.x, p.N);
  if (!(p.threshold > 0.0 && p.threshold <= 1.0) || !(p.rank_tol >= 0.0 && p.rank_tol < 1.0) || p.m_max < 1) die("OrthParams: m_max %d threshold %g rank_tol %g", p.m_max, p.threshold, p.rank_tol);
  if (p.n_ops < 1) die("OrthParams: %d operations", p.n_ops);
  need(p.ops, (size_t)p.n_ops * sizeof(OrthOp), "OrthParams.ops");
  int pending = -1;
  for (int o = 0; o < p.n_ops; ++o) {
    const OrthOp &op = p.ops[o];
    if (op.site < 0 || op.site >= p.N || op.kind < kOrthRight || op.kind > kOrthCentre || op.cut < 0 || op.cut > 2) die("OrthOp %d: site %d kind %d cut %d", o, op.site, op.kind, op.cut);
    if (pending >= 0 && op.site != pending) die("OrthOp %d names site %d, the carried factor belongs to site %d", o, op.site, pending);
    pending = -1;
    if (op.kind == kOrthRight) { if (op.site == p.N - 1) die("OrthOp %d: the last site has no right bond", o); pending = op.site + 1; }
    if (op.kind == kOrthLeft) { if (op.site == 0) die("OrthOp %d: the first site has no left bond", o); pending = op.site - 1; }
    if (op.kind == kOrthCentre && (op.site != p.l_pos || o != p.n_ops - 1)) die("OrthOp %d: centre on site %d (label on %d, %d operations)", o, op.site, p.l_pos, p.n_ops);
  }
  if (p.ops[p.n_ops - 1].kind != kOrthCentre) die("OrthParams: the list does not end with the centre");
  if (p.aux_stride < (size_t)mb * mb) die("OrthParams: carried factors of %zu doubles for bond %d", p.aux_stride, mb);
  need(p.aux, 4 * p.aux_stride * 8, "OrthParams.aux");
  need(p.Mbuf, p.lab_elems * 8, "OrthParams.Mbuf");
  need(p.W, ((size_t)p.N * p.core_stride + p.lab_elems) * 8, "OrthParams.W");
  need(p.out_cores, (size_t)p.N * p.core_stride * 4, "OrthParams.out_cores");
  need(p.out_lab, p.lab_elems * 4, "OrthParams.out_lab");
  for (int i = 0; i < p.N; ++i) {
    const int ml = i == 0 ? 1 : p.bond[i - 1], mr = i == p.N - 1 ? 1 : p.bond[i];
    const size_t ne = (size_t)ml * p.D * mr * (i == p.l_pos ? p.L : 1);
    if (ne > (i == p.l_pos ? p.lab_elems : p.core_stride)) die("OrthParams: core %d of %zu floats beyond its slot", i, ne);
    if (i == p.l_pos) need(p.labcore, ne * 4, "OrthParams.labcore");
    else need(p.cores + (size_t)i * p.core_stride, ne * 4, "OrthParams.cores");
  }
  if (p.sigma_ld < mb) die("OrthParams: spectra rows of %d for bond %d", p.sigma_ld, mb);
  need(p.sigma_out, (size_t)(p.N - 1) * p.sigma_ld * 8, "OrthParams.sigma_out");
  need(p.discarded_out, (size_t)(p.N - 1) * 8, "OrthParams.discarded_out");
  need(p.rank_out, (size_t)(p.N - 1) * 4, "OrthParams.rank_out");
  need(p.result, 2 * 8, "OrthParams.result");
  need(p.status, 4, "OrthParams.status");
}

// inner products and linear combinations (kernels_algebra.hip): one parameter block for the chain, meet and place kernels.  Both bond
// tables and both offset tables are read here as the kernels read them; every core of either chain, the staging areas and half
// results of the workgroups of the launch, the outputs and (place kernel) the float32 result with the summed cores inside their slots.
static void check_algebra(const AlgebraParams &p, dim3 g, dim3 b, size_t shm, int which) {  // which: 0 chain, 1 meet, 2 place
  scan(&p, sizeof p, "AlgebraParams");
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N) die("AlgebraParams: N %d D %d L %d l_pos %d", p.N, p.D, p.L, p.l_pos);
  if (p.n_prod != 1 && p.n_prod != 3) die("AlgebraParams: %d products", p.n_prod);
  const int chains = (which == 2 || p.n_prod == 3) ? 2 : 1;
  if (which == 2 && p.n_prod != 3) die("sum_place_kernel without a second chain");
  need(p.bond, (size_t)chains * (p.N - 1) * 4, "AlgebraParams.bond");
  need(p.off, (size_t)(chains - 1) * p.N * 8 + (size_t)p.N * 8, "AlgebraParams.off");
  int mb = 1;
  for (int ch = 0; ch < chains; ++ch) {
    const int *bond = p.bond + (size_t)ch * (p.N - 1);
    const long long *off = p.off + (size_t)ch * p.N;
    const float *plain = ch ? p.v_plain : p.w_plain, *lab = ch ? p.v_lab : p.w_lab;
    for (int i = 0; i < p.N; ++i) {
      const int ml = i == 0 ? 1 : bond[i - 1], mr = i == p.N - 1 ? 1 : bond[i];
      if (ml < 1 || mr < 1) die("AlgebraParams: chain %d site %d is %d x %d", ch, i, ml, mr);
      mb = mb > mr ? mb : mr;
      const size_t ne = (size_t)ml * p.D * mr * (i == p.l_pos ? p.L : 1);
      if (i == p.l_pos) need(lab, ne * 4, ch ? "AlgebraParams.v_lab" : "AlgebraParams.w_lab");
      else {
        if (off[i] < 0) die("AlgebraParams: chain %d core %d at offset %lld", ch, i, off[i]);
        need(plain + off[i], ne * 4, ch ? "AlgebraParams.v_plain" : "AlgebraParams.w_plain");
      }
    }
  }
  need(p.status, 4, "AlgebraParams.status");
  if (which == 2) {
    if (g.x != (unsigned)p.N || g.y != 1 || g.z != 1 || b.x != 256) die("sum_place_kernel: grid %u block %u for N %d", g.x, b.x, p.N);
    if (!(p.alpha == p.alpha && p.beta == p.beta)) die("AlgebraParams: alpha %g beta %g", p.alpha, p.beta);
    need(p.out_cores, (size_t)p.N * p.core_stride * 4, "AlgebraParams.out_cores");
    need(p.out_lab, p.lab_elems * 4, "AlgebraParams.out_lab");
    for (int i = 0; i < p.N; ++i) {
      const int ml = i == 0 ? 1 : p.bond[i - 1] + p.bond[p.N - 1 + i - 1], mr = i == p.N - 1 ? 1 : p.bond[i] + p.bond[p.N - 1 + i];
      const size_t ne = (size_t)ml * p.D * mr * (i == p.l_pos ? p.L : 1);
      if (ne > (i == p.l_pos ? p.lab_elems : p.core_stride)) die("AlgebraParams: summed core %d of %zu floats beyond its slot", i, ne);
    }
    return;
  }
  const size_t m2 = (size_t)mb * mb;
  if ((size_t)p.lds_m2 < m2 || p.half_stride < m2 || p.stage_stride < m2 * p.D) die("AlgebraParams: lds_m2 %d half_stride %zu stage_stride %zu for bond %d", p.lds_m2, p.half_stride, p.stage_stride, mb);
  if (b.x != 1024 || g.x != (unsigned)p.n_prod || g.y != (which == 0 ? 2u : 1u) || g.z != 1) die("inner kernel %d: grid (%u, %u) block %u for %d products", which, g.x, g.y, b.x, p.n_prod);
  if (which == 0 && (shm < ((size_t)2 * p.lds_m2 + 32) * 8 || (size_t)p.lds_m2 > 10 * 1024)) die("inner_chain_kernel: %zu bytes of LDS for bond %d", shm, mb);
  if (which == 1 && shm < ((size_t)p.lds_m2 + 1024) * 8) die("inner_meet_kernel: %zu bytes of LDS for bond %d", shm, mb);
  if (p.metric_sites != 0 && p.metric_sites != 1 && p.metric_sites != p.N) die("AlgebraParams: metric_sites %d", p.metric_sites);
  if (p.metric_sites) need(p.metric, (size_t)p.metric_sites * p.D * p.D * 8, "AlgebraParams.metric");
  need(p.stage, (size_t)p.n_prod * 2 * 2 * p.stage_stride * 8, "AlgebraParams.stage");
  need(p.half_E, (size_t)p.n_prod * 2 * p.half_stride * 8, "AlgebraParams.half_E");
  need(p.half_expo, (size_t)p.n_prod * 2 * 4, "AlgebraParams.half_expo");
  need(p.out, (size_t)p.n_prod * 2 * 8, "AlgebraParams.out");
}

// samples and log-likelihoods (kernels_sample.hip): one parameter block for the two environment launches and the walk.  The bond,
// slot and tile tables, the classes and the given levels are read here as the kernels read them: every core, every environment a
// workgroup of the launch stores or reads, the staging areas, the grid, the uniforms and the outputs with their extents; every
// sample in exactly one tile, and that tile of its class.
static void check_sample(const SampleParams &p, dim3 g, dim3 b, size_t shm, bool walk) {
  scan(&p, sizeof p, "SampleParams");
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N) die("SampleParams: N %d D %d L %d l_pos %d", p.N, p.D, p.L, p.l_pos);
  if (p.K < 2 || p.K > kSmpMaxK || p.n < 1 || p.n_given < 0 || p.n_given > p.N) die("SampleParams: K %d n %d n_given %d", p.K, p.n, p.n_given);
  if (p.n_slots < 1 || p.n_slots > p.L + 1 || p.n_tiles < 1) die("SampleParams: %d slots %d tiles", p.n_slots, p.n_tiles);
  need(p.bond, (size_t)(p.N - 1) * 4, "SampleParams.bond");
  int mb = 1;
  for (int i = 0; i < p.N; ++i) {
    const int ml = i == 0 ? 1 : p.bond[i - 1], mr = i == p.N - 1 ? 1 : p.bond[i];
    if (ml < 1 || mr < 1) die("SampleParams: site %d is %d x %d", i, ml, mr);
    mb = mb > mr ? mb : mr;
    const size_t ne = (size_t)ml * p.D * mr * (i == p.l_pos ? p.L : 1);
    if (i == p.l_pos) need(p.lab, ne * 4, "SampleParams.lab");
    else need(p.cores + (size_t)i * p.core_stride, ne * 4, "SampleParams.cores");
  }
  const size_t m2 = (size_t)mb * mb;
  if (p.lds_m != mb || mb > kSmpMaxBond || p.env_stride < m2 || p.stage_stride < m2 * p.D) die("SampleParams: lds_m %d env_stride %zu stage_stride %zu for bond %d", p.lds_m, p.env_stride, p.stage_stride, mb);
  need(p.S, (size_t)p.D * p.D * 8, "SampleParams.S");
  need(p.slot_class, (size_t)p.n_slots * 4, "SampleParams.slot_class");
  for (int j = 0; j < p.n_slots; ++j)
    if (p.slot_class[j] < -1 || p.slot_class[j] >= p.L || (j && p.slot_class[j] <= p.slot_class[j - 1])) die("SampleParams: slot %d is class %d", j, p.slot_class[j]);
  need(p.env_shared, (size_t)(p.N + 1) * p.env_stride * 8, "SampleParams.env_shared");
  if (p.l_pos >= 1) need(p.env_slots, (size_t)p.n_slots * (p.l_pos + 1) * p.env_stride * 8, "SampleParams.env_slots");
  need(p.status, 2 * 4, "SampleParams.status");
  if (p.status[0] != 0 || p.status[1] != INT_MAX) die("SampleParams: status words %d %d at launch", p.status[0], p.status[1]);
  if (!walk) {
    if (p.phase != 1 && p.phase != 2) die("sample_env_kernel: phase %d", p.phase);
    if (p.phase == 2 && p.l_pos < 1) die("sample_env_kernel: phase 2 with the label on site 0");
    const unsigned want = p.phase == 1 ? 1u : (unsigned)p.n_slots;
    if (g.x != want || g.y != 1 || g.z != 1 || b.x != 1024) die("sample_env_kernel phase %d: grid %u block %u for %d slots", p.phase, g.x, b.x, p.n_slots);
    if (shm < sample_env_lds_bytes(mb, p.D) || m2 > 4 * 1024) die("sample_env_kernel: %zu bytes of LDS for bond %d", shm, mb);
    need(p.stage, (size_t)want * p.stage_stride * 8, "SampleParams.stage");
    return;
  }
  if (p.phase != 0) die("sample_walk_kernel: phase %d", p.phase);
  if (g.x != (unsigned)p.n_tiles || g.y != 1 || g.z != 1 || b.x != 512) die("sample_walk_kernel: grid %u block %u for %d tiles", g.x, b.x, p.n_tiles);
  if (shm < sample_walk_lds_bytes(mb, p.D, p.L, p.K)) die("sample_walk_kernel: %zu bytes of LDS for bond %d", shm, mb);
  need(p.phi, (size_t)p.K * p.D * 8, "SampleParams.phi");
  need(p.w, (size_t)p.K * 8, "SampleParams.w");
  need(p.tile_slot, (size_t)p.n_tiles * 4, "SampleParams.tile_slot");
  need(p.tile_samples, (size_t)p.n_tiles * kSmpTile * 4, "SampleParams.tile_samples");
  need(p.classes, (size_t)p.n * 4, "SampleParams.classes");
  if (p.n_given) need(p.given, (size_t)p.n * p.n_given * 4, "SampleParams.given");
  if (p.u) need(p.u, (size_t)p.n * (p.N + 1) * 8, "SampleParams.u");
  need(p.levels, (size_t)p.n * p.N * 4, "SampleParams.levels");
  need(p.labels, (size_t)p.n * 4, "SampleParams.labels");
  need(p.logp, (size_t)p.n * 2 * 8, "SampleParams.logp");
  std::vector<char> seen((size_t)p.n, 0);
  for (int t = 0; t < p.n_tiles; ++t) {
    const int slot = p.tile_slot[t];
    if (slot < 0 || slot >= p.n_slots) die("SampleParams: tile %d of slot %d", t, slot);
    for (int k = 0; k < kSmpTile; ++k) {
      const int smp = p.tile_samples[t * kSmpTile + k];
      if (smp == -1) continue;
      if (smp < 0 || smp >= p.n || seen[smp]) die("SampleParams: tile %d holds sample %d", t, smp);
      seen[smp] = 1;
      if (p.classes[smp] != p.slot_class[slot]) die("SampleParams: sample %d of class %d in a tile of class %d", smp, p.classes[smp], p.slot_class[slot]);
      for (int i = 0; i < p.n_given; ++i)
        if (p.given[(size_t)smp * p.n_given + i] < 0 || p.given[(size_t)smp * p.n_given + i] >= p.K) die("SampleParams: given level of sample %d site %d", smp, i);
    }
  }
  for (int smp = 0; smp < p.n; ++smp)
    if (!seen[smp]) die("SampleParams: sample %d is in no tile", smp);
}

// the gradient of the log-norm (kernels_nll.hip): one parameter block for the environment kernel and the gradient kernel.  The table
// is read here as the kernels read it: every core, both environment stacks and both exponent arrays over N + 1 slots, and every
// core's part of G at its offset in the flat layout.
// the block's own extents -> the largest bond (grad: every core's part of G as well)
static int lognorm_extents(const LogNormParams &p, bool grad) {
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N) die("LogNormParams: N %d D %d L %d l_pos %d", p.N, p.D, p.L, p.l_pos);
  if (p.metric_sites != 0 && p.metric_sites != 1 && p.metric_sites != p.N) die("LogNormParams: metric_sites %d", p.metric_sites);
  if (p.mode != 0 && p.mode != 1) die("LogNormParams: mode %d", p.mode);
  need(p.tab, (size_t)2 * p.N * 4, "LogNormParams.tab");
  int mb = 1;
  size_t off = 0;
  for (int i = 0; i < p.N; ++i) {
    const int ml = i == 0 ? 1 : p.tab[i - 1], mr = i == p.N - 1 ? 1 : p.tab[i];
    if (ml < 1 || mr < 1) die("LogNormParams: site %d is %d x %d", i, ml, mr);
    mb = mb > mr ? mb : mr;
    const size_t ne = (size_t)ml * p.D * mr * (i == p.l_pos ? p.L : 1);
    if ((size_t)p.tab[p.N + i] != off) die("LogNormParams: core %d at offset %d, the flat layout has it at %zu", i, p.tab[p.N + i], off);
    if (i == p.l_pos) need(p.lab, ne * 4, "LogNormParams.lab");
    else {
      if (ne > p.core_stride) die("LogNormParams: core %d of %zu floats in a slot of %zu", i, ne, p.core_stride);
      need(p.cores + (size_t)i * p.core_stride, ne * 4, "LogNormParams.cores");
    }
    if (grad) need(p.G + off, ne * 4, "LogNormParams.G");
    off += ne;
  }
  const size_t m2 = (size_t)mb * mb;
  if (p.lds_m != mb || mb > kLnzMaxBond || p.env_stride < m2) die("LogNormParams: lds_m %d env_stride %zu for bond %d", p.lds_m, p.env_stride, mb);
  if (p.metric_sites) need(p.metric, (size_t)p.metric_sites * p.D * p.D * 8, "LogNormParams.metric");
  need(p.envL, (size_t)(p.N + 1) * p.env_stride * 8, "LogNormParams.envL");
  need(p.envR, (size_t)(p.N + 1) * p.env_stride * 8, "LogNormParams.envR");
  need(p.expL, (size_t)(p.N + 1) * 4, "LogNormParams.expL");
  need(p.expR, (size_t)(p.N + 1) * 4, "LogNormParams.expR");
  need(p.out, 2 * 8, "LogNormParams.out");
  need(p.status, 2 * 4, "LogNormParams.status");
  if (p.class_plus1 < 0 || p.class_plus1 > p.L || (grad && p.class_plus1 != 0)) die("LogNormParams: class slot %d of %d labels", p.class_plus1 - 1, p.L);
  return mb;
}

static void check_lognorm(const LogNormParams &p, dim3 g, dim3 b, size_t shm, bool grad) {
  scan(&p, sizeof p, "LogNormParams");
  const int mb = lognorm_extents(p, grad);
  if (!grad) {
    if (p.status[0] != 0 || p.status[1] != 0) die("LogNormParams: status words %d %d at launch", p.status[0], p.status[1]);
    if (g.x != 2 || g.y != 1 || g.z != 1 || b.x != 1024) die("lognorm_env_kernel: grid %u block %u", g.x, b.x);
    if (shm < lognorm_env_lds_bytes(mb, p.D)) die("lognorm_env_kernel: %zu bytes of LDS for bond %d", shm, mb);
  } else {
    if (g.x != (unsigned)p.N || g.y != (unsigned)p.L || g.z != 1 || b.x != 512) die("lognorm_grad_kernel: grid (%u, %u) block %u for N %d L %d", g.x, g.y, b.x, p.N, p.L);
    if (shm < lognorm_grad_lds_bytes(mb, p.D)) die("lognorm_grad_kernel: %zu bytes of LDS for bond %d", shm, mb);
  }
}

// pixel-pair marginals (kernels_pair.hip): the three launches behind the environment launch of the call.  Their block e is that
// launch's with the grid's metric; the grid, the values, B_j of every site and the per-site outputs; for the row launches the chunk's
// sites (distinct, ascending, inside the chain) and Q, its exponents and the statistics over the chunk's rows; grid, block and LDS.
static void check_pair(const PairParams &p, dim3 g, dim3 b, size_t shm, int which) {      // 0 close, 1 walk, 2 statistics
  scan(&p, sizeof p, "PairParams");
  const LogNormParams &e = p.e;
  const int mb = lognorm_extents(e, false);
  if (e.metric_sites != 1 || mb > kPairMaxBond) die("PairParams: metric_sites %d bond %d", e.metric_sites, mb);
  if (p.K < 2 || p.K > kSmpMaxK) die("PairParams: K %d", p.K);
  const size_t N = (size_t)e.N, DD = (size_t)e.D * e.D;
  need(p.phi, (size_t)p.K * e.D * 8, "PairParams.phi");
  need(p.w, (size_t)p.K * 8, "PairParams.w");
  need(p.values, (size_t)p.K * 8, "PairParams.values");
  need(p.B, N * DD * e.env_stride * 8, "PairParams.B");
  need(p.q1, N * DD * 8, "PairParams.q1");
  need(p.stats1, N * 3 * 8, "PairParams.stats1");
  if (which == 0) {
    if (g.x != (unsigned)e.N || g.y != 1 || g.z != 1 || b.x != (unsigned)kPairCloseThreads) die("pair_close_kernel: grid %u block %u for N %d", g.x, b.x, e.N);
    if (shm < pair_close_lds_bytes(mb, e.D, p.K)) die("pair_close_kernel: %zu bytes of LDS for bond %d", shm, mb);
    return;
  }
  if (p.n_rows < 1 || p.n_rows > e.N) die("PairParams: %d rows", p.n_rows);
  const size_t R = (size_t)p.n_rows;
  need(p.rows, R * 4, "PairParams.rows");
  for (int r = 0; r < p.n_rows; ++r)
    if (p.rows[r] < 0 || p.rows[r] >= e.N || (r > 0 && p.rows[r] <= p.rows[r - 1])) die("PairParams: rows[%d] = %d (N %d, ascending)", r, p.rows[r], e.N);
  need(p.Q, R * N * DD * DD * 8, "PairParams.Q");
  need(p.qexp, R * N * DD * 4, "PairParams.qexp");
  need(p.stats, R * N * 3 * 8, "PairParams.stats");
  if (which == 1) {
    if (g.x != (unsigned)p.n_rows || g.y != (unsigned)DD || g.z != 1 || b.x != (unsigned)pair_walk_threads(mb))
      die("pair_walk_kernel: grid (%u, %u) block %u for %d rows at D %d, bond %d", g.x, g.y, b.x, p.n_rows, e.D, mb);
    if (shm < pair_walk_lds_bytes(mb, e.D)) die("pair_walk_kernel: %zu bytes of LDS for bond %d", shm, mb);
  } else {
    if (g.x != (unsigned)e.N || g.y != (unsigned)p.n_rows || g.z != 1 || b.x != (unsigned)kPairStatThreads)
      die("pair_stats_kernel: grid (%u, %u) block %u for N %d, %d rows", g.x, g.y, b.x, e.N, p.n_rows);
    if (shm < pair_stats_lds_bytes(e.D, p.K)) die("pair_stats_kernel: %zu bytes of LDS for D %d K %d", shm, e.D, p.K);
  }
}

// the cotangent of the likelihood's data term (kernels_nll.hip): f and the labels over the chunk, cot over its padded columns, the
// per-sample terms and flags at the chunk's offset within the batch
static void check_nll_cot(const NllCotParams &p, dim3 g, dim3 b) {
  scan(&p, sizeof p, "NllCotParams");
  if (p.L < 1 || p.b < 1 || p.b > p.b_pad || p.b_pad % 64 || p.f_bpad < p.b_pad || p.off < 0 || p.batch < p.off + p.b)
    die("NllCotParams: L %d b %d b_pad %d f_bpad %d off %d batch %d", p.L, p.b, p.b_pad, p.f_bpad, p.off, p.batch);
  if ((size_t)g.x * b.x < (size_t)p.b_pad || g.y != 1 || b.x != 256) die("nll_cot_kernel: grid %u x %u for b_pad %d", g.x, b.x, p.b_pad);
  need(p.f, ((size_t)(p.L - 1) * p.f_bpad + p.b) * 4, "NllCotParams.f");
  if (p.y) {
    need(p.y, (size_t)p.b * 4, "NllCotParams.y");
    for (int s = 0; s < p.b; ++s)
      if (p.y[s] < 0 || p.y[s] >= p.L) die("NllCotParams: label %d of sample %d outside [0, %d)", p.y[s], s, p.L);
  }
  if (p.cot) need(p.cot, (size_t)p.L * p.b_pad * 4, "NllCotParams.cot");
  need(p.terms + p.off, (size_t)p.b * 8, "NllCotParams.terms");
  need(p.bad + p.off, (size_t)p.b * 4, "NllCotParams.bad");
}

// the same given any set of known pixels (kernels_sample_masked.hip): one parameter block for the environment launch and the walk of
// one chunk of tiles.  The bond, tile and row tables, the mask and the known levels are read here as the kernels read them: every
// core, the stack slots and E of every row of the launch, the grid, the uniforms and the outputs with their extents; T the one the
// host derives for both kernels; no sample twice in a launch.  The (sample, class) pairs of the launches since the last
// san_stub_masked_reset are kept for san_stub_masked_check: every sample of a call in exactly one tile, and that tile of its class.
static std::vector<std::pair<int, int>> g_masked_rows[2];        // [0] environment launches, [1] walk launches
// san_stub_site_cond_call(1): the environment launches that follow are those of tnml_site_conditionals, whose tile is site_cond_tile's;
// the block of the last environment launch, for the site_cond_kernel launch behind it
static int g_site_cond_call = 0;
static SampleMaskedParams g_last_env{};
static void check_sample_masked(const SampleMaskedParams &p, dim3 g, dim3 b, size_t shm, bool walk) {
  scan(&p, sizeof p, "SampleMaskedParams");
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N) die("SampleMaskedParams: N %d D %d L %d l_pos %d", p.N, p.D, p.L, p.l_pos);
  if (p.K < 2 || p.K > kSmpMaxK || p.n < 1 || p.n_tiles < 1 || (p.mask_rows != 1 && p.mask_rows != p.n)) die("SampleMaskedParams: K %d n %d tiles %d mask_rows %d", p.K, p.n, p.n_tiles, p.mask_rows);
  need(p.bond, (size_t)(p.N - 1) * 4, "SampleMaskedParams.bond");
  int mb = 1;
  for (int i = 0; i < p.N; ++i) {
    const int ml = i == 0 ? 1 : p.bond[i - 1], mr = i == p.N - 1 ? 1 : p.bond[i];
    if (ml < 1 || mr < 1) die("SampleMaskedParams: site %d is %d x %d", i, ml, mr);
    mb = mb > mr ? mb : mr;
    const size_t ne = (size_t)ml * p.D * mr * (i == p.l_pos ? p.L : 1);
    if (i == p.l_pos) need(p.lab, ne * 4, "SampleMaskedParams.lab");
    else need(p.cores + (size_t)i * p.core_stride, ne * 4, "SampleMaskedParams.cores");
  }
  const size_t m2 = (size_t)mb * mb, rows = (size_t)p.n_tiles * p.T;
  if (p.lds_m != mb || mb > kSmpMaxBond || p.env_stride < m2) die("SampleMaskedParams: lds_m %d env_stride %zu for bond %d", p.lds_m, p.env_stride, mb);
  const int want_T = g_site_cond_call == 2 ? masked_grad_tile(mb, p.D, p.L, p.K) : g_site_cond_call ? site_cond_tile(mb, p.D, p.L, p.K) : sample_masked_tile(mb, p.D, p.L, p.K);
  if (p.T < 1 || p.T != want_T) die("SampleMaskedParams: tiles of %d rows, %d fit at bond %d", p.T, want_T, mb);
  if (!walk) g_last_env = p;
  need(p.S, (size_t)p.D * p.D * 8, "SampleMaskedParams.S");
  need(p.phi, (size_t)p.K * p.D * 8, "SampleMaskedParams.phi");
  need(p.w, (size_t)p.K * 8, "SampleMaskedParams.w");
  need(p.tile_class, (size_t)p.n_tiles * 4, "SampleMaskedParams.tile_class");
  need(p.tile_rows, rows * 4, "SampleMaskedParams.tile_rows");
  need(p.mask, (size_t)p.mask_rows * p.N, "SampleMaskedParams.mask");
  need(p.known, (size_t)p.n * p.N * 4, "SampleMaskedParams.known");
  need(p.stack, rows * (p.N + 1) * p.env_stride * 8, "SampleMaskedParams.stack");
  need(p.E, rows * 8, "SampleMaskedParams.E");
  need(p.status, 2 * 4, "SampleMaskedParams.status");
  if (p.status[0] != 0 || p.status[1] != INT_MAX) die("SampleMaskedParams: status words %d %d at launch", p.status[0], p.status[1]);
  const char *kn = walk ? "sample_walk_masked_kernel" : "sample_env_masked_kernel";
  if (g.x != (unsigned)p.n_tiles || g.y != 1 || g.z != 1 || b.x != 512) die("%s: grid %u block %u for %d tiles", kn, g.x, b.x, p.n_tiles);
  if (shm < (walk ? sample_masked_walk_lds_bytes(mb, p.D, p.L, p.K, p.T) : sample_masked_env_lds_bytes(mb, p.D, p.T))) die("%s: %zu bytes of LDS for bond %d, T %d", kn, shm, mb, p.T);
  if (walk) {
    if (p.u) need(p.u, (size_t)p.n * (p.N + 1) * 8, "SampleMaskedParams.u");
    need(p.levels, (size_t)p.n * p.N * 4, "SampleMaskedParams.levels");
    need(p.labels, (size_t)p.n * 4, "SampleMaskedParams.labels");
    need(p.logp0, (size_t)p.n * 8, "SampleMaskedParams.logp0");
  }
  std::vector<char> seen((size_t)p.n, 0);
  for (int t = 0; t < p.n_tiles; ++t) {
    const int cls = p.tile_class[t];
    if (cls < -1 || cls >= p.L) die("SampleMaskedParams: tile %d of class %d", t, cls);
    for (int k = 0; k < p.T; ++k) {
      const int smp = p.tile_rows[(size_t)t * p.T + k];
      if (smp == -1) continue;
      if (smp < 0 || smp >= p.n || seen[smp]) die("SampleMaskedParams: tile %d holds sample %d", t, smp);
      seen[smp] = 1;
      g_masked_rows[walk].emplace_back(smp, cls);
      const unsigned char *ms = p.mask + (size_t)(p.mask_rows == 1 ? 0 : smp) * p.N;
      for (int i = 0; i < p.N; ++i)
        if (ms[i] && (p.known[(size_t)smp * p.N + i] < 0 || p.known[(size_t)smp * p.N + i] >= p.K)) die("SampleMaskedParams: known level of sample %d site %d", smp, i);
    }
  }
}

// per-pixel conditionals (kernels_site_cond.hip): site_cond_kernel behind the environment launch of the same chunk.  Its block m
// is that launch's, field for field (the same tile, tables, rows and stack; lds_m filled in); the values, the left environments of
// the launch's rows and the outputs the call asked for with their extents; grid, block and LDS.
static void check_site_cond(const SiteCondParams &p, dim3 g, dim3 b, size_t shm) {
  scan(&p, sizeof p, "SiteCondParams");
  if (g_site_cond_call != 1) die("site_cond_kernel outside a tnml_site_conditionals call");
  const SampleMaskedParams &m = p.m, &e = g_last_env;
  if (m.T != e.T || m.n_tiles != e.n_tiles || m.lds_m != e.lds_m || m.n != e.n || m.tile_class != e.tile_class || m.tile_rows != e.tile_rows ||
      m.stack != e.stack || m.env_stride != e.env_stride || m.mask != e.mask || m.known != e.known || m.mask_rows != e.mask_rows || m.bond != e.bond ||
      m.cores != e.cores || m.lab != e.lab || m.S != e.S || m.phi != e.phi || m.w != e.w || m.status != e.status)
    die("site_cond_kernel: its block is not the one of the environment launch before it (T %d against %d)", m.T, e.T);
  const size_t rows = (size_t)m.n_tiles * m.T, sites = (size_t)m.n * m.N;
  if (m.T != site_cond_tile(m.lds_m, m.D, m.L, m.K) || m.lds_m > kSccMaxBond) die("site_cond_kernel: tiles of %d rows at bond %d", m.T, m.lds_m);
  need(p.values, (size_t)m.K * 8, "SiteCondParams.values");
  need(p.lf_next, rows * m.env_stride * 8, "SiteCondParams.lf_next");
  if (!p.q && !p.stats && !p.mode) die("site_cond_kernel: no output");
  if (p.q) need(p.q, sites * m.D * m.D * 8, "SiteCondParams.q");
  if (p.stats) need(p.stats, sites * 4 * 8, "SiteCondParams.stats");
  if (p.mode) need(p.mode, sites * 4, "SiteCondParams.mode");
  if (g.x != (unsigned)m.n_tiles || g.y != 1 || g.z != 1 || b.x != 512) die("site_cond_kernel: grid %u block %u for %d tiles", g.x, b.x, m.n_tiles);
  if (shm < site_cond_lds_bytes(m.lds_m, m.D, m.K, m.T)) die("site_cond_kernel: %zu bytes of LDS for bond %d, T %d", shm, m.lds_m, m.T);
}

// likelihood gradients from incomplete data (kernels_nll_masked.hip): masked_grad_kernel behind the environment launch of the same
// chunk.  Its block m is that launch's, field for field; the offsets, the row weights, the left environments and the partial
// gradients of the launch with their extents; grid, block and LDS.  A row with a sample carries 2 / n, a row without one 0 (padding) or
// -2 (the normaliser: the first row of a tile of class -1); the normaliser rows since the last san_stub_masked_reset are counted.
static long g_nmg_normalisers = 0;
static void check_masked_grad(const MaskedGradParams &p, dim3 g, dim3 b, size_t shm) {
  scan(&p, sizeof p, "MaskedGradParams");
  if (g_site_cond_call != 2) die("masked_grad_kernel outside a tnml_nll_masked call");
  const SampleMaskedParams &m = p.m, &e = g_last_env;
  if (m.T != e.T || m.n_tiles != e.n_tiles || m.lds_m != e.lds_m || m.n != e.n || m.tile_class != e.tile_class || m.tile_rows != e.tile_rows ||
      m.stack != e.stack || m.env_stride != e.env_stride || m.mask != e.mask || m.known != e.known || m.mask_rows != e.mask_rows || m.bond != e.bond ||
      m.cores != e.cores || m.lab != e.lab || m.S != e.S || m.phi != e.phi || m.w != e.w || m.status != e.status)
    die("masked_grad_kernel: its block is not the one of the environment launch before it (T %d against %d)", m.T, e.T);
  const size_t rows = (size_t)m.n_tiles * m.T;
  if (m.T != masked_grad_tile(m.lds_m, m.D, m.L, m.K) || m.lds_m > kNmgMaxBond) die("masked_grad_kernel: tiles of %d rows at bond %d", m.T, m.lds_m);
  need(p.off, (size_t)m.N * 4, "MaskedGradParams.off");
  size_t total = 0;
  for (int i = 0; i < m.N; ++i) {
    const int ml = i == 0 ? 1 : m.bond[i - 1], mr = i == m.N - 1 ? 1 : m.bond[i];
    if ((size_t)p.off[i] != total) die("masked_grad_kernel: core %d at offset %d, expected %zu", i, p.off[i], total);
    total += (size_t)ml * m.D * mr * (i == m.l_pos ? m.L : 1);
  }
  if (p.total != total) die("masked_grad_kernel: total %zu for cores of %zu floats", p.total, total);
  need(p.wrow, rows * 8, "MaskedGradParams.wrow");
  need(p.lf_next, rows * m.env_stride * 8, "MaskedGradParams.lf_next");
  need(p.part, (size_t)m.n_tiles * total * 8, "MaskedGradParams.part");
  need(p.status, 2 * 4, "MaskedGradParams.status");
  for (size_t r = 0; r < rows; ++r) {
    const int smp = m.tile_rows[r];
    const double w = p.wrow[r];
    if (smp >= 0 ? w != 2.0 / m.n : (w != 0.0 && !(w == -2.0 && r % m.T == 0 && m.tile_class[r / m.T] == -1)))
      die("masked_grad_kernel: row %zu (sample %d) carries weight %g", r, smp, w);
    if (w == -2.0) ++g_nmg_normalisers;
  }
  if (g.x != (unsigned)m.n_tiles || g.y != 1 || g.z != 1 || b.x != 512) die("masked_grad_kernel: grid %u block %u for %d tiles", g.x, b.x, m.n_tiles);
  if (shm < masked_grad_lds_bytes(m.lds_m, m.D, m.K, m.T)) die("masked_grad_kernel: %zu bytes of LDS for bond %d, T %d", shm, m.lds_m, m.T);
}
static void check_masked_grad_reduce(const MaskedGradReduceParams &p, dim3 g, dim3 b) {
  scan(&p, sizeof p, "MaskedGradReduceParams");
  if (p.n_tiles < 1 || p.total < 1 || (p.first != 0 && p.first != 1) || (p.last != 0 && p.last != 1)) die("MaskedGradReduceParams: tiles %d total %zu", p.n_tiles, p.total);
  need(p.part, (size_t)p.n_tiles * p.total * 8, "MaskedGradReduceParams.part");
  need(p.acc, p.total * 8, "MaskedGradReduceParams.acc");
  need(p.G, p.total * 4, "MaskedGradReduceParams.G");
  need(p.status, 2 * 4, "MaskedGradReduceParams.status");
  if (g.y != 1 || g.z != 1 || (size_t)g.x * b.x < p.total) die("masked_grad_reduce_kernel: grid %u x %u for %zu elements", g.x, b.x, p.total);
}

// gradient training (kernels_optim.hip).  loss_cot_kernel: f and cot at their own strides, the labels of the chunk, one thread per
// column of cot.  optim_step_kernel: one workgroup per site; every core's slot and its part of G, vel / m / v through the table.
static void check_loss_cot(const LossCotParams &p, dim3 g, dim3 b, size_t shm) {
  scan(&p, sizeof p, "LossCotParams");
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64 || p.f_bpad < p.b_pad || p.L < 1) die("LossCotParams: b %d b_pad %d f_bpad %d L %d", p.b, p.b_pad, p.f_bpad, p.L);
  if (p.act_fn < 0 || p.act_fn > 2 || p.loss_fn < 0 || p.loss_fn > 2) die("LossCotParams: act_fn %d loss_fn %d", p.act_fn, p.loss_fn);
  if (g.y != 1 || g.z != 1 || (size_t)g.x * b.x < (size_t)p.b_pad) die("loss_cot_kernel: grid %u x %u for b_pad %d", g.x, b.x, p.b_pad);
  if (shm < loss_cot_lds_bytes(p.L) || shm < (size_t)2 * p.L * b.x * 4) die("loss_cot_kernel: %zu bytes of LDS for L %d", shm, p.L);
  need(p.f, ((size_t)(p.L - 1) * p.f_bpad + p.b) * 4, "LossCotParams.f");
  need(p.y, (size_t)p.b * 4, "LossCotParams.y");
  need(p.cot, (size_t)p.L * p.b_pad * 4, "LossCotParams.cot");
}
static void check_optim_step(const OptimStepParams &p, dim3 g, dim3 b) {
  scan(&p, sizeof p, "OptimStepParams");
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N) die("OptimStepParams: N %d D %d L %d l_pos %d", p.N, p.D, p.L, p.l_pos);
  if (g.x != (unsigned)p.N || g.y != 1 || g.z != 1 || b.x != 256) die("optim_step_kernel: grid %u block %u for N %d", g.x, b.x, p.N);
  if (p.kind != TNML_OPT_SGD && p.kind != TNML_OPT_ADAM) die("OptimStepParams: kind %d", p.kind);
  if (p.kind == TNML_OPT_ADAM && (p.clip || !p.s0 || !p.s1)) die("OptimStepParams: Adam with clip %d, m %p, v %p", p.clip, (void *)p.s0, (void *)p.s1);
  if (p.kind == TNML_OPT_ADAM && !(p.corr1 > 0 && p.corr1 <= 1 && p.corr2 > 0 && p.corr2 <= 1)) die("OptimStepParams: bias corrections %g %g", p.corr1, p.corr2);
  if (p.kind == TNML_OPT_SGD && (p.mu > 0) != (p.s0 != nullptr)) die("OptimStepParams: momentum %g with vel %p", p.mu, (void *)p.s0);
  need(p.tab, (size_t)2 * p.N * 4, "OptimStepParams.tab");
  size_t off = 0;
  for (int i = 0; i < p.N; ++i) {
    const int ml = i == 0 ? 1 : p.tab[i - 1], mr = i == p.N - 1 ? 1 : p.tab[i];
    if (ml < 1 || mr < 1) die("OptimStepParams: site %d is %d x %d", i, ml, mr);
    const size_t ne = (size_t)ml * p.D * mr * (i == p.l_pos ? p.L : 1);
    if ((size_t)p.tab[p.N + i] != off) die("OptimStepParams: core %d at offset %d, the flat layout has it at %zu", i, p.tab[p.N + i], off);
    if (i == p.l_pos) need(p.labcore, ne * 4, "OptimStepParams.labcore");
    else {
      if (ne > p.core_stride) die("OptimStepParams: core %d of %zu floats in a slot of %zu", i, ne, p.core_stride);
      need(p.cores + (size_t)i * p.core_stride, ne * 4, "OptimStepParams.cores");
    }
    need(p.G + off, ne * 4, "OptimStepParams.G");
    if (p.s0) need(p.s0 + off, ne * 4, "OptimStepParams.s0");
    if (p.s1) need(p.s1 + off, ne * 4, "OptimStepParams.s1");
    if (p.skip) need(p.skip, 4, "OptimStepParams.skip");
    if (p.renorm != 0 && p.renorm != 1) die("OptimStepParams: renorm %d", p.renorm);
    off += ne;
  }
}

// ---- call trace ----------------------------------------------------------------------------------------------------------------
static FILE *g_tr = nullptr;
static long g_tr_lines = 0;
static bool tracing() {
  static const bool on = [] { const char *f = getenv("TNML_SAN_TRACE"); return f && *f && (g_tr = fopen(f, "w")); }();
  return on;
}
static void tr(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void tr(const char *fmt, ...) {
  if (!tracing()) return;
  va_list ap;
  va_start(ap, fmt);
  vfprintf(g_tr, fmt, ap);
  va_end(ap);
  if (fmt[strlen(fmt) - 1] == '\n') ++g_tr_lines;
}
static std::string dp(const void *p) {
  if (!p) return "0";
  if (!in_arena(p)) return "host";
  char b[24];
  snprintf(b, sizeof b, "@%zx", (size_t)((const char *)p - g_base));
  return b;
}
// streams (kind 0) and events (kind 1) are handles to their number in the order of creation; -1: the null stream
static void *new_handle(int kind) { static long next[2]; long *h = (long *)malloc(sizeof(long)); *h = next[kind]++; return h; }
static long id(const void *h) { return h ? *(const long *)h : -1; }
#define I(f) tr(" " #f "=%lld", (long long)p.f);
#define R(f) tr(" " #f "=%.17g", (double)p.f);
#define P(f) tr(" " #f "=%s", dp(p.f).c_str());
#define V(f) tr(" " #f "=[%s %d %d %d %d %d]", dp(p.f.base).c_str(), p.f.n_in, p.f.n_out, p.f.s_in, p.f.s_d, p.f.s_out);
static void tr_struct(const NarrowParams &p) {
  I(L) I(D) I(h) I(g) I(s) I(m) I(bsize) I(l2_flag) R(lr) R(wd) R(inv_b_global) P(red) V(lab) V(pl) P(Nh) P(Ng) P(Bnew)
  P(out_behind) I(ob_s_h) I(ob_s_d) I(ob_s_m) P(out_ahead) I(oa_s_m) I(oa_s_d) I(oa_s_g) P(Nh_new) P(metrics) P(dbg) P(stamps)
  P(counters) P(Bdirect) I(stop_after_update) I(fused) I(prep_ready) P(slabs) I(nslabs) I(slab_stride) I(nred) P(red_out) P(prepB)
  P(prepG) P(sync) R(trunc_thr) I(left_dir) P(m_out) R(chol_thr) R(svd_stop2) P(status) I(wait_count) I(pipe) I(z_first) I(z_rows)
  I(zsize) P(zred) V(zcore) P(flag) I(token) I(persist) I(write_ahead) I(persist_off) I(Mcap) P(prepRaw) P(pready) I(pwant) P(Apub)
  P(aflag) P(coreflag) I(coretoken) P(zpoll_flag) I(zpoll_want) P(done_flag) I(done_val) P(abort_flag)
}
static void tr_struct(const WideParams &p) {
  I(b) I(b_pad) I(L) I(h) I(g) I(hp) I(gp) I(do_f) I(do_ext) I(first_ext) I(act_fn) I(loss_fn) R(T) P(x_km1) P(x_k) P(x_kp1) P(Hprev)
  P(Hcur) P(Gprev) P(Gcur) P(Bprev) V(ext_core) P(y) P(f) P(slabs) I(slab_stride) I(bsize) P(stamps)
}
static void tr_struct(const WidePipeParams &p) {
  I(b) I(b_pad) I(L) I(hj) I(gj) I(gn) I(hprev) I(first) I(do_ext) I(first_ext) I(do_f) I(wait_flag) I(do_z) I(act_fn) I(loss_fn) R(T)
  P(x_jm1) P(x_j) P(x_jp1) P(x_jp2) P(Eprev) P(Ecur) V(ext_core) P(Gj) P(Gn) P(Bnew) P(y) P(f) I(zsize) I(slab_stride) P(slabs) P(gslabs)
  P(zred) P(gcnt) P(tcnt) I(nwide) I(gsz) I(ngroups) I(one_level) I(slice_red) I(slice_S) I(slice_R) P(sarrive) P(sdone) I(wg0) I(tiles_per_wg) I(ntiles) P(flag) I(token) P(status) I(persist)
  P(coreflag) I(corewant) P(zready) I(zpublish) P(abort_flag) P(stamps)
}
static void tr_struct(const PersistHelperParams &p) {
  I(zr) I(s) I(g) I(L) I(h) I(l2_flag) P(W) V(lab) V(pl) P(Ng) P(T) P(TN) P(Z) P(prepRaw) P(prepB) P(prepG) P(Apub) P(flag) I(want)
  P(aflag) I(awant) P(zready) I(zwant) P(tcnt) P(pcnt) P(abort_flag) P(status) P(stamps)
}
static void tr_struct(const PersistStep &p) { tr(" n:"); tr_struct(p.n); tr(" w:"); tr_struct(p.w); tr(" t:"); tr_struct(p.t); tr(" shape=%d", p.shape); }
static void tr_struct(const PrepParams &p) { V(lab) V(pl) P(Nh) P(Ng) I(h) I(g) I(s) I(L) I(l2_flag) P(prepB) P(prepG) I(nparts) }
static void tr_struct(const MeetParams &p) { P(Lenv) P(Renv) P(x) P(core) P(f) I(b) I(b_pad) I(ml) I(mr) I(D) I(L) I(rows_per_chunk) }
static void tr_struct(const InputGradParams &p) {
  P(bond) P(cores) P(labcore) P(X) P(cot) P(stack) P(g) P(cf) I(core_stride) I(b) I(b_pad) I(x_bpad) I(N) I(D) I(L) I(l_pos) I(cap) I(mb)
}
static void tr_struct(const CoreGradParams &p) {
  P(tab) P(cores) P(labcore) P(X) P(cot) P(stackP) P(stackQ) P(G) P(cf) I(core_stride) I(b) I(b_pad) I(x_bpad) I(N) I(D) I(L) I(l_pos) I(cap)
  I(mb) I(first)
}
static void tr_struct(const InputGradScaledParams &p) { tr_struct(p.base); P(estack) }
static void tr_struct(const CoreGradScaledParams &p) { tr_struct(p.base); P(estack) }
static void tr_struct(const ScaledPredParams &p) { P(bond) P(cores) P(labcore) P(X) P(mant) P(expo) P(f) I(core_stride) I(b) I(b_pad) I(N) I(D) I(L) I(l_pos) I(mb) }
static void tr_struct(const LossCotParams &p) { P(f) P(y) P(cot) I(L) I(b) I(b_pad) I(f_bpad) I(act_fn) I(loss_fn) R(T) }
static void tr_struct(const OptimStepParams &p) {
  P(tab) P(cores) P(labcore) P(G) P(s0) P(s1) I(core_stride) I(N) I(D) I(L) I(l_pos) I(kind) I(clip) R(lr) R(wd) R(mu) R(beta1) R(beta2) R(eps)
  R(corr1) R(corr2)
  if (p.renorm || p.skip) { I(renorm) P(skip) }                  // (likelihood training alone: the traces of the discriminative path stay as they were)
}
static void tr_struct(const AlgebraParams &p) {
  I(N) I(D) I(L) I(l_pos) I(n_prod) I(metric_sites) I(lds_m2) P(bond) P(off) P(w_plain) P(w_lab) P(v_plain) P(v_lab) P(metric) P(stage) I(stage_stride)
  P(half_E) I(half_stride) P(half_expo) P(out) P(status) R(alpha) R(beta) P(out_cores) P(out_lab) I(core_stride) I(lab_elems)
}
static void tr_struct(const SampleParams &p) {
  I(N) I(D) I(L) I(l_pos) I(K) I(n) I(n_given) I(n_tiles) I(n_slots) I(phase) I(lds_m) P(bond) P(cores) P(lab) I(core_stride) P(S) P(phi) P(w) P(slot_class)
  P(env_shared) P(env_slots) I(env_stride) P(stage) I(stage_stride) P(tile_slot) P(tile_samples) P(classes) P(given) P(u) I(seed) P(levels) P(labels) P(logp) P(status)
}
static void tr_struct(const SampleMaskedParams &p) {
  I(N) I(D) I(L) I(l_pos) I(K) I(n) I(T) I(n_tiles) I(lds_m) I(mask_rows) P(bond) P(cores) P(lab) I(core_stride) P(S) P(phi) P(w) P(tile_class) P(tile_rows)
  P(mask) P(known) P(stack) I(env_stride) P(E) P(u) I(seed) P(levels) P(labels) P(logp0) P(status)
}
static void tr_struct(const SiteCondParams &p) {
  tr_struct(p.m);
  P(values) P(lf_next) P(q) P(stats) P(mode)
}
static void tr_struct(const MaskedGradParams &p) {
  tr_struct(p.m);
  P(off) P(wrow) P(lf_next) P(part) I(total) P(status)
}
static void tr_struct(const MaskedGradReduceParams &p) { P(part) P(acc) P(G) I(total) I(n_tiles) I(first) I(last) P(status) }
static void tr_struct(const LogNormParams &p) {
  I(N) I(D) I(L) I(l_pos) I(metric_sites) I(lds_m) I(mode) P(tab) P(cores) P(lab) I(core_stride) P(metric) P(envL) P(envR) P(expL) P(expR) I(env_stride)
  P(G) P(out) P(status)
}
static void tr_struct(const PairParams &p) {
  tr_struct(p.e);
  I(e.class_plus1) I(K) I(n_rows) P(phi) P(w) P(values) P(rows) P(B) P(q1) P(stats1) P(Q) P(qexp) P(stats)
}
static void tr_struct(const NllCotParams &p) { P(f) P(y) P(cot) P(terms) P(bad) I(L) I(b) I(b_pad) I(f_bpad) I(off) I(batch) }
static void tr_struct(const InputGradPixels &p) { P(g) P(data) P(idx) P(out) I(b) I(N) I(D) }
static void tr_struct(const BigExtArgs &p) { P(Eprev) P(x_km1) P(x_k) V(A) I(b_pad) P(Ecur) P(Pk) }
static void tr_struct(const ChainSite &p) { I(core_off) I(is_label) I(n_in) I(n_out) I(s_in) I(s_d) I(s_out) I(x_site) I(env_out_off) }
static void tr_struct(const NormChainSite &p) { I(core_off) I(n_in) I(n_out) I(s_in) I(s_d) I(s_out) I(env_out_off) }
#undef I
#undef R
#undef P
#undef V
template <class S> static void tr_rows(const char *what, const S *rows, int n) {
  for (int i = 0; i < n; ++i) { tr("  %s %d:", what, i); tr_struct(rows[i]); tr("\n"); }
}
// every argument of a launch, by the parameter types of the kernel's demangled signature
static void tr_launch(const std::string &name, dim3 g, dim3 b, size_t shm, hipStream_t st, void **args) {
  const size_t lp = name.find('('), rp = name.rfind(')');
  tr("launch %s grid=%u,%u,%u block=%u,%u,%u lds=%zu stream=s%ld", name.substr(0, lp).c_str(), g.x, g.y, g.z, b.x, b.y, b.z, shm, id(st));
  std::vector<std::string> types;
  for (size_t i = lp + 1, from = i, depth = 0; lp != std::string::npos && i <= rp; ++i) {
    const char ch = name[i];
    depth += (ch == '<') - (ch == '>');
    if ((ch == ',' && !depth) || i == rp) { if (i > from) types.push_back(name.substr(from, i - from)); from = i + 1; }
  }
  for (size_t i = 0; i < types.size(); ++i) {
    const std::string &t = types[i];
    auto is = [&](const char *s) { return t.find(s) != std::string::npos; };
    tr(" |");
    if (is("*")) tr(" %s", dp(*(void **)args[i]).c_str());
    else if (is("NarrowParams")) tr_struct(*(const NarrowParams *)args[i]);
    else if (is("WidePipeParams")) tr_struct(*(const WidePipeParams *)args[i]);
    else if (is("WideParams")) tr_struct(*(const WideParams *)args[i]);
    else if (is("PrepParams")) tr_struct(*(const PrepParams *)args[i]);
    else if (is("MeetParams")) tr_struct(*(const MeetParams *)args[i]);
    else if (is("InputGradScaledParams")) tr_struct(*(const InputGradScaledParams *)args[i]);
    else if (is("CoreGradScaledParams")) tr_struct(*(const CoreGradScaledParams *)args[i]);
    else if (is("ScaledPredParams")) tr_struct(*(const ScaledPredParams *)args[i]);
    else if (is("InputGradParams")) tr_struct(*(const InputGradParams *)args[i]);
    else if (is("CoreGradParams")) tr_struct(*(const CoreGradParams *)args[i]);
    else if (is("InputGradPixels")) tr_struct(*(const InputGradPixels *)args[i]);
    else if (is("LossCotParams")) tr_struct(*(const LossCotParams *)args[i]);
    else if (is("OptimStepParams")) tr_struct(*(const OptimStepParams *)args[i]);
    else if (is("BigExtArgs")) tr_struct(*(const BigExtArgs *)args[i]);
    else if (is("AlgebraParams")) tr_struct(*(const AlgebraParams *)args[i]);
    else if (is("SampleParams")) tr_struct(*(const SampleParams *)args[i]);
    else if (is("SampleMaskedParams")) tr_struct(*(const SampleMaskedParams *)args[i]);
    else if (is("MaskedGradReduceParams")) tr_struct(*(const MaskedGradReduceParams *)args[i]);
    else if (is("MaskedGradParams")) tr_struct(*(const MaskedGradParams *)args[i]);
    else if (is("SiteCondParams")) tr_struct(*(const SiteCondParams *)args[i]);
    else if (is("PairParams")) tr_struct(*(const PairParams *)args[i]);
    else if (is("NllCotParams")) tr_struct(*(const NllCotParams *)args[i]);
    else if (is("LogNormParams")) tr_struct(*(const LogNormParams *)args[i]);
    else if (is("CoreView")) { const CoreView &v = *(const CoreView *)args[i]; tr(" [%s %d %d %d %d %d]", dp(v.base).c_str(), v.n_in, v.n_out, v.s_in, v.s_d, v.s_out); }
    else if (is("BigFrontTiles")) tr(" %d %d", ((int *)args[i])[0], ((int *)args[i])[1]);
    else if (is("float")) tr(" %.9g", *(float *)args[i]);
    else if (is("long")) tr(" %lld", *(long long *)args[i]);
    else if (is("int") || is("bool")) tr(" %d", *(int *)args[i]);
    else tr(" ?");
  }
  tr("\n");
  // tables and record arrays behind the first argument (their length is the second)
  if (types.size() < 2 || types[0].find('*') == std::string::npos) return;
  const void *tab = *(void **)args[0];
  const int n = *(int *)args[1];
  if (types[0].find("NormChainSite") != std::string::npos) tr_rows("site", (const NormChainSite *)tab, n);
  else if (types[0].find("ChainSite") != std::string::npos) tr_rows("site", (const ChainSite *)tab, n);
  else if (types[0].find("PersistStep") != std::string::npos) tr_rows("step", (const PersistStep *)tab, n + 1);      // (record n: the batch side's prologue)
}
static void tr_copy(const char *what, hipMemcpyKind k, const void *d, const void *s, size_t n, hipStream_t st) {
  const char *kind = k == hipMemcpyHostToDevice ? "H2D" : k == hipMemcpyDeviceToHost ? "D2H" : k == hipMemcpyDeviceToDevice ? "D2D" : k == hipMemcpyHostToHost ? "H2H" : "default";
  tr("%s %s dst=%s src=%s n=%zu stream=s%ld\n", what, kind, dp(d).c_str(), dp(s).c_str(), n, id(st));
}
}  // namespace san
using namespace san;

extern "C" {
// ---- registration and launch ----------------------------------------------------------------------------------------------------
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *dev_name, unsigned, void *, void *, void *, void *, int *) {
  int st = 0;
  char *dm = abi::__cxa_demangle(dev_name, nullptr, nullptr, &st);
  std::string nm = dm ? dm : dev_name;
  free(dm);
  for (size_t at; (at = nm.find("(anonymous namespace)::")) != std::string::npos;) nm.erase(at, 23);
  g_kernels[host_fn] = nm;
}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
static thread_local struct { dim3 g, b; size_t shm; hipStream_t st; } t_cfg;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t shm, hipStream_t st) { t_cfg = {g, b, shm, st}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *g, dim3 *b, size_t *shm, hipStream_t *st) { *g = t_cfg.g; *b = t_cfg.b; *shm = t_cfg.shm; *st = t_cfg.st; return hipSuccess; }

hipError_t hipLaunchKernel(const void *fn, dim3 g, dim3 b, void **args, size_t shm, hipStream_t st) {
  auto it = g_kernels.find(fn);
  const std::string name = it == g_kernels.end() ? "?" : it->second;
  g_ctx = name.c_str();
  const unsigned long long thr = (unsigned long long)b.x * b.y * b.z;
  if (g.x < 1 || g.y < 1 || g.z < 1 || g.y > 65535 || g.z > 65535 || thr < 1 || thr > 1024 || shm > 160 * 1024)
    die("illegal launch: grid (%u,%u,%u) block (%u,%u,%u) dynamic LDS %zu", g.x, g.y, g.z, b.x, b.y, b.z, shm);
  const std::string key = name.substr(0, name.find('('));
  g_launches[key]++;
  if (tracing()) tr_launch(name, g, b, shm, st, args);
  auto has = [&](const char *s) { return name.find(s) != std::string::npos; };
  if (has("sweep_persist") || has("persist_update_kernel") || has("persist_helper_kernel") || has("persist_batch_kernel")) {
    const PersistStep *st = *(const PersistStep **)args[0];
    const int n = *(int *)args[1];
    need(st, (size_t)(n + 1) * sizeof(PersistStep), "persistent step records");
    for (int k = 0; k < n; ++k) { check_narrow(st[k].n); check_pipe(st[k].w); scan(&st[k].t, sizeof st[k].t, "PersistHelperParams"); }
    check_pipe(st[n].w);                 // the prologue of the batch side
    for (int k = 0; k <= n; ++k)         // a marked record needs a kernel compiled for its shape: the launched one
      if (st[k].shape && (st[k].shape < 1 || st[k].shape > kNumPersistShapes || k == n || !has("sweep_persist_kernel<") || has("DynShape")))
        die("record %d carries shape %d in a launch of %s", k, st[k].shape, name.c_str());
    g_last_persist = st; g_last_persist_n = n;
  } else if (has("step_pipe_kernel")) {
    const NarrowParams &n = *(const NarrowParams *)args[0];
    const WidePipeParams &w = *(const WidePipeParams *)args[1];
    if (n.bsize > 0) check_narrow(n);    // (a prologue launch carries no update)
    check_pipe(w);
    if (g.x > 256) die("step_pipe_kernel: %u workgroups cannot be co-resident on 256 CUs", g.x);
  } else if (has("label_meet_kernel")) {
    check_meet(*(const MeetParams *)args[0], g, b, shm);
  } else if (has("input_grad_scaled_kernel")) {
    check_input_grad_scaled(*(const InputGradScaledParams *)args[0], g, b, shm);
  } else if (has("core_grad_chain_scaled_kernel")) {
    check_core_grad_scaled(*(const CoreGradScaledParams *)args[0], g, b, shm);
  } else if (has("scaled_pred_kernel")) {
    check_scaled_pred(*(const ScaledPredParams *)args[0], g, b, shm);
  } else if (has("input_grad_kernel")) {
    check_input_grad(*(const InputGradParams *)args[0], g, b, shm);
  } else if (has("core_grad_chain_kernel") || has("core_grad_reduce_kernel")) {
    check_core_grad(*(const CoreGradParams *)args[0], g, b, shm, has("core_grad_reduce_kernel"));
  } else if (has("loss_cot_kernel")) {
    check_loss_cot(*(const LossCotParams *)args[0], g, b, shm);
  } else if (has("optim_step_kernel")) {
    check_optim_step(*(const OptimStepParams *)args[0], g, b);
  } else if (has("orth_load_kernel") || has("orth_chain_kernel") || has("orth_store_kernel")) {
    check_orth(*(const OrthParams *)args[0], g, b, shm, has("orth_chain_kernel") ? 1 : has("orth_store_kernel") ? 2 : 0);
  } else if (has("inner_chain_kernel") || has("inner_meet_kernel") || has("sum_place_kernel")) {
    check_algebra(*(const AlgebraParams *)args[0], g, b, shm, has("inner_chain_kernel") ? 0 : has("inner_meet_kernel") ? 1 : 2);
  } else if (has("sample_env_kernel") || has("sample_walk_kernel")) {
    check_sample(*(const SampleParams *)args[0], g, b, shm, has("sample_walk_kernel"));
  } else if (has("sample_env_masked_kernel") || has("sample_walk_masked_kernel")) {
    check_sample_masked(*(const SampleMaskedParams *)args[0], g, b, shm, has("sample_walk_masked_kernel"));
  } else if (has("masked_grad_reduce_kernel")) {
    check_masked_grad_reduce(*(const MaskedGradReduceParams *)args[0], g, b);
  } else if (has("masked_grad_kernel")) {
    check_masked_grad(*(const MaskedGradParams *)args[0], g, b, shm);
  } else if (has("site_cond_kernel")) {
    check_site_cond(*(const SiteCondParams *)args[0], g, b, shm);
  } else if (has("pair_close_kernel") || has("pair_walk_kernel") || has("pair_stats_kernel")) {
    check_pair(*(const PairParams *)args[0], g, b, shm, has("pair_close_kernel") ? 0 : has("pair_walk_kernel") ? 1 : 2);
  } else if (has("lognorm_env_kernel") || has("lognorm_grad_kernel")) {
    check_lognorm(*(const LogNormParams *)args[0], g, b, shm, has("lognorm_grad_kernel"));
  } else if (has("nll_cot_kernel")) {
    check_nll_cot(*(const NllCotParams *)args[0], g, b);
  } else if (has("nll_sum_kernel")) {            // (terms, bad, n, acc)
    const int n = *(int *)args[2];
    if (n < 1 || g.x != 1 || b.x != 256) die("nll_sum_kernel: n %d grid %u block %u", n, g.x, b.x);
    need(*(const double **)args[0], (size_t)n * 8, "nll_sum: terms"); need(*(const int **)args[1], (size_t)n * 4, "nll_sum: flags");
    need(*(double **)args[3], 2 * 8, "nll_sum: sums");
  } else if (has("nll_record_kernel")) {         // (acc, out, status, rec, skip)
    if (g.x != 1) die("nll_record_kernel: grid %u", g.x);
    need(*(const double **)args[0], 2 * 8, "nll_record: sums"); need(*(const double **)args[1], 2 * 8, "nll_record: sign and log|Z|");
    need(*(const int **)args[2], 2 * 4, "nll_record: status words"); need(*(double **)args[3], 4 * 8, "nll_record: the step's slot");
    need(*(int **)args[4], 4, "nll_record: skip word");
  } else if (has("input_grad_onehot_kernel")) {   // (f, f_bpad, L, b, cot, b_pad)
    const int fbp = *(int *)args[1], L = *(int *)args[2], bb = *(int *)args[3], bp = *(int *)args[5];
    if (bb < 1 || bb > bp || bp > fbp || (size_t)g.x * b.x < (size_t)bp) die("input_grad_onehot_kernel: b %d b_pad %d f_bpad %d grid %u x %u", bb, bp, fbp, g.x, b.x);
    need(*(const float **)args[0], ((size_t)(L - 1) * fbp + bb) * 4, "one-hot: f"); need(*(float **)args[4], (size_t)L * bp * 4, "one-hot: cot");
  } else if (has("input_grad_pixels_kernel")) {
    const InputGradPixels &q = *(const InputGradPixels *)args[0];
    scan(&q, sizeof q, "InputGradPixels");
    if (q.b < 1 || q.N < 1 || q.D < 2 || q.D > kMaxD || (size_t)g.x * b.x < (size_t)q.b * q.N) die("input_grad_pixels_kernel: b %d N %d D %d grid %u x %u", q.b, q.N, q.D, g.x, b.x);
    need(q.g, (size_t)q.b * q.N * q.D * 4, "pixels: g"); need(q.out, (size_t)q.b * q.N * 4, "pixels: out"); need(q.idx, (size_t)q.b * 4, "pixels: index list");
    for (int i = 0; i < q.b; ++i) need(q.data + (size_t)q.idx[i] * q.N, (size_t)q.N * 4, "pixels: dataset row");
  } else if (has("narrow_step_kernel")) {
    check_narrow(*(const NarrowParams *)args[0]);
  } else if (has("wide_step") || has("f_only_kernel")) {
    // (the MFMA kernel's grid carries D*D slice workgroups behind the nblk sample workgroups)
    check_wide(*(const WideParams *)args[0], has("wide_step_mfma_kernel") ? *(int *)args[2] : (int)g.x, has("f_only_kernel"));
  } else if (has("env_chain_roles_kernel")) {
    check_chain(*(const ChainSite **)args[0], *(int *)args[1], *(const float **)args[2], *(const float **)args[3], *(const float **)args[4],
                *(float **)args[5], *(float **)args[6], *(int *)args[7], 1);
    if ((int)g.x * 16 != *(int *)args[7]) die("chain grid %u x 16 samples != b_pad %d", g.x, *(int *)args[7]);
  } else if (has("env_chain_kernel")) {
    check_chain(*(const ChainSite **)args[0], *(int *)args[1], *(const float **)args[2], *(const float **)args[3], *(const float **)args[4],
                has("<true>") ? nullptr : *(float **)args[5], *(float **)args[6], *(int *)args[8], *(int *)args[9]);
  } else if (has("big_merge_wd_kernel") || has("big_merge_wd_mfma_kernel")) { // (NarrowParams, merged tensor out, NL, PR, workspace, block partials): the factored chain's entry
    const NarrowParams &n = *(const NarrowParams *)args[0];
    check_narrow(n);
    need(*(float **)args[1], (size_t)n.bsize * 4, "large-tensor path: merged tensor");
    if (n.l2_flag) {
      need(*(const double **)args[2], (size_t)n.h * kD * n.s * n.L * 8, "large-tensor path: NL");
      need(*(const double **)args[3], (size_t)n.s * kD * n.g * 8, "large-tensor path: PR");
    }
    if (g.x > (unsigned)kBigParts) die("big_merge_wd_kernel: %u blocks leave partials, room for %d", g.x, kBigParts);
    need(*(double **)args[5], (size_t)g.x * 3 * 8, "large-tensor path: block partials");
  } else if (has("big_wd_kernel")) {       // (NarrowParams, merged tensor, Nh^T.B, workspace, block partials): the classic chain's entry
    const NarrowParams &n = *(const NarrowParams *)args[0];
    check_narrow(n);
    need(*(const float **)args[1], (size_t)n.bsize * 4, "large-tensor path: merged tensor");
    if (n.l2_flag) need(*(const double **)args[2], (size_t)n.bsize * 8, "large-tensor path: Nh^T.B");
    if (g.x > (unsigned)kBigParts) die("big_wd_kernel: %u blocks leave partials, room for %d", g.x, kBigParts);
    need(*(double **)args[4], (size_t)g.x * 3 * 8, "large-tensor path: block partials");
  } else if (has("big_nlpr_kernel")) {     // (NarrowParams, NL, PR)
    const NarrowParams &n = *(const NarrowParams *)args[0];
    check_narrow(n);
    need(*(double **)args[1], (size_t)n.h * kD * n.s * n.L * 8, "big_nlpr: NL");
    need(*(double **)args[2], (size_t)n.s * kD * n.g * 8, "big_nlpr: PR");
    if (*(double **)args[2] < *(double **)args[1] + (size_t)n.h * kD * n.s * n.L) die("big_nlpr: PR overlaps NL");
  } else if (has("big_gram_kernel")) {     // (B_new, n, len, si, sx, gram)
    const int n = *(int *)args[1], len = *(int *)args[2];
    need(*(const float **)args[0], (size_t)n * len * 4, "large-tensor path: B_new");
    need(*(double **)args[5], (size_t)8 * kBigMaxN * kBigMaxN * 8, "large-tensor path: partial Gram matrices");
    if (n > kBigMaxN || (n & 1)) die("big_gram_kernel: short side %d", n);
    if ((int)g.x * 16 < n || (int)g.y * 16 < n) die("big_gram_kernel: grid (%u, %u) of 16 x 16 tiles for n = %d", g.x, g.y, n);
    if (*(unsigned **)args[6]) need(*(unsigned **)args[6], 4, "big_gram: flag word of the side stream");
  } else if (has("big_ext_kernel")) {      // (BigExtArgs: E_{k-1}, x_{k-1}, x_k, core view, b_pad, E_k, P'_k)
    check_big_ext(*(const BigExtArgs *)args[0], shm);
    const BigExtArgs &a = *(const BigExtArgs *)args[0];
    if ((int)g.x * 64 != a.b_pad) die("big_ext_kernel: grid %u x 64 samples != b_pad %d", g.x, a.b_pad);
    if ((int)g.y * 16 < a.A.n_out) die("big_ext_kernel: %u workgroup rows of 16 for %d bond indices", g.y, a.A.n_out);
  } else if (has("big_contract_kernel")) { // (Z, core view, ncols, red)
    const CoreView &A = *(const CoreView *)args[1];
    const size_t nc = *(int *)args[2];
    need(*(const float **)args[0], ((size_t)A.n_in * kD * nc + kMetricSlots) * 4, "big_contract: Z");
    need(A.base, view_extent(A, 1) * 4, "big_contract: core");
    need(*(float **)args[3], ((size_t)A.n_out * nc + kMetricSlots) * 4, "big_contract: raw gradient");
    if (shm < (size_t)A.n_in * kD * 8 * 4) die("big_contract_kernel: %zu bytes of LDS", shm);
    if ((size_t)g.x * 64 < nc || (int)g.y * 8 < A.n_out) die("big_contract_kernel: grid (%u, %u) for %zu columns, %d rows", g.x, g.y, nc, A.n_out);
  } else if (has("big_front_kernel")) {    // (NarrowParams, NL, PR, Z, core view, ncols, red, tile split, BigExtArgs, poll flag, poll value, ext acquire)
    const NarrowParams &n = *(const NarrowParams *)args[0];
    check_narrow(n);
    const CoreView &A = *(const CoreView *)args[4];
    const size_t nc = *(int *)args[5];
    struct Tiles { int contract_blocks, ext_blocks; };
    const Tiles &ft = *(const Tiles *)args[7];
    if (n.l2_flag) {
      need(*(double **)args[1], (size_t)n.h * kD * n.s * n.L * 8, "big_front: NL");
      need(*(double **)args[2], (size_t)n.s * kD * n.g * 8, "big_front: PR");
      if (*(double **)args[2] < *(double **)args[1] + (size_t)n.h * kD * n.s * n.L) die("big_front: PR overlaps NL");
      if ((int)g.x <= ft.contract_blocks + ft.ext_blocks) die("big_front_kernel: grid %u leaves no workgroup for the L2 products", g.x);
    }
    need(*(const float **)args[3], ((size_t)A.n_in * kD * nc + kMetricSlots) * 4, "big_front: Z");
    need(A.base, view_extent(A, 1) * 4, "big_front: core");
    need(*(float **)args[6], ((size_t)A.n_out * nc + kMetricSlots) * 4, "big_front: raw gradient");
    if ((size_t)A.n_out * nc != (size_t)n.bsize) die("big_front_kernel: gradient %d x %zu, merged tensor %d", A.n_out, nc, n.bsize);
    if ((size_t)ft.contract_blocks * 4 < (size_t)((A.n_out + 15) / 16) * ((nc + 15) / 16)) die("big_front_kernel: %d workgroups for the contraction's tiles", ft.contract_blocks);
    if (*(const unsigned **)args[9]) need(*(const unsigned **)args[9], 4, "big_front: sequence number of the side stream");
    const BigExtArgs &ea = *(const BigExtArgs *)args[8];
    if (ft.ext_blocks) {
      check_big_ext(ea, (size_t)1 << 20);                      // (no LDS in this form)
      if (ea.b_pad % 64 || (size_t)ft.ext_blocks * 4 < (size_t)((ea.A.n_out + 15) / 16) * (ea.b_pad / 16)) die("big_front_kernel: %d workgroups for the extension's tiles, b_pad %d", ft.ext_blocks, ea.b_pad);
    }
  } else if (has("big_signal_kernel")) {   // (flag, value)
    need(*(unsigned **)args[0], 4, "big_signal: flag word");
  } else if (has("big_gate_kernel")) {     // (flag, want, status)
    need(*(const unsigned **)args[0], 4, "big_gate: flag word"); need(*(int **)args[2], 4, "big_gate: status");
  } else if (has("reduce_slabs")) {        // (slabs, nblk, slab_stride, n, red)
    const int nblk = *(int *)args[1], stride = *(int *)args[2], n = *(int *)args[3];
    if (n > stride) die("reduce_slabs: %d elements of a slab of %d", n, stride);
    need(*(const float **)args[0], (size_t)nblk * stride * 4, "slabs"); need(*(float **)args[4], (size_t)n * 4, "reduced slab");
  }
  g_ctx = "";
  return hipSuccess;
}

// ---- memory ----------------------------------------------------------------------------------------------------------------------
hipError_t hipMalloc(void **p, size_t n) {
  if (alloc_fails()) return hipErrorOutOfMemory;
  if (!g_base) {
    g_base = (char *)mmap(nullptr, kArena, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (g_base == MAP_FAILED) { perror("mmap"); abort(); }
  }
  const size_t sz = (n + 4095) & ~(size_t)4095;
  if (g_used + sz + kGap > kArena) return hipErrorOutOfMemory;
  char *q = g_base + g_used + kGap;
  if (sz && mprotect(q, sz, PROT_READ | PROT_WRITE)) { perror("mprotect"); abort(); }
  g_used += sz + kGap;
  g_alloc[(uintptr_t)q] = n;
  *p = q;
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  if (!p) return hipSuccess;
  auto it = g_alloc.find((uintptr_t)p);
  if (it == g_alloc.end()) die("hipFree(%p): not the base of a live allocation", p);
  const size_t sz = (it->second + 4095) & ~(size_t)4095;
  if (sz) { madvise(p, sz, MADV_DONTNEED); mprotect(p, sz, PROT_NONE); }     // a later use faults
  g_alloc.erase(it);
  return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { if (alloc_fails()) return hipErrorOutOfMemory; *p = malloc(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
static void copy_checked(void *d, const void *s, size_t n, hipMemcpyKind k, const char *what) {
  g_ctx = what;
  if (n == 0) return;
  const bool dd = k == hipMemcpyHostToDevice || k == hipMemcpyDeviceToDevice || (k == hipMemcpyDefault && in_arena(d));
  const bool sd = k == hipMemcpyDeviceToHost || k == hipMemcpyDeviceToDevice || (k == hipMemcpyDefault && in_arena(s));
  if (dd) need(d, n, "copy destination"); else if (in_arena(d)) die("host destination %p is device memory", d);
  if (sd) need(s, n, "copy source"); else if (in_arena(s)) die("host source %p is device memory", s);
  memmove(d, s, n);                        // host sides are checked by AddressSanitizer
  g_ctx = "";
}
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { tr_copy("memcpy", k, d, s, n, nullptr); copy_checked(d, s, n, k, "hipMemcpy"); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st) { tr_copy("memcpy_async", k, d, s, n, st); copy_checked(d, s, n, k, "hipMemcpyAsync"); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void *d, size_t dpitch, const void *s, size_t spitch, size_t w, size_t h, hipMemcpyKind k, hipStream_t st) {
  tr("memcpy2d_async rows=%zu dst_pitch=%zu src_pitch=%zu of ", h, dpitch, spitch);
  tr_copy("row", k, d, s, w, st);
  if (w > dpitch || w > spitch) die("hipMemcpy2DAsync: width %zu exceeds a pitch (%zu, %zu)", w, dpitch, spitch);
  for (size_t r = 0; r < h; ++r) copy_checked((char *)d + r * dpitch, (const char *)s + r * spitch, w, k, "hipMemcpy2DAsync");
  return hipSuccess;
}
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t st) {
  tr("memset dst=%s v=%d n=%zu stream=s%ld\n", dp(d).c_str(), v, n, id(st));
  g_ctx = "hipMemset";
  if (n) { need(d, n, "memset"); memset(d, v, n); }
  g_ctx = "";
  return hipSuccess;
}
hipError_t hipMemset(void *d, int v, size_t n) { return hipMemsetAsync(d, v, n, nullptr); }

// ---- device, streams, events -----------------------------------------------------------------------------------------------------
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600 *p, int) {
  memset(p, 0, sizeof *p);
  strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
  strcpy(p->name, "sanitizer stand-in for MI355X");
  p->multiProcessorCount = 256;
  p->sharedMemPerBlock = 160 * 1024;
  p->maxSharedMemoryPerMultiProcessor = 160 * 1024;
  p->totalGlobalMem = (size_t)288 << 30;
  p->warpSize = 64;
  p->maxThreadsPerBlock = 1024;
  return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "error (stub)"; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)new_handle(0); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { tr("stream_sync s%ld\n", id(s)); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { tr("stream_wait s%ld e%ld\n", id(s), id(e)); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)new_handle(1); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { tr("event_record e%ld s%ld\n", id(e), id(s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { tr("event_sync e%ld\n", id(e)); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.01f; return hipSuccess; }

// ---- RCCL: a one-rank world --------------------------------------------------------------------------------------------------------
ncclResult_t ncclGetUniqueId(ncclUniqueId *id) { memset(id, 7, sizeof *id); return ncclSuccess; }
ncclResult_t ncclCommInitRank(ncclComm_t *c, int n, ncclUniqueId, int r) { if (n != 1 || r != 0) return ncclInvalidArgument; *c = (ncclComm_t)malloc(8); return ncclSuccess; }
ncclResult_t ncclCommDestroy(ncclComm_t c) { free(c); return ncclSuccess; }
const char *ncclGetErrorString(ncclResult_t) { return "rccl (stub)"; }
ncclResult_t ncclAllReduce(const void *s, void *d, size_t count, ncclDataType_t t, ncclRedOp_t, ncclComm_t, hipStream_t st) {
  tr("allreduce send=%s recv=%s count=%zu stream=s%ld\n", dp(s).c_str(), dp(d).c_str(), count, id(st));
  g_ctx = "ncclAllReduce";
  ++g_allreduces;
  const size_t el = t == ncclFloat ? 4 : (t == ncclDouble ? 8 : 4);
  need(s, count * el, "send buffer"); need(d, count * el, "receive buffer");
  if (s != d) memmove(d, s, count * el);
  g_ctx = "";
  return ncclSuccess;
}

// ---- report ----------------------------------------------------------------------------------------------------------------------
void san_stub_report(void) {
  long total = 0;
  for (auto &kv : g_launches) total += kv.second;
  printf("san-stub: %ld launches checked (%zu kernels), %ld pointer extents checked, %zu live allocations\n", total, g_launches.size(), g_checked_ptrs, g_alloc.size());
  for (auto &kv : g_launches) printf("    %-60s %ld\n", kv.first.c_str(), kv.second);
  if (tracing()) { fflush(g_tr); printf("san-stub: call trace of %ld lines written\n", g_tr_lines); }
}
long san_stub_allreduces(void) { return g_allreduces; }
long san_stub_launches(const char *substr) {
  long n = 0;
  for (auto &kv : g_launches) if (kv.first.find(substr) != std::string::npos) n += kv.second;
  return n;
}
long san_stub_alloc_calls(void) { return g_alloc_calls; }
// the nth allocation call from now on fails once (0: withdraw a failure that has not fired); pending: it has not fired yet
void san_stub_fail_alloc(long nth) { g_fail_call = nth > 0 ? g_alloc_calls + nth : 0; }
int san_stub_fail_pending(void) { return g_fail_call != 0; }
void san_stub_poke_int(void *dev, int v) { need(dev, 4, "poke"); memcpy(dev, &v, 4); }
// tnml_sample_masked: forget the rows seen so far; every sample of a call of n samples in exactly one tile of the launches since, and
// that tile of its class (walk: the walk launches)
void san_stub_masked_reset(void) { g_masked_rows[0].clear(); g_masked_rows[1].clear(); }
void san_stub_masked_check(int walk, int n, const int32_t *classes) {
  std::vector<int> cls((size_t)n, INT_MIN);
  for (auto &r : g_masked_rows[walk ? 1 : 0]) {
    if (r.first >= n || cls[r.first] != INT_MIN) die("tnml_sample_masked: sample %d is in two tiles of the %s launches", r.first, walk ? "walk" : "environment");
    cls[r.first] = r.second;
  }
  for (int s = 0; s < n; ++s)
    if (cls[s] != (classes ? classes[s] : -1)) die("tnml_sample_masked: sample %d of class %d is in %s", s, classes ? classes[s] : -1, cls[s] == INT_MIN ? "no tile" : "a tile of another class");
}
// the calls that follow are tnml_site_conditionals' (1), tnml_nll_masked_grad / _step's (2) or the sampler's (0): which tile rule the
// environment launches are held to
void san_stub_site_cond_call(int on) { g_site_cond_call = on; }
// the normaliser rows (weight -2) of the masked_grad_kernel launches since the last call of this function
long san_stub_nmg_normalisers(void) { const long k = g_nmg_normalisers; g_nmg_normalisers = 0; return k; }
// the records of the last persistent launch as the "device" holds them (n steps; record n is the batch side's prologue)
const void *san_stub_last_persist(int *n_steps) { *n_steps = g_last_persist_n; return g_last_persist; }
}
