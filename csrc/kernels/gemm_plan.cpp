// Host side of the grouped DGEMM: the dispatch policy (environment knobs and
// their setters), the launch plan -- which kernel, tile shape and grid
// launch_gemm_batch (tile_kernels.hip) issues for a descriptor list -- the
// chunk plan and the per-thread launch log. Plain C++: no kernel is launched, no
// device is asked and no descriptor pointer is dereferenced here.
#include <algorithm>
#include <cstdlib>

#include "kernels.hpp"

namespace parsec {
namespace kern {

static GemmPolicy gemm_policy_init() {
  GemmPolicy p;
  auto num = [](const char* name, int& v) {
    if (const char* e = getenv(name)) v = atoi(e);
  };
  num("PARSEC_GEMM_TILE", p.tile);
  num("PARSEC_GEMM_FULL", p.full);
  num("PARSEC_GEMM_BIG_TILES", p.big_tiles);
  num("PARSEC_GEMM_SPLITK", p.splitk);
  num("PARSEC_GEMM_MAINLOOP", p.mainloop);
  num("PARSEC_GEMM_PIPELINE", p.pipeline);
  num("PARSEC_GEMM_CHUNK_FILL", p.chunk_fill);
  num("PARSEC_GEMM_SLOTS", p.slots);
  num("PARSEC_GEMM_EPI", p.epi);
  p.mainloop = p.mainloop != 0;
  p.pipeline = p.pipeline != 0;
  if (getenv("PARSEC_GEMM_SLOTS")) p.slots = std::max(1, p.slots);
  if (p.epi != 0 && p.epi != 1) p.epi = -1;
  int pad_test = 0;
  num("PARSEC_GEMM_PAD_TEST", pad_test);
  p.pad_test = pad_test != 0;
  p.pad_debug = getenv("PARSEC_GEMM_PAD_DEBUG") != nullptr;
  return p;
}
GemmPolicy& gemm_policy() {
  static GemmPolicy p = gemm_policy_init();
  return p;
}
// The pinned body addresses an operand as a uniform base plus a 32-bit
// per-thread byte offset that spans the columns of the stored operand a k-tile
// touches: BK of A (BM when A is transposed), BN of B (BK when B is transposed).
int gemm_pipeline_fits(int bm, int bn, int bk, int transA, int transB, long long lda, long long ldb) {
  const unsigned long long span_a = (unsigned long long)(transA ? bm : bk) * (unsigned long long)lda * sizeof(double);
  const unsigned long long span_b = (unsigned long long)(transB ? bk : bn) * (unsigned long long)ldb * sizeof(double);
  // strictly below 2^32: the buffer resource of the loads covers 2^32 - 1 bytes
  return span_a < (1ull << 32) && span_b < (1ull << 32);
}

// launch record of this thread (gemm_launch_log): a ring of the last launches
static thread_local bool t_gemm_log_on = false;
static thread_local GemmLaunchRecord t_gemm_log[kGemmLaunchLogSize];
static thread_local unsigned t_gemm_log_count = 0;  // records written since the last reset

// ---- Decide. What launch_gemm_batch issues for a descriptor list is computed
// here on the host alone, from the descriptors and an explicit environment; no
// pointer is dereferenced and no device is asked.
// Descriptors per launch (<= kMaxGemmBatch, the kernel-argument limit): the cut
// that fills whole rounds of resident 128x128 workgroups best. 40 tiles of
// 512^2 are 640 128-tiles = 1.25 rounds of 512 slots (62 % of the second round
// idle); 32 of them are exactly one round.
template <class Tiles128>  // tiles128(i): 128 x 128 tiles of descriptor i
static int gemm_chunk_cut(Tiles128 tiles128, int n, int slots, bool fill_rounds) {
  const int cap = std::min(n, kMaxGemmBatch);
  if (!fill_rounds) return cap;
  int best = cap, tiles = 0;
  double best_fill = -1.0;
  for (int c = 1; c <= cap; ++c) {
    tiles += tiles128(c - 1);
    if (tiles < slots) continue;
    const int rounds = (tiles + slots - 1) / slots;
    const double fill = (double)tiles / ((double)rounds * slots);
    if (fill >= best_fill - 1e-9) { best_fill = fill; best = c; }  // ties: the larger cut
  }
  return best_fill >= 0.0 ? best : cap;
}
int gemm_chunk_plan(const int* m, const int* n, int count, int slots, int* out) {
  int cuts = 0;
  for (int s = 0; s < count;) {
    const int c = gemm_chunk_cut([&](int i) { return ((m[s + i] + 127) / 128) * ((n[s + i] + 127) / 128); }, count - s, std::max(1, slots),
                                 gemm_policy().chunk_fill != 0);
    out[cuts++] = c;
    s += c;
  }
  return cuts;
}

// One launch of n descriptors of one operand mode: tile shape, kernel, grid.
static GemmLaunchRecord gemm_plan_launch(const GemmDesc* descs, int n, const GemmPlanEnv& env) {
  const GemmPolicy& p = env.policy;
  GemmLaunchRecord r{};
  int t128 = 0;
  bool big = true;
  for (int i = 0; i < n; ++i) {
    t128 += ((descs[i].m + 127) / 128) * ((descs[i].n + 127) / 128);
    if (descs[i].m < 128 || descs[i].n < 128) big = false;
  }
  // 128x128: 8 waves (2 x 4) of 64x32, 126 VGPRs -> 4 waves per SIMD with two
  // workgroups per CU (profiles/r1_gemm_variants_v8.log); 64x64: 4 waves of 32x32
  const bool use_big = p.tile == 128 || (p.tile == 0 && big && t128 >= p.big_tiles);
  const int BM = use_big ? 128 : 64, BN = BM, BK = 16;
  r.bm = BM; r.bn = BN;
  r.descs = n;
  r.transA = descs[0].transA != 0; r.transB = descs[0].transB != 0;
  r.pad_bytes = use_big ? env.pad_bytes : 0;
  int total = 0;
  bool full = p.full != 0;
  for (int i = 0; i < n; ++i) {
    const GemmDesc& g = descs[i];
    full = full && g.m % BM == 0 && g.n % BN == 0 && g.k > 0 && g.k % BK == 0 && (g.lda | g.ldb) % 2 == 0 &&
           ((uintptr_t)g.A | (uintptr_t)g.B) % 16 == 0;
    total += ((g.m + BM - 1) / BM) * ((g.n + BN - 1) / BN);
  }
  r.total_tiles = r.main_tiles = r.grid = total;
  r.ksplit = 1;
  const int slots = env.slots;
  if (use_big && p.splitk != 0 && total > slots) {
    // the last partial round of workgroups: split its tiles' K range so it
    // finishes in 1/s of a tile time; needs beta == 1 (partials are added into C)
    // and >= 256 of K per chunk (fewer flops per added byte would be bound by
    // the chip's f64 atomic rate)
    const int tail = total % slots;
    int kmin = 1 << 30;
    bool ok = tail > 0 && 2 * tail <= slots;
    for (int i = 0; ok && i < n; ++i) {
      ok = descs[i].beta == 1.0 && !descs[i].a_lower && !descs[i].b_upper && !descs[i].Cin && !descs[i].C2;
      kmin = std::min(kmin, descs[i].k);
    }
    const int s = ok ? std::min({slots / std::max(tail, 1), kmin / 256, 8}) : 1;
    if (s >= 2) {
      r.main_tiles = total - tail;
      r.ksplit = s;
      r.grid = r.main_tiles + tail * s;
    }
  }
  // atomic epilogue: every descriptor accumulates into C (beta 1, no separate Cin / C2)
  bool epi = p.epi != 0 && full;
  for (int i = 0; epi && i < n; ++i) epi = descs[i].beta == 1.0 && !descs[i].Cin && !descs[i].C2 && (p.epi > 0 || descs[i].k >= 1024);
  // rotated k loop (gemm_tile ML = 1) for the full launches
  const bool rot = full && p.mainloop == 1;
  // its pinned body (ML = 2): no yield poll or CU claim, 32-bit per-thread operand offsets
  bool pipe = rot && p.pipeline == 1 && !env.yield && !env.claim;
  for (int i = 0; pipe && i < n; ++i) pipe = gemm_pipeline_fits(BM, BN, BK, descs[i].transA, descs[i].transB, descs[i].lda, descs[i].ldb) != 0;
  r.full = full; r.epilogue = epi ? 1 : 0;
  r.rotated = rot; r.pipelined = pipe;
  return r;
}

// Group descriptors by (transA, transB): one grouped launch per combination
// (the vendor library is an A/B reference only: scripts/kbench_gemm_vs_vendor.py).
// A descriptor with alpha == 0 or k <= 0 references neither A nor B (BLAS): it
// goes out as K = 0 in a launch of its own kind, C := beta C from the
// bounds-checked kernel's epilogue, so NaN / Inf in the operands stay out of C
// and the k loops carry no test for it. (Gated descriptors are a protocol of
// the panel solve and stay where they are.) `sorted` receives the descriptors
// in launch order; a chunk without tiles launches nothing and has no record.
std::vector<GemmLaunch> gemm_plan(const GemmDesc* descs, int n, const GemmPlanEnv& env, std::vector<GemmDesc>& sorted) {
  std::vector<GemmDesc> g[5];
  for (int i = 0; i < n; ++i) {
    const GemmDesc& d = descs[i];
    if ((d.alpha == 0.0 || d.k <= 0) && !d.gate) {
      GemmDesc z = d;
      z.k = 0;
      z.transA = z.transB = 0;
      z.a_lower = z.b_upper = 0;
      g[4].push_back(z);
    } else {
      g[(d.transA ? 2 : 0) | (d.transB ? 1 : 0)].push_back(d);
    }
  }
  std::vector<GemmLaunch> plan;
  sorted.clear();
  for (const auto& v : g) {
    for (size_t s = 0; s < v.size();) {
      const GemmDesc* d = v.data() + s;
      const int c = gemm_chunk_cut([d](int i) { return ((d[i].m + 127) / 128) * ((d[i].n + 127) / 128); }, (int)(v.size() - s), env.slots,
                                   env.policy.chunk_fill != 0);
      const GemmLaunchRecord r = gemm_plan_launch(d, c, env);
      if (r.total_tiles > 0) plan.push_back({r, (int)sorted.size()});
      sorted.insert(sorted.end(), d, d + c);
      s += (size_t)c;
    }
  }
  return plan;
}
int gemm_launch_plan(const GemmDesc* descs, int n, int slots, bool one_per_cu, bool bulk_yield, int claim, GemmLaunchRecord* out) {
  std::vector<GemmDesc> sorted;
  const GemmPlanEnv env{gemm_policy(), std::max(1, one_per_cu ? slots / 2 : slots), one_per_cu ? kBulkPadBytes : 0, bulk_yield, claim >= 2};
  const std::vector<GemmLaunch> plan = gemm_plan(descs, n, env, sorted);
  for (size_t i = 0; i < plan.size(); ++i) out[i] = plan[i].rec;
  return (int)plan.size();
}

// Split-K tail of the 128x128 kernel on (1) / off (0), < 0 queries; returns the previous setting.
int gemm_splitk(int on) {
  const int prev = gemm_policy().splitk;
  if (on >= 0) gemm_policy().splitk = on;
  return prev;
}

// k loop of the full register-staged GEMM launches: 0 plain, 1 rotated, < 0 queries; returns the previous setting.
int gemm_mainloop(int mode) {
  const int prev = gemm_policy().mainloop;
  if (mode >= 0) gemm_policy().mainloop = mode == 0 ? 0 : 1;
  return prev;
}

// Body of the rotated k loop (consulted only when gemm_mainloop is 1): 0 compiler-scheduled, 1 pinned, < 0 queries; returns the previous setting.
int gemm_pipeline(int mode) {
  const int prev = gemm_policy().pipeline;
  if (mode >= 0) gemm_policy().pipeline = mode == 0 ? 0 : 1;
  return prev;
}

// Round-filling launch chunks on (1) / off (0), < 0 queries; returns the previous setting.
int gemm_chunk_fill(int on) {
  const int prev = gemm_policy().chunk_fill;
  if (on >= 0) gemm_policy().chunk_fill = on != 0;
  return prev;
}

void gemm_launch_log_append(const GemmLaunchRecord& r) {
  if (t_gemm_log_on) t_gemm_log[t_gemm_log_count++ % kGemmLaunchLogSize] = r;
}

int gemm_launch_log(int on) {
  const int prev = t_gemm_log_on;
  if (on >= 0) t_gemm_log_on = on != 0;
  return prev;
}

int gemm_launch_log_read(GemmLaunchRecord* out, bool reset) {
  const unsigned have = std::min<unsigned>(t_gemm_log_count, kGemmLaunchLogSize);
  for (unsigned i = 0; i < have; ++i) out[i] = t_gemm_log[(t_gemm_log_count - have + i) % kGemmLaunchLogSize];
  if (reset) t_gemm_log_count = 0;
  return (int)have;
}

// Tile-size policy of the grouped GEMM (0 = auto, 64, 128); returns the previous one.
int gemm_tile_policy(int p) {
  const int prev = gemm_policy().tile;
  if (p >= 0) gemm_policy().tile = p;
  return prev;
}

}  // namespace kern
}  // namespace parsec
