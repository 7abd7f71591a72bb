// Host state of the tile Cholesky's panel solve: the mode / limit of
// PARSEC_DPOTRF_TRSM (trsm_inverse_mode) and the table of condition estimates
// that tile POTRFs publish to pinned host memory. No kernel is launched here;
// the HIP runtime is used for the pinned and device slots only.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "kernels.hpp"

namespace parsec {
namespace kern {

// ---------------------------------------------- host-published panel estimates
// Under PARSEC_DPOTRF_TRSM=auto the tile POTRF that writes W = L^-1 publishes
// max|L| max|W| into pinned host memory when its last step launch retires. The
// engine dispatches TRSM(m, k) only after POTRF(k)'s completion event, so the
// TRSM launch reads the estimate on the host and launches the substitution
// kernel only for the panels above the limit: no gated kernel rides the
// critical stream behind every panel GEMM. A W whose estimate is unknown here
// (factored by another process, or not yet published) takes the device-side
// gate (scan in the copy kernel, in-place gated substitution kernel).
namespace {
constexpr uint32_t kEstSlots = 4096;
struct EstimateSlots {
  std::mutex m;
  bool tried = false;
  double* host = nullptr;              // [kEstSlots], pinned; 0 = not published
  unsigned long long* dev = nullptr;   // [kEstSlots][4]: max|L|, max|W|, arrivals, pad
  const double* owner[kEstSlots] = {};
  uint32_t next = 0;
  std::unordered_map<const double*, uint32_t> of_w;
};
EstimateSlots g_est[16];
std::atomic<bool> g_est_any{false};  // some device has estimate slots (forget() is a no-op before)
int g_est_route = -1;  // PARSEC_DPOTRF_TRSM_ESTIMATE: 1 = host-published (default), 0 = device gate only
EstimateSlots* est_slots() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  return &g_est[dev];
}
}  // namespace

int trsm_estimate_route(int on) {
  if (g_est_route < 0) {
    const char* e = getenv("PARSEC_DPOTRF_TRSM_ESTIMATE");
    g_est_route = e ? (atoi(e) != 0) : 1;
  }
  const int prev = g_est_route;
  if (on >= 0) g_est_route = on != 0;
  return prev;
}

// A slot for the POTRF writing W (device / host halves), or false.
bool trsm_estimate_acquire(const double* W, unsigned long long** dev, double** host) {
  if (trsm_estimate_route(-1) == 0 || parsec::trsm_inverse_mode(-1, 0.0) != 1) return false;
  EstimateSlots* e = est_slots();
  if (!e) return false;
  std::lock_guard<std::mutex> lk(e->m);
  if (!e->tried) {
    e->tried = true;
    void* h = nullptr;
    void* d = nullptr;
    if (hipHostMalloc(&h, kEstSlots * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); h = nullptr; }
    if (h && hipMalloc(&d, kEstSlots * 4 * sizeof(unsigned long long)) != hipSuccess) { (void)hipGetLastError(); d = nullptr; }
    if (h && d && hipMemset(d, 0, kEstSlots * 4 * sizeof(unsigned long long)) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
      std::memset(h, 0, kEstSlots * sizeof(double));
      e->host = static_cast<double*>(h);
      e->dev = static_cast<unsigned long long*>(d);
      g_est_any.store(true, std::memory_order_release);
    } else {
      (void)hipGetLastError();
      if (h) (void)hipHostFree(h);
      if (d) (void)hipFree(d);
    }
  }
  if (!e->host) return false;
  const uint32_t slot = e->next++ % kEstSlots;
  if (e->owner[slot]) {
    auto it = e->of_w.find(e->owner[slot]);
    if (it != e->of_w.end() && it->second == slot) e->of_w.erase(it);
  }
  e->owner[slot] = W;
  e->of_w[W] = slot;
  *reinterpret_cast<volatile double*>(&e->host[slot]) = 0.0;
  *dev = e->dev + (size_t)slot * 4;
  *host = e->host + slot;
  return true;
}

// A device buffer was (re)allocated: whatever W it held is gone, so an estimate
// keyed by its address must not be found for the next tile living there (a
// receive buffer recycled from the pool or the zone, a tile re-staged after
// eviction). Called by the zone allocator, device_alloc and the comm engine's
// receive-buffer pool.
void trsm_estimate_forget(const void* p) {
  if (!p || !g_est_any.load(std::memory_order_acquire)) return;
  for (EstimateSlots& e : g_est) {
    std::lock_guard<std::mutex> lk(e.m);
    if (!e.host) continue;
    auto it = e.of_w.find(static_cast<const double*>(p));
    if (it == e.of_w.end()) continue;
    if (e.owner[it->second] == p) e.owner[it->second] = nullptr;
    e.of_w.erase(it);
  }
}

// The published estimate of the POTRF that wrote W (> 0), or 0 when unknown.
double trsm_estimate_lookup(const void* p) {
  const double* W = static_cast<const double*>(p);
  if (trsm_estimate_route(-1) == 0) return 0.0;
  EstimateSlots* e = est_slots();
  if (!e || !e->host) return 0.0;
  std::lock_guard<std::mutex> lk(e->m);
  auto it = e->of_w.find(W);
  if (it == e->of_w.end() || e->owner[it->second] != W) return 0.0;
  const double v = *reinterpret_cast<volatile const double*>(&e->host[it->second]);
  std::atomic_thread_fence(std::memory_order_acquire);
  return v;
}

// tests: every W address holding a published estimate on the current device
std::vector<uintptr_t> trsm_estimate_known() {
  std::vector<uintptr_t> out;
  EstimateSlots* e = est_slots();
  if (!e) return out;
  std::lock_guard<std::mutex> lk(e->m);
  if (!e->host) return out;
  for (const auto& kv : e->of_w)
    if (e->owner[kv.second] == kv.first && *reinterpret_cast<volatile const double*>(&e->host[kv.second]) > 0.0) out.push_back((uintptr_t)kv.first);
  return out;
}

// Estimates published / taken on the host / left to the device gate (tests, bench)
static std::atomic<uint64_t> g_est_stats[3];
void trsm_estimate_count(int which) { g_est_stats[which].fetch_add(1, std::memory_order_relaxed); }

// counters: [0] estimates published by POTRF, [1] panel decisions taken on the
// host, [2] panels left to the device gate
void trsm_estimate_stats(uint64_t out[3], bool reset) {
  for (int i = 0; i < 3; ++i) out[i] = reset ? g_est_stats[i].exchange(0) : g_est_stats[i].load();
}

}  // namespace kern

// Panel-solve mode of the tile Cholesky (kernels.hpp trsm_inverse_mode).
// PARSEC_DPOTRF_TRSM = inverse | auto | blocked, PARSEC_DPOTRF_TRSM_LIMIT = the
// estimate above which auto solves by substitution (scripts/trsm_inverse_numerics.py,
// profiles/r4_trsm_inverse_numerics.txt).
static std::atomic<int> g_trsm_mode{-1};
static std::atomic<double> g_trsm_limit{0.0};
static void trsm_mode_init() {
  static std::once_flag once;
  std::call_once(once, [] {
    int m = 1;
    if (const char* e = getenv("PARSEC_DPOTRF_TRSM")) m = !strcmp(e, "inverse") ? 0 : !strcmp(e, "blocked") ? 2 : 1;
    double lim = 1e6;
    if (const char* e = getenv("PARSEC_DPOTRF_TRSM_LIMIT")) lim = atof(e);
    int exp = -1;
    g_trsm_mode.compare_exchange_strong(exp, m);
    double z = 0.0;
    g_trsm_limit.compare_exchange_strong(z, lim > 0 ? lim : 1e6);
  });
}
int trsm_inverse_mode(int mode, double limit) {
  trsm_mode_init();
  const int prev = g_trsm_mode.load();
  if (mode >= 0) g_trsm_mode.store(mode);
  if (limit > 0) g_trsm_limit.store(limit);
  return prev;
}
double trsm_inverse_limit() {
  trsm_mode_init();
  return g_trsm_limit.load(std::memory_order_relaxed);
}

}  // namespace parsec
