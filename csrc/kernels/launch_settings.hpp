// Launch settings of the calling thread, internal to the kernel layer: what
// every launcher of csrc/kernels passes to the kernels it issues right now.
// launch_kernel_batch sets them for the batch it flushes; a thread that never
// entered a scope launches with all four zero.
#pragma once

namespace parsec {
namespace kern {

struct LaunchSettings {
  // critical stream's batch: raise the waves' issue priority (s_setprio). A
  // critical kernel sharing a CU with bulk GEMM waves otherwise gets a third of
  // the SIMD's MFMA pipe and waits behind their instructions (the SIMD
  // arbitrates by priority, then age).
  int prio = 0;
  // extra dynamic LDS of a 128x128 GEMM launch: kBulkPadBytes pads a workgroup
  // to 82 KB, so a CU holds ONE bulk GEMM workgroup and keeps room for a
  // critical-path tile-POTRF step workgroup (78 KB)
  int pad = 0;
  int claim = 0;  // critical-path launch: its workgroups claim their CUs (1: tile-POTRF steps, 2: every kernel)
  int yield = 0;  // bulk launch: its GEMM waves yield claimed CUs
};

LaunchSettings& launch_settings();  // thread-local

// Replaces the thread's settings for a scope and puts the previous ones back.
struct LaunchScope {
  LaunchSettings prev;
  explicit LaunchScope(const LaunchSettings& s) : prev(launch_settings()) { launch_settings() = s; }
  ~LaunchScope() { launch_settings() = prev; }
  LaunchScope(const LaunchScope&) = delete;
  LaunchScope& operator=(const LaunchScope&) = delete;
};

}  // namespace kern
}  // namespace parsec
