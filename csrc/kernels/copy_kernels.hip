// Byte-copy and multi-source gather kernels of the communication engine
// (device_copy_kernel / device_gather_kernel, declared in device/device.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../device/device.hpp"

namespace parsec {

// Device-to-device byte copy as a kernel (16-byte vectors, grid-stride): used for
// pulls from peer-process (IPC) allocations so the copy is an ordinary kernel in
// stream order on this process's queue.
__global__ __launch_bounds__(256) void copy_bytes_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
__global__ void copy_tail_kernel(char* __restrict__ dst, const char* __restrict__ src, size_t n) {
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

int device_copy_kernel(void* dst, const void* src, size_t bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const bool aligned = ((uintptr_t)dst % 16 == 0) && ((uintptr_t)src % 16 == 0);
  size_t n16 = aligned ? bytes / 16 : 0;
  if (n16) {
    const unsigned blocks = (unsigned)std::min<size_t>(1024, (n16 + 255) / 256);
    hipLaunchKernelGGL(copy_bytes_kernel, dim3(blocks), dim3(256), 0, s, static_cast<uint4*>(dst), static_cast<const uint4*>(src), n16);
  }
  const size_t done = n16 * 16;
  if (bytes > done) hipLaunchKernelGGL(copy_tail_kernel, dim3(1), dim3(256), 0, s, static_cast<char*>(dst) + done, static_cast<const char*>(src) + done, bytes - done);
  return (int)hipGetLastError();
}

// Multi-source gather: ONE launch moves up to kMaxGather transfers, each from
// another peer's IPC mapping. Across xGMI every peer GPU sits behind its own
// link, so the transfers of one launch pull over up to 7 links at once while
// the process keeps one copy stream (one hardware queue). Workgroups are split
// between the transfers in proportion to their size (at most 64 per transfer,
// 4 x 16-byte loads in flight per thread: ~1 MiB in flight per link).
constexpr int kMaxGather = 16;
struct GatherArgs {
  int count;
  int wg_start[kMaxGather + 1];
  uint4* dst[kMaxGather];
  const uint4* src[kMaxGather];
  unsigned long long n16[kMaxGather];
};
static_assert(sizeof(GatherArgs) <= 4096, "GatherArgs exceeds the kernel argument limit");
__global__ __launch_bounds__(256) void gather_kernel(const GatherArgs a) {
  int t = 0;
  while (t + 1 < a.count && (int)blockIdx.x >= a.wg_start[t + 1]) ++t;
  const int w = (int)blockIdx.x - a.wg_start[t], nw = a.wg_start[t + 1] - a.wg_start[t];
  uint4* __restrict__ d = a.dst[t];
  const uint4* __restrict__ s = a.src[t];
  const size_t n = a.n16[t], stride = (size_t)nw * 256;
  size_t i = (size_t)w * 256 + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    const uint4 v0 = s[i], v1 = s[i + stride], v2 = s[i + 2 * stride], v3 = s[i + 3 * stride];
    d[i] = v0;
    d[i + stride] = v1;
    d[i + 2 * stride] = v2;
    d[i + 3 * stride] = v3;
  }
  for (; i < n; i += stride) d[i] = s[i];
}

int device_gather_kernel(void* const* dst, const void* const* src, const size_t* bytes, int n, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n;) {
    GatherArgs a{};
    int wg = 0;
    for (; i < n && a.count < kMaxGather; ++i) {
      const bool aligned = ((uintptr_t)dst[i] % 16 == 0) && ((uintptr_t)src[i] % 16 == 0) && bytes[i] % 16 == 0;
      if (!aligned || bytes[i] == 0) {  // odd sizes / offsets: a copy kernel of its own, same stream
        if (bytes[i] && device_copy_kernel(dst[i], src[i], bytes[i], stream) != 0) return -1;
        continue;
      }
      const int k = a.count++;
      a.dst[k] = static_cast<uint4*>(dst[i]);
      a.src[k] = static_cast<const uint4*>(src[i]);
      a.n16[k] = bytes[i] / 16;
      a.wg_start[k] = wg;
      wg += (int)std::min<size_t>(64, std::max<size_t>(1, a.n16[k] / (256 * 16)));
    }
    if (!a.count) continue;
    a.wg_start[a.count] = wg;
    hipLaunchKernelGGL(gather_kernel, dim3(wg), dim3(256), 0, st, a);
  }
  return (int)hipGetLastError();
}

}  // namespace parsec
