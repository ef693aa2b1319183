// report_common.h — what the device reports share (trace_take.hip, sample.hip, backlog.hip).
//
// A report is count -> scan -> scatter beside the round path: a count kernel leaves one number per
// item (a host, or a wave of 64 hosts), one workgroup scans them into offsets, a scatter kernel puts
// every row at its offset. The count and the scatter are the report's own; the scan, the wave
// reductions, the first-offender error word and the host scaffolding around the launches are here,
// once. (The events a context keeps between calls, ReportEvents, are in sgn_internal.h with sgn_ctx.)
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <type_traits>

#include "sgn_internal.h"

namespace sgn {
namespace report {

// ---- device side ----------------------------------------------------------------------------
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// the error word of a report's header: the first writer of a bit stores its offender
template <typename Info>
__device__ __forceinline__ void report_fail(uint32_t* err, Info* info, uint32_t bit, std::common_type_t<Info> what) {
  if ((atomicOr(err, bit) & bit) == 0) *info = what;
}

// over the 64 lanes of a wave, the result in every lane; every lane of the wave calls them
__device__ __forceinline__ uint64_t wave_sum(uint64_t s) {
#pragma unroll
  for (uint32_t x = 32; x > 0; x >>= 1) s += __shfl_xor(s, x);
  return s;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t s) {
#pragma unroll
  for (uint32_t x = 32; x > 0; x >>= 1) {
    const uint64_t v = __shfl_xor(s, x);
    s = v < s ? v : s;
  }
  return s;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t s) {
#pragma unroll
  for (uint32_t x = 1; x < 64; x <<= 1) {
    const uint64_t v = __shfl_xor(s, x);
    s = v > s ? v : s;
  }
  return s;
}
// (time, host) becomes the lesser of itself and (t, h): on equal times the lower HostId stays
__device__ __forceinline__ void argmin_fold(uint64_t& time, uint32_t& host, uint64_t t, uint32_t h) {
  if (t < time || (t == time && h < host)) {
    time = t;
    host = h;
  }
}
__device__ __forceinline__ void wave_argmin(uint64_t& time, uint32_t& host) {
#pragma unroll
  for (uint32_t x = 1; x < 64; x <<= 1) {
    const uint64_t t = __shfl_xor(time, x);
    const uint32_t h = __shfl_xor(host, x);
    argmin_fold(time, host, t, h);
  }
}
// a set lane's rank among the set lanes of a ballot
__device__ __forceinline__ uint32_t rank_below(uint64_t mask, uint32_t lane) { return (uint32_t)__popcll(mask & ((1ull << lane) - 1)); }

// The scan: ONE workgroup of kScanThreads walks n items in tiles of kScanTile (kScanPer consecutive
// items a thread) and carries the running total from tile to tile. load(j) gives item j,
// store(j, sum of the items before j, item j) takes its exclusive prefix; the total comes back in
// every thread. T needs operator+, a zero T{} and scan_shfl_up(T, d) (a pair shuffles its members
// one by one). n must be uniform over the workgroup, and every thread calls: there are two
// __syncthreads() inside the tile loop.
constexpr uint32_t kScanThreads = 256, kScanPer = 4;
constexpr uint32_t kScanTile = kScanThreads * kScanPer;

__device__ __forceinline__ uint32_t scan_shfl_up(uint32_t v, uint32_t d) { return __shfl_up(v, d); }

template <typename T, typename Load, typename Store>
__device__ __forceinline__ T tiled_scan(uint32_t n, Load load, Store store) {
  __shared__ T ws[kScanThreads / 64];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  T carry{};  // (the same in every thread)
  for (uint32_t t0 = 0; t0 < n; t0 += kScanTile) {
    const uint32_t j0 = t0 + threadIdx.x * kScanPer;
    T c[kScanPer];
    T tc{};
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; j++) {
      c[j] = j0 + j < n ? load(j0 + j) : T{};
      tc = tc + c[j];
    }
    T ic = tc;  // inclusive scan over the wave, then over the workgroup's waves
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const T v = scan_shfl_up(ic, d);
      if (lane >= d) ic = ic + v;
    }
    if (lane == 63) ws[w] = ic;
    const T below = scan_shfl_up(ic, 1);  // the lanes before this one
    __syncthreads();
    T e = carry, tot{};
#pragma unroll
    for (uint32_t v = 0; v < kScanThreads / 64; v++) {
      if (v < w) e = e + ws[v];
      tot = tot + ws[v];
    }
    if (lane) e = e + below;
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; j++) {
      if (j0 + j >= n) break;
      store(j0 + j, e, c[j]);
      e = e + c[j];
    }
    carry = carry + tot;
    __syncthreads();  // (the next tile writes ws)
  }
  return carry;
}

// ---- host side ------------------------------------------------------------------------------
inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the time between two recorded events; 0 where HIP has none
inline float elapsed_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

// a scratch buffer laid out piece by piece: take() gives the next piece's offset
struct ScratchLay {
  size_t bytes = 0;
  size_t take(size_t n, size_t align) {
    const size_t at = (bytes + align - 1) & ~(align - 1);
    bytes = at + n;
    return at;
  }
};

// the kernels launched so far, then their header on the host; the context's stream is idle on return
template <typename Hdr>
int read_header(sgn_ctx* ctx, const Hdr* d_hdr, Hdr* h) {
  SGN_HIP(ctx, hipGetLastError());
  SGN_HIP(ctx, hipMemcpyAsync(h, d_hdr, sizeof(Hdr), hipMemcpyDeviceToHost, ctx->stream));
  SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // namespace report
}  // namespace sgn
