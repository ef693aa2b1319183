// What does a waited-for scalar load cost against a constant-lane v_readlane_b32, at one wave
// per SIMD (the round kernel's occupancy: nothing hides a stall)?
//
//   hipcc --offload-arch=gfx950 -O2 tools/smem_latency_bench.hip -o tools/smem_latency_bench
//   tools/smem_latency_bench
//
// Every workgroup is one wave; the grid is one wave per SIMD (4 per CU). Each wave times, with
// s_memtime, (a) a chain of N scalar loads from a hot 1-KB buffer, each followed by s_waitcnt
// lgkmcnt(0) — the form the round kernel's DevSim reloads take — and (b) the same number of
// constant-lane v_readlane_b32 from a register that holds the same dwords, each result consumed
// by a scalar add. A first untimed pass of (a) makes the buffer hot in the scalar cache. Prints
// the median and the fastest wave's cycles per operation for both, and the s_memtime overhead
// (an empty timed section) that is already subtracted.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                  \
      return 1;                                                                \
    }                                                                          \
  } while (0)

constexpr int N = 64;  // operations per chain (one per 16 bytes of the 1-KB buffer)

__device__ __forceinline__ uint64_t now() {
  uint64_t t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

template <int K>
__device__ __forceinline__ void sload_chain(const uint32_t* buf, uint32_t& acc) {
  if constexpr (K < N) {
    uint32_t v;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(buf), "n"(K * 16) : "memory");
    acc += v;
    sload_chain<K + 1>(buf, acc);
  }
}
template <int K>
__device__ __forceinline__ void readlane_chain(uint32_t reg, uint32_t& acc) {
  if constexpr (K < N) {
    uint32_t v;
    asm volatile("v_readlane_b32 %0, %1, %2" : "=s"(v) : "v"(reg), "n"(K));
    acc += v;
    readlane_chain<K + 1>(reg, acc);
  }
}

// out[3 * wave + {0, 1, 2}] = cycles of the empty section, the load chain, the readlane chain
__global__ __launch_bounds__(64) void k_bench(const uint32_t* __restrict__ buf, uint64_t* out, uint32_t* sink) {
  uint32_t acc = 0;
  sload_chain<0>(buf, acc);  // warm the scalar cache (and the instruction cache's first lines)
  uint32_t reg = buf[4 * (threadIdx.x & 63)];  // lane k: the dword chain (a) reads at step k
  asm volatile("" : "+v"(reg));
  const uint64_t e0 = now();
  const uint64_t e1 = now();
  const uint64_t a0 = now();
  sload_chain<0>(buf, acc);
  const uint64_t a1 = now();
  uint32_t acc2 = 0;
  const uint64_t b0 = now();
  readlane_chain<0>(reg, acc2);
  asm volatile("" ::"s"(acc2));
  const uint64_t b1 = now();
  if (threadIdx.x == 0) {
    out[3 * blockIdx.x + 0] = e1 - e0;
    out[3 * blockIdx.x + 1] = a1 - a0;
    out[3 * blockIdx.x + 2] = b1 - b0;
    // both chains read the same dwords: the sums agree (the first pass counted twice)
    sink[blockIdx.x] = acc - 2 * acc2;
  }
}

int main() {
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, 0));
  const int waves = p.multiProcessorCount * 4;
  uint32_t* buf;
  uint64_t* out;
  uint32_t* sink;
  CK(hipMalloc(&buf, 1024));
  CK(hipMalloc(&out, sizeof(uint64_t) * 3 * waves));
  CK(hipMalloc(&sink, sizeof(uint32_t) * waves));
  std::vector<uint32_t> h(256);
  for (int i = 0; i < 256; i++) h[i] = 2654435761u * (uint32_t)(i + 1);
  CK(hipMemcpy(buf, h.data(), 1024, hipMemcpyHostToDevice));
  for (int rep = 0; rep < 3; rep++) {  // (the last repetition is reported)
    hipLaunchKernelGGL(k_bench, dim3(waves), dim3(64), 0, 0, buf, out, sink);
    CK(hipDeviceSynchronize());
  }
  std::vector<uint64_t> o(3 * (size_t)waves);
  std::vector<uint32_t> s(waves);
  CK(hipMemcpy(o.data(), out, sizeof(uint64_t) * o.size(), hipMemcpyDeviceToHost));
  CK(hipMemcpy(s.data(), sink, sizeof(uint32_t) * s.size(), hipMemcpyDeviceToHost));
  int bad = 0;
  for (int w = 0; w < waves; w++) bad += s[w] != 0;
  std::vector<double> e(waves), a(waves), b(waves);
  for (int w = 0; w < waves; w++) {
    e[w] = (double)o[3 * w];
    a[w] = ((double)o[3 * w + 1] - e[w]) / N;
    b[w] = ((double)o[3 * w + 2] - e[w]) / N;
  }
  auto med = [](std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
  };
  auto mn = [](const std::vector<double>& v) { return *std::min_element(v.begin(), v.end()); };
  printf("{\"device\": \"%s\", \"waves\": %d, \"ops_per_chain\": %d, \"timer_overhead_cycles_median\": %.1f, "
         "\"sload_waited_cycles_per_op\": {\"median\": %.1f, \"min\": %.1f}, "
         "\"readlane_cycles_per_op\": {\"median\": %.1f, \"min\": %.1f}, \"sum_mismatches\": %d}\n",
         p.name, waves, N, med(e), med(a), mn(a), med(b), mn(b), bad);
  CK(hipFree(buf));
  CK(hipFree(out));
  CK(hipFree(sink));
  return bad != 0;
}
