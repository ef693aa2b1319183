// drain_take.hip — the drain records taken out ordered, with per-host spans (sgn_drain_pending,
// sgn_drain_take, sgn_selftest_drain_order).
//
// The round kernels append drain records wherever their atomic counter puts them, and an earlier
// sgn_drain may have left records held on the host. A take hands the caller ALL of them, ordered by
// sgn_drain's key (host, time, src_host, src_eid, tag, status), one span per host with records, all
// or nothing. Unlike a trace record a drain record carries no per-host counter, so this report ends
// in a comparison sort of every host's segment:
//   1. k_dt_count    one pass over both inputs (the device buffer, the uploaded held records): per
//                    owned host the record count (atomics on a dense array);
//   2. k_dt_scan     an exclusive scan of the counts over the hosts (tiled_scan): each host's offset,
//                    the spans, the lists of the segments too large for a wave (one list per class),
//                    the largest segment; the host applies the capacity rule on the header;
//   3. k_dt_scatter  every record to its host's segment of buffer X, at off[h] + an atomic cursor:
//                    the segments are complete and unordered inside;
//   4. the order     X -> Y, shaped by the segment size:
//        k_dt_order_wave   a segment of at most kWaveMax records: one wave, a record a lane, the rank
//                          of a lane's key among the wave's (m broadcasts), one permuted store;
//        k_dt_order_tile   a tile of at most kTile records (a whole segment, or a piece of a larger
//                          one): one workgroup, keys and record indices in LDS, a bitonic network on
//                          the indices, one permuted write of the records;
//        k_dt_merge        the larger segments: sorted runs of w records merged pairwise (merge path:
//                          a thread finds its kMergePer outputs' diagonal by bisection and merges
//                          them serially), Y -> X -> Y ..., w doubling from kTile. The pass count is
//                          made even (a pass whose w covers the segment copies it), so the result is
//                          in Y whatever the segment sizes.
// then one device-to-host copy of Y. No record moves inside a buffer: every kernel reads one buffer
// and writes the other, so no lane reads what another wrote in the same launch.
//
// A sgn_drain_rec is 48 bytes, three 16-byte pieces: {time, src_eid}, {handle, host | src_host << 32},
// {dst_host | status << 32, payload_len | tag << 32}; in a 16-byte aligned buffer every piece is one
// aligned 16-byte load or store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "report_common.h"
#include "sgn_workload.h"

using namespace sgn;
using namespace sgn::report;

// ---- device side ----------------------------------------------------------------------------
namespace {

constexpr uint32_t kDtThreads = 256;     // every kernel here
constexpr uint32_t kDtMaxBlocks = 2048;  // count, scatter: grid-stride above that
constexpr uint32_t kWaveMax = 64;        // records a wave orders at once
// records a workgroup orders at once: 32 bytes of LDS a record (28 of key, 4 of index), 32 KiB a
// workgroup — five such workgroups fit a CU's 160 KiB
constexpr uint32_t kTile = 1024;
constexpr uint32_t kMergePer = 8;  // outputs a thread of k_dt_merge produces
constexpr uint32_t kRecPieces = 3;
static_assert(kTile % kMergePer == 0 && (kTile & (kTile - 1)) == 0, "a thread's outputs lie in one pair of runs");
static_assert(sizeof(sgn_drain_rec) == 48, "a record is three 16-byte pieces");
static_assert(offsetof(sgn_drain_rec, time) == 0 && offsetof(sgn_drain_rec, src_eid) == 8, "piece 0");
static_assert(offsetof(sgn_drain_rec, handle) == 16 && offsetof(sgn_drain_rec, host) == 24 &&
                  offsetof(sgn_drain_rec, src_host) == 28, "piece 1");
static_assert(offsetof(sgn_drain_rec, dst_host) == 32 && offsetof(sgn_drain_rec, status) == 36 &&
                  offsetof(sgn_drain_rec, payload_len) == 40 && offsetof(sgn_drain_rec, tag) == 44, "piece 2");
static_assert(sizeof(sgn_trace_span) == 24, "");

enum : uint32_t {
  DT_EHOST = 1u,   // a record of a host this shard does not own
  DT_ERANGE = 2u,  // the scatter met a record outside its host's segment (skipped)
  DT_ESPAN = 4u,   // a span outside the record buffers (its segment was not ordered)
};
struct __attribute__((aligned(16))) DtHdr {
  uint64_t total, n_spans;  // k_dt_scan: records counted, hosts with records
  uint32_t err, err_host;   // DT_E*, and the first offender (HostId)
  uint32_t n_mid, n_big;    // k_dt_scan: segments of (kWaveMax, kTile] records, of more
  unsigned long long largest;  // ... the largest segment
  uint64_t pad[3];
};
static_assert(sizeof(DtHdr) == 64, "");

struct Rec {
  u64x2 q0, q1, q2;
};
// sgn_drain's key inside one host: (time, src_host, src_eid, tag, status), every field in full width
struct Key {
  uint64_t time, eid;
  uint32_t src, tag, st;
};
__device__ __forceinline__ Rec rec_load(const u64x2* __restrict__ b, uint64_t i) {
  const u64x2* p = b + i * kRecPieces;
  return Rec{p[0], p[1], p[2]};
}
__device__ __forceinline__ void rec_store(u64x2* __restrict__ b, uint64_t i, const Rec& r) {
  u64x2* p = b + i * kRecPieces;
  p[0] = r.q0;
  p[1] = r.q1;
  p[2] = r.q2;
}
__device__ __forceinline__ uint32_t rec_host(const Rec& r) { return (uint32_t)r.q1.y; }
__device__ __forceinline__ Key rec_key(const Rec& r) {
  return Key{r.q0.x, r.q0.y, (uint32_t)(r.q1.y >> 32), (uint32_t)(r.q2.y >> 32), (uint32_t)(r.q2.x >> 32)};
}
__device__ __forceinline__ bool key_less(const Key& a, const Key& b) {
  if (a.time != b.time) return a.time < b.time;
  if (a.src != b.src) return a.src < b.src;
  if (a.eid != b.eid) return a.eid < b.eid;
  if (a.tag != b.tag) return a.tag < b.tag;
  return a.st < b.st;
}
__device__ __forceinline__ bool key_equal(const Key& a, const Key& b) {
  return a.time == b.time && a.src == b.src && a.eid == b.eid && a.tag == b.tag && a.st == b.st;
}

// record i of the two inputs laid end to end: a[0 .. na), then b[0 .. nb)
__device__ __forceinline__ Rec input_load(const u64x2* __restrict__ a, uint64_t na, const u64x2* __restrict__ b, uint64_t i) {
  return i < na ? rec_load(a, i) : rec_load(b, i - na);
}

// 1. per owned host (index HostId - lo): its records. cnt starts at 0 (the host code's memset).
__global__ __launch_bounds__(kDtThreads) void k_dt_count(const u64x2* __restrict__ a, uint64_t na, const u64x2* __restrict__ b,
                                                         uint64_t nb, uint32_t lo, uint32_t nH,
                                                         unsigned long long* __restrict__ cnt, DtHdr* __restrict__ hdr) {
  const uint64_t n = na + nb;
  for (uint64_t i = (uint64_t)blockIdx.x * kDtThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kDtThreads) {
    const u64x2 q1 = (i < na ? a + i * kRecPieces : b + (i - na) * kRecPieces)[1];
    const uint32_t host = (uint32_t)q1.y, idx = host - lo;
    if (idx >= nH) {
      report_fail(&hdr->err, &hdr->err_host, DT_EHOST, host);
      continue;
    }
    atomicAdd(&cnt[idx], 1ull);
  }
}

// what k_dt_scan scans: a host's records, 1 for a host that has any, and 1 in its class when the
// segment is too large for a wave
struct DtSum {
  uint64_t c;
  uint32_t s, m, b;
};
__device__ __forceinline__ DtSum operator+(DtSum x, DtSum y) { return DtSum{x.c + y.c, x.s + y.s, x.m + y.m, x.b + y.b}; }
__device__ __forceinline__ DtSum scan_shfl_up(DtSum v, uint32_t d) {
  return DtSum{__shfl_up(v.c, d), __shfl_up(v.s, d), __shfl_up(v.m, d), __shfl_up(v.b, d)};
}

// 2. one workgroup scans the hosts: off[h] = records of the hosts before h, a span for every host
// with records (ascending HostId), and the span indices of the two larger classes
__global__ __launch_bounds__(kScanThreads) void k_dt_scan(const unsigned long long* __restrict__ cnt, uint32_t lo, uint32_t nH,
                                                          uint64_t* __restrict__ off, sgn_trace_span* __restrict__ spans,
                                                          uint32_t* __restrict__ mid, uint32_t* __restrict__ big, uint64_t list_cap,
                                                          DtHdr* __restrict__ hdr) {
  unsigned long long largest = 0;
  const DtSum sum = tiled_scan<DtSum>(
      nH,
      [&](uint32_t h) {
        const uint64_t c = cnt[h];
        largest = c > largest ? c : largest;
        return DtSum{c, c ? 1u : 0u, c > kWaveMax && c <= kTile ? 1u : 0u, c > kTile ? 1u : 0u};
      },
      [&](uint32_t h, DtSum before, DtSum own) {
        off[h] = before.c;
        if (own.c && before.s < list_cap) spans[before.s] = sgn_trace_span{lo + h, 0u, before.c, own.c};
        if (own.m && before.m < list_cap) mid[before.m] = before.s;
        if (own.b && before.b < list_cap) big[before.b] = before.s;
      });
  if (largest) atomicMax(&hdr->largest, largest);
  if (threadIdx.x == 0) {
    hdr->total = sum.c;
    hdr->n_spans = sum.s;
    hdr->n_mid = sum.m;
    hdr->n_big = sum.b;
  }
}

// 3. every record to its host's segment of x, in the order the cursor gives. cur starts at 0. A
// record outside its segment — impossible while cnt is the count of these same inputs — is skipped
// and reported, never stored.
__global__ __launch_bounds__(kDtThreads) void k_dt_scatter(const u64x2* __restrict__ a, uint64_t na, const u64x2* __restrict__ b,
                                                           uint64_t nb, uint32_t lo, uint32_t nH,
                                                           const unsigned long long* __restrict__ cnt,
                                                           unsigned long long* __restrict__ cur, const uint64_t* __restrict__ off,
                                                           u64x2* __restrict__ x, DtHdr* __restrict__ hdr) {
  const uint64_t n = na + nb;
  for (uint64_t i = (uint64_t)blockIdx.x * kDtThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kDtThreads) {
    const Rec r = input_load(a, na, b, i);
    const uint32_t host = rec_host(r), idx = host - lo;
    uint64_t j = ~0ull;
    if (idx < nH) {
      const uint64_t k = atomicAdd(&cur[idx], 1ull);
      const uint64_t o = off[idx];
      if (k < cnt[idx] && o < n && k < n - o) j = o + k;
    }
    if (j >= n) {
      report_fail(&hdr->err, &hdr->err_host, DT_ERANGE, host);
      continue;
    }
    rec_store(x, j, r);
  }
}

// a span as the order kernels use it: false (and reported) when it does not lie inside the n records
__device__ __forceinline__ bool span_get(const sgn_trace_span* __restrict__ spans, uint64_t s, uint64_t n, uint64_t* first,
                                         uint64_t* m, DtHdr* __restrict__ hdr) {
  const sgn_trace_span sp = spans[s];
  *first = sp.first;
  *m = sp.count;
  if (sp.first > n || sp.count > n - sp.first) {
    report_fail(&hdr->err, &hdr->err_host, DT_ESPAN, sp.host);
    return false;
  }
  return true;
}

// 4a. a wave per segment of at most kWaveMax records, four segments a workgroup: lane l holds record
// l, and its place is the number of the segment's records that go before it (equal keys: the lower
// lane first, so the places are a permutation whatever the keys)
__global__ __launch_bounds__(kDtThreads) void k_dt_order_wave(const sgn_trace_span* __restrict__ spans, uint64_t n_spans,
                                                              const u64x2* __restrict__ x, u64x2* __restrict__ y, uint64_t n,
                                                              DtHdr* __restrict__ hdr) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w0 = (uint64_t)blockIdx.x * (kDtThreads / 64) + (threadIdx.x >> 6);
  for (uint64_t s = w0; s < n_spans; s += (uint64_t)gridDim.x * (kDtThreads / 64)) {
    uint64_t first, m64;
    if (!span_get(spans, s, n, &first, &m64, hdr)) continue;  // (uniform over the wave)
    if (m64 > kWaveMax) continue;
    const uint32_t m = (uint32_t)m64;
    Rec r{};
    if (lane < m) r = rec_load(x, first + lane);
    const Key me = rec_key(r);
    uint32_t rank = 0;
    for (uint32_t j = 0; j < m; j++) {  // (every lane runs the loop: the shuffles read lane j)
      const Key o{__shfl(me.time, j), __shfl(me.eid, j), __shfl(me.src, j), __shfl(me.tag, j), __shfl(me.st, j)};
      rank += key_less(o, me) || (j < lane && key_equal(o, me)) ? 1u : 0u;
    }
    if (lane < m && rank < m) rec_store(y, first + rank, r);
  }
}

// 4b. a workgroup per tile of at most kTile records: the tiles of the segments `list` names (span
// indices), tile t of a segment being its records [t * kTile, (t + 1) * kTile). Keys and indices in
// LDS; a bitonic network over the next power of two orders the indices (an index past the tile's
// length stands for a key above every key); then record idx[p] of the tile goes to place p.
__global__ __launch_bounds__(kDtThreads) void k_dt_order_tile(const sgn_trace_span* __restrict__ spans,
                                                              const uint32_t* __restrict__ list, uint32_t n_list,
                                                              const u64x2* __restrict__ x, u64x2* __restrict__ y, uint64_t n,
                                                              DtHdr* __restrict__ hdr) {
  __shared__ uint64_t s_time[kTile], s_eid[kTile];
  __shared__ uint32_t s_src[kTile], s_tag[kTile], s_st[kTile], s_idx[kTile];
  for (uint32_t e = blockIdx.x; e < n_list; e += gridDim.x) {
    uint64_t first, m;
    if (!span_get(spans, list[e], n, &first, &m, hdr)) continue;  // (uniform over the workgroup)
    const uint64_t n_tiles = (m + kTile - 1) / kTile;
    for (uint64_t t = blockIdx.y; t < n_tiles; t += gridDim.y) {
      const uint64_t base = first + t * kTile;
      const uint32_t len = (uint32_t)std::min<uint64_t>(kTile, m - t * kTile);
      uint32_t P = 2;
      while (P < len) P <<= 1;
      for (uint32_t i = threadIdx.x; i < P; i += kDtThreads) {
        if (i < len) {
          const Key k = rec_key(rec_load(x, base + i));
          s_time[i] = k.time;
          s_eid[i] = k.eid;
          s_src[i] = k.src;
          s_tag[i] = k.tag;
          s_st[i] = k.st;
        }
        s_idx[i] = i;
      }
      __syncthreads();
      // index a goes before index b: a total order (equal keys and the padding by index)
      auto before = [&](uint32_t a, uint32_t b) {
        if (a >= len || b >= len) return a < b;
        const Key ka{s_time[a], s_eid[a], s_src[a], s_tag[a], s_st[a]}, kb{s_time[b], s_eid[b], s_src[b], s_tag[b], s_st[b]};
        return key_less(ka, kb) || (a < b && key_equal(ka, kb));
      };
      for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
          for (uint32_t i = threadIdx.x; i < P; i += kDtThreads) {
            const uint32_t l = i ^ j;
            if (l > i) {
              const uint32_t ia = s_idx[i], ib = s_idx[l];
              const bool up = (i & k) == 0;
              if (before(ib, ia) == up) {
                s_idx[i] = ib;
                s_idx[l] = ia;
              }
            }
          }
          __syncthreads();
        }
      }
      for (uint32_t p = threadIdx.x; p < len; p += kDtThreads) {
        const uint32_t src = s_idx[p];
        if (src < len) rec_store(y, base + p, rec_load(x, base + src));
      }
      __syncthreads();  // (the next tile writes the keys)
    }
  }
}

// 4c. one merge pass over the segments `list` names: the sorted runs of w records of src, pairwise,
// into runs of 2w records of dst (a last run without a partner is copied). A thread produces
// kMergePer consecutive outputs: it bisects their diagonal of the pair's merge path (the left run
// first on equal keys), then merges serially. w is a multiple of kMergePer, so a thread's outputs
// lie in one pair.
__global__ __launch_bounds__(kDtThreads) void k_dt_merge(const sgn_trace_span* __restrict__ spans, const uint32_t* __restrict__ list,
                                                         uint32_t n_list, const u64x2* __restrict__ src, u64x2* __restrict__ dst,
                                                         uint64_t n, uint64_t w, DtHdr* __restrict__ hdr) {
  for (uint32_t e = blockIdx.y; e < n_list; e += gridDim.y) {
    uint64_t first, m;
    if (!span_get(spans, list[e], n, &first, &m, hdr)) continue;
    const uint64_t n_chunks = (m + kMergePer - 1) / kMergePer;
    for (uint64_t c = (uint64_t)blockIdx.x * kDtThreads + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * kDtThreads) {
      const uint64_t o0 = c * kMergePer;                       // the first output, within the segment
      const uint32_t no = (uint32_t)std::min<uint64_t>(kMergePer, m - o0);
      const uint64_t a0 = o0 - o0 % (2 * w);                   // the pair: a[a0 .. a0 + la), b[b0 .. b0 + lb)
      const uint64_t la = std::min<uint64_t>(w, m - a0), b0 = a0 + la;
      const uint64_t lb = std::min<uint64_t>(w, m - b0);
      const uint64_t d = o0 - a0;                              // the diagonal: d outputs of the pair lie before
      const u64x2* A = src + (first + a0) * kRecPieces;
      const u64x2* B = src + (first + b0) * kRecPieces;
      uint64_t lo = d > lb ? d - lb : 0, hi = std::min<uint64_t>(d, la);
      while (lo < hi) {  // the outputs before d take lo of a's records
        const uint64_t mid = (lo + hi) >> 1;
        if (key_less(rec_key(rec_load(B, d - 1 - mid)), rec_key(rec_load(A, mid)))) hi = mid;
        else lo = mid + 1;
      }
      uint64_t i = lo, j = d - lo;
      Rec ra{}, rb{};
      if (i < la) ra = rec_load(A, i);
      if (j < lb) rb = rec_load(B, j);
      for (uint32_t k = 0; k < no; k++) {
        const bool take_a = j >= lb || (i < la && !key_less(rec_key(rb), rec_key(ra)));
        if (take_a) {
          rec_store(dst, first + o0 + k, ra);
          if (++i < la) ra = rec_load(A, i);
        } else {
          rec_store(dst, first + o0 + k, rb);
          if (++j < lb) rb = rec_load(B, j);
        }
      }
    }
  }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
namespace {

// the scratch: header, per-host words, spans and class lists, the two record buffers, the upload
struct DtLay {
  size_t hdr, cnt, cur, off, spans, mid, big, x, y, up, bytes;
};
DtLay dt_lay(uint32_t nH, uint64_t n, uint64_t n_up) {
  const size_t lists = (size_t)std::min<uint64_t>(nH, n);  // (at most one span per host and per record)
  ScratchLay s;
  DtLay l;
  l.hdr = s.take(sizeof(DtHdr), 128);
  l.cnt = s.take((size_t)nH * 8, 8);  // (header, cnt and cur adjacent: one memset to zero)
  l.cur = s.take((size_t)nH * 8, 8);
  l.off = s.take((size_t)nH * 8, 128);
  l.spans = s.take(lists * sizeof(sgn_trace_span), 128);
  l.mid = s.take(lists * 4, 128);
  l.big = s.take(lists * 4, 128);
  l.x = s.take((size_t)n * sizeof(sgn_drain_rec), 128);
  l.y = s.take((size_t)n * sizeof(sgn_drain_rec), 128);
  l.up = s.take((size_t)n_up * sizeof(sgn_drain_rec), 128);
  l.bytes = s.take(0, 128);
  return l;
}

int dt_ensure(sgn_ctx* ctx, size_t bytes, const char* what) {
  if (!ctx->dt_ev[0] && !ctx->dt_ev.make()) return set_error(ctx, SGN_EDEVICE, std::string("hipEventCreate failed (") + what + ")");
  if (ctx->dt_bytes >= bytes) return 0;
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {  // (the old scratch stays: nothing changed)
    (void)hipGetLastError();
    return set_error(ctx, SGN_ENOMEM, std::string("device allocation failed (") + what + ")");
  }
  if (ctx->dt_mem) (void)hipFree(ctx->dt_mem);
  ctx->dt_mem = p;
  ctx->dt_bytes = bytes;
  return 0;
}

// The four stages on n = na + nb records of hosts [lo, lo + nH): d_a (anywhere on the device) and
// the nb records at the scratch's upload area (the caller put them there, on the context's stream).
// All or nothing under the capacity rule; on success out holds the ordered records and spans the
// spans. The scratch must have been laid out by dt_lay(nH, n, n_up) and hold that much.
int dt_run(sgn_ctx* ctx, const char* what, const sgn_drain_rec* d_a, uint64_t na, uint64_t nb, uint64_t n_up, uint32_t lo,
           uint32_t nH, sgn_drain_rec* out, uint64_t cap, uint64_t* n_out, sgn_trace_span* spans, uint64_t span_cap,
           uint64_t* n_spans, std::chrono::steady_clock::time_point t_begin) {
  const uint64_t n = na + nb;
  const DtLay L = dt_lay(nH, n, n_up);
  char* m = (char*)ctx->dt_mem;
  DtHdr* d_hdr = (DtHdr*)(m + L.hdr);
  unsigned long long* d_cnt = (unsigned long long*)(m + L.cnt);
  unsigned long long* d_cur = (unsigned long long*)(m + L.cur);
  uint64_t* d_off = (uint64_t*)(m + L.off);
  sgn_trace_span* d_spans = (sgn_trace_span*)(m + L.spans);
  uint32_t* d_mid = (uint32_t*)(m + L.mid);
  uint32_t* d_big = (uint32_t*)(m + L.big);
  u64x2* d_x = (u64x2*)(m + L.x);
  u64x2* d_y = (u64x2*)(m + L.y);
  const u64x2* d_b = (const u64x2*)(m + L.up);
  const uint64_t list_cap = std::min<uint64_t>(nH, n);
  const ReportEvents<8>& E = ctx->dt_ev;
  hipStream_t st = ctx->stream;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(kDtMaxBlocks, (n + kDtThreads - 1) / kDtThreads);
  const std::string pre = std::string(what) + ": ";

  SGN_HIP(ctx, hipMemsetAsync(m + L.hdr, 0, L.cur + (size_t)nH * 8 - L.hdr, st));  // header, cnt, cur
  (void)hipEventRecord(E[0], st);
  hipLaunchKernelGGL(k_dt_count, dim3(blocks), dim3(kDtThreads), 0, st, (const u64x2*)d_a, na, d_b, nb, lo, nH, d_cnt, d_hdr);
  (void)hipEventRecord(E[1], st);
  hipLaunchKernelGGL(k_dt_scan, dim3(1), dim3(kScanThreads), 0, st, (const unsigned long long*)d_cnt, lo, nH, d_off, d_spans, d_mid,
                     d_big, list_cap, d_hdr);
  (void)hipEventRecord(E[2], st);
  DtHdr h{};
  if (int rc = read_header(ctx, d_hdr, &h)) return rc;
  auto bad = [&](const DtHdr& x) {
    const char* why = x.err & DT_EHOST    ? "a record of a host outside the owned range: host "
                      : x.err & DT_ERANGE ? "a record outside its host's segment: host "
                                          : "a span outside the record buffer: host ";
    return set_error(ctx, SGN_EDEVICE, pre + why + std::to_string(x.err_host) + " (nothing was taken)");
  };
  if (h.err) return bad(h);
  if (h.total != n || h.n_spans > list_cap || h.largest > n || (uint64_t)h.n_mid + h.n_big > h.n_spans)
    return set_error(ctx, SGN_EDEVICE, pre + "the per-host counts add up to " + std::to_string(h.total) + " of " + std::to_string(n) +
                                           " pending records (nothing was taken)");
  if (cap < n || (spans && span_cap < h.n_spans)) {
    *n_out = n;
    if (n_spans) *n_spans = h.n_spans;
    return set_error(ctx, SGN_ERANGE, pre + std::to_string(n) + " records of " + std::to_string(h.n_spans) +
                                          " hosts are pending, the caller's arrays are smaller (nothing was taken)");
  }
  (void)hipEventRecord(E[3], st);
  hipLaunchKernelGGL(k_dt_scatter, dim3(blocks), dim3(kDtThreads), 0, st, (const u64x2*)d_a, na, d_b, nb, lo, nH,
                     (const unsigned long long*)d_cnt, d_cur, (const uint64_t*)d_off, d_x, d_hdr);
  (void)hipEventRecord(E[4], st);
  // the order: every class reads x and writes y; the merge passes of the large segments then go
  // y -> x -> y, an even number of them
  const uint64_t wave_blocks = std::min<uint64_t>((h.n_spans + kDtThreads / 64 - 1) / (kDtThreads / 64), 1u << 20);
  hipLaunchKernelGGL(k_dt_order_wave, dim3((uint32_t)wave_blocks), dim3(kDtThreads), 0, st, (const sgn_trace_span*)d_spans, h.n_spans,
                     (const u64x2*)d_x, d_y, n, d_hdr);
  if (h.n_mid)
    hipLaunchKernelGGL(k_dt_order_tile, dim3(std::min<uint32_t>(h.n_mid, 1u << 20), 1), dim3(kDtThreads), 0, st,
                       (const sgn_trace_span*)d_spans, (const uint32_t*)d_mid, h.n_mid, (const u64x2*)d_x, d_y, n, d_hdr);
  if (h.n_big) {
    const uint64_t tiles = (h.largest + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_dt_order_tile, dim3(std::min<uint32_t>(h.n_big, 1u << 16), (uint32_t)std::min<uint64_t>(tiles, 1024)),
                       dim3(kDtThreads), 0, st, (const sgn_trace_span*)d_spans, (const uint32_t*)d_big, h.n_big, (const u64x2*)d_x, d_y,
                       n, d_hdr);
    uint32_t passes = 0;
    for (uint64_t w = kTile; w < h.largest; w <<= 1) passes++;
    passes += passes & 1u;
    const uint64_t chunks = (h.largest + kMergePer - 1) / kMergePer;
    const dim3 grid((uint32_t)std::min<uint64_t>((chunks + kDtThreads - 1) / kDtThreads, 1024), std::min<uint32_t>(h.n_big, 1024));
    uint64_t w = kTile;
    for (uint32_t p = 0; p < passes; p++, w <<= 1)
      hipLaunchKernelGGL(k_dt_merge, grid, dim3(kDtThreads), 0, st, (const sgn_trace_span*)d_spans, (const uint32_t*)d_big, h.n_big,
                         (const u64x2*)((p & 1u) ? d_x : d_y), (p & 1u) ? d_y : d_x, n, w, d_hdr);
  }
  (void)hipEventRecord(E[5], st);
  if (int rc = read_header(ctx, d_hdr, &h)) return rc;
  if (h.err) return bad(h);
  SGN_HIP(ctx, hipMemcpyAsync(out, d_y, n * sizeof(sgn_drain_rec), hipMemcpyDeviceToHost, st));
  if (spans && h.n_spans)
    SGN_HIP(ctx, hipMemcpyAsync(spans, d_spans, h.n_spans * sizeof(sgn_trace_span), hipMemcpyDeviceToHost, st));
  (void)hipEventRecord(E[6], st);
  SGN_HIP(ctx, hipStreamSynchronize(st));
  *n_out = n;
  if (n_spans) *n_spans = h.n_spans;
  sgn_drain_take_timing& T = ctx->dt_timing;
  T.kernel_ms[0] = elapsed_ms(E[0], E[1]);
  T.kernel_ms[1] = elapsed_ms(E[1], E[2]);
  T.kernel_ms[2] = elapsed_ms(E[3], E[4]);
  T.kernel_ms[3] = elapsed_ms(E[4], E[5]);
  T.copy_ms = elapsed_ms(E[5], E[6]);
  T.records = n;
  T.hosts = h.n_spans;
  T.largest_span = h.largest;
  T.spans_by_class[0] = h.n_spans - h.n_mid - h.n_big;
  T.spans_by_class[1] = h.n_mid;
  T.spans_by_class[2] = h.n_big;
  T.total_ms = ms_since(t_begin);
  return 0;
}

sgn_drain_take_timing dt_timing_zero() {
  sgn_drain_take_timing t{};
  t.wave_max = kWaveMax;
  t.tile = kTile;
  return t;
}

int dt_precheck(sgn_ctx* ctx, const char* what) {
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (ctx->S.tkind != SGN_TRAFFIC_EXTERNAL) return set_error(ctx, SGN_ESTATE, std::string(what) + " needs SGN_TRAFFIC_EXTERNAL traffic");
  return 0;
}

}  // namespace

namespace sgn {

void drain_take_release(sgn_ctx* ctx) {
  if (ctx->dt_mem) (void)hipFree(ctx->dt_mem);
  ctx->dt_mem = nullptr;
  ctx->dt_bytes = 0;
  ctx->dt_ev.release();
  ctx->dt_timing = dt_timing_zero();
}

}  // namespace sgn

extern "C" {

int sgn_drain_pending(sgn_ctx* ctx, uint64_t* n) {
  if (n) *n = 0;
  if (!ctx || !n) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_drain_pending: null argument") : SGN_EINVAL;
  if (int rc = dt_precheck(ctx, "sgn_drain_pending")) return rc;
  if (int rc = sync_ctrl(ctx)) return rc;
  *n = ctx->h_ctrl->drain_n + ctx->drain_held.size();
  return 0;
}

int sgn_drain_take(sgn_ctx* ctx, sgn_drain_rec* out, uint64_t cap, uint64_t* n_out, sgn_trace_span* spans, uint64_t span_cap,
                   uint64_t* n_spans) {
  if (n_out) *n_out = 0;
  if (n_spans) *n_spans = 0;
  if (!ctx || !n_out || (!out && cap) || (!spans && span_cap))
    return ctx ? set_error(ctx, SGN_EINVAL, "sgn_drain_take: null argument") : SGN_EINVAL;
  if (int rc = dt_precheck(ctx, "sgn_drain_take")) return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = sync_ctrl(ctx)) return rc;
  const DevSim& S = ctx->S;
  const uint64_t na = ctx->h_ctrl->drain_n, nb = ctx->drain_held.size(), n = na + nb;
  ctx->dt_timing = dt_timing_zero();
  if (na > S.drain_cap) return set_error(ctx, SGN_EOVERFLOW, "sgn_drain_take: more records pending than the drain buffer holds");
  if (n == 0) {
    ctx->dt_timing.total_ms = ms_since(t_begin);
    return 0;
  }
  if (int rc = dt_ensure(ctx, dt_lay(S.nH, n, nb).bytes, "sgn_drain_take")) return rc;
  if (nb)  // the held records behind the device's, as the second input
    SGN_HIP(ctx, hipMemcpyAsync((char*)ctx->dt_mem + dt_lay(S.nH, n, nb).up, ctx->drain_held.data(), nb * sizeof(sgn_drain_rec),
                                hipMemcpyHostToDevice, ctx->stream));
  if (int rc = dt_run(ctx, "sgn_drain_take", (const sgn_drain_rec*)S.drain, na, nb, nb, S.lo, S.nH, out, cap, n_out, spans, span_cap,
                      n_spans, t_begin))
    return rc;
  // the records are the caller's: the handles by sgn_drain's rule (a held record's handle comes out
  // the same again: the rule reads only the record and the append-only handle table), the device
  // buffer empty, nothing held
  for (uint64_t i = 0; i < n; i++) {
    sgn_drain_rec& r = out[i];
    const uint32_t slot = r.tag & SGN_TAG_SLOT_MASK;
    r.handle = ((r.tag & SGN_TAG_EXT) && r.src_host >= ctx->lo && r.src_host < ctx->hi && slot < ctx->handles.size())
                   ? ctx->handles[slot] : 0;
  }
  ctx->ctrl_fresh = false;
  if (na) {
    const uint64_t zero = 0;
    SGN_HIP(ctx, hipMemcpy((char*)S.ctrl + offsetof(Ctrl, drain_n), &zero, 8, hipMemcpyHostToDevice));
    ctx->h_ctrl->drain_n = 0;
  }
  ctx->drain_held.clear();
  ctx->dt_timing.total_ms = ms_since(t_begin);
  return 0;
}

int sgn_drain_take_timing_get(sgn_ctx* ctx, sgn_drain_take_timing* out) {
  if (!ctx || !out) return SGN_EINVAL;
  *out = ctx->dt_timing;
  out->wave_max = kWaveMax;
  out->tile = kTile;
  return 0;
}

int sgn_selftest_drain_order(sgn_ctx* ctx, const sgn_drain_rec* recs, uint64_t n, uint32_t host_lo, uint32_t n_hosts,
                             sgn_drain_rec* out, sgn_trace_span* spans, uint64_t span_cap, uint64_t* n_spans) {
  if (n_spans) *n_spans = 0;
  if (!ctx || (n && (!recs || !out)) || (!spans && span_cap))
    return ctx ? set_error(ctx, SGN_EINVAL, "sgn_selftest_drain_order: null argument") : SGN_EINVAL;
  const auto t_begin = std::chrono::steady_clock::now();
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  ctx->dt_timing = dt_timing_zero();
  if (n == 0) return 0;
  if (int rc = dt_ensure(ctx, dt_lay(n_hosts, n, n).bytes, "sgn_selftest_drain_order")) return rc;
  // all n records go to the upload area; its first half then stands for the device buffer (the
  // kernels' first input), the rest for the held records (their second)
  const size_t up = dt_lay(n_hosts, n, n).up;
  const uint64_t na = n / 2;
  SGN_HIP(ctx, hipMemcpyAsync((char*)ctx->dt_mem + up, recs + na, (n - na) * sizeof(sgn_drain_rec), hipMemcpyHostToDevice, ctx->stream));
  if (na)
    SGN_HIP(ctx, hipMemcpyAsync((char*)ctx->dt_mem + up + (n - na) * sizeof(sgn_drain_rec), recs, na * sizeof(sgn_drain_rec),
                                hipMemcpyHostToDevice, ctx->stream));
  uint64_t n_got = 0;
  return dt_run(ctx, "sgn_selftest_drain_order", (const sgn_drain_rec*)((char*)ctx->dt_mem + up + (n - na) * sizeof(sgn_drain_rec)), na,
                n - na, n, host_lo, n_hosts, out, n, &n_got, spans, span_cap, n_spans, t_begin);
}

}  // extern "C"

uint64_t sgn::layout_sig_drain_take() { return kLayoutSig; }
