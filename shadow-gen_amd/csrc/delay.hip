// delay.hip — the router delay report: queueing delay per packet, folded on the device
// (sgn_delay_enable, sgn_delay_fold, sgn_delay_get, sgn_delay_clear, sgn_selftest_delay_fold).
//
// A packet's router delay at host h is the `a` of its exit record (DELIVER or CODEL_DROP) minus the
// `a` of its POP record. Within one host the router is FIFO, so the k-th exit pairs with the k-th
// POP; packets still in the router when an interval ends wait in the CARRY, per owned host the FIFO
// of {pop time, source event id, source host}, compact per-host segments in device memory. A fold
// runs on what a take has just built — the staging buffer ordered by (host, seq), one span per host
// (trace_take.hip) — and leaves every record on the device:
//   1. k_delay_count   one pass over the records: per owned host its pops and its exits (a wave whose
//                      64 records are of one host adds two popcounts, else a lane an atomic); the same
//                      launch lists the spans too large for a wave and finds the largest;
//   2. k_delay_scan    one workgroup (tiled_scan over the hosts): the new carry length
//                      c + pops - exits, its offset, the total — the host grows the buffer before
//                      anything is written — and the too-many-exits error;
//   3. k_delay_keep    one lane per entry of the old carry: entry k of a host survives when
//                      k >= exits, at place k - exits of the host's new segment;
//      k_delay_match_wave  a span of at most kDlWave records: one wave, a record a lane; ballots and
//                      popcounts rank the pops and the exits; exit j pairs with entry j of (old carry
//                      ++ the span's pops): an old entry is loaded, a pop of the span comes from its
//                      lane by a shuffle (the lane of the q-th set bit of the pop ballot);
//      k_delay_match_walk  a larger span: one workgroup walks it in chunks of kDlTile records with a
//                      block scan and a carried base; the pops leave their record index in a scratch
//                      array by rank, the exits of the same or a later chunk read it;
//                      both: pop c + p goes to the new carry when c + p >= exits; per-span sums,
//                      counts and maximum go to a delta row, the histograms to LDS (one atomic per
//                      non-empty bin and workgroup at the end);
//   4. k_delay_commit  only when nothing failed: the delta rows into the per-host accumulators, the
//                      fold's histograms into the report's. The host then swaps the carry buffers.
// Every kernel reads one carry buffer and writes the other, and nothing the report keeps changes
// before the commit: a failed fold leaves accumulators and carry as they were.
// sgn_delay_get is count -> scan -> scatter over the accumulators (the shape of backlog.hip).
//
// A sgn_trace_rec is seven 8-byte words: {kind | host << 32, peer | flags << 32, a, b, c, seq,
// rng_pos}; the kernels here load words 0, 1, 2 and 4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "backlog_read.h"
#include "report_common.h"

using namespace sgn;
using namespace sgn::report;
using namespace sgn::backlog_read;

// ---- device side ----------------------------------------------------------------------------
namespace {

constexpr uint32_t kDlThreads = 256;     // count, keep, match_wave, commit, the rows kernels
constexpr uint32_t kDlMaxBlocks = 2048;  // grid-stride above that
constexpr uint32_t kDlWave = 64;         // records a wave matches at once
constexpr uint32_t kDlTile = 1024;       // records a workgroup handles per pass (a record a thread)
constexpr uint32_t kRecWords = sizeof(sgn_trace_rec) / 8;
constexpr uint32_t kBins = SGN_DELAY_BINS;
static_assert(sizeof(sgn_trace_rec) == 56 && offsetof(sgn_trace_rec, kind) == 0 && offsetof(sgn_trace_rec, host) == 4 &&
                  offsetof(sgn_trace_rec, peer) == 8 && offsetof(sgn_trace_rec, a) == 16 && offsetof(sgn_trace_rec, c) == 32,
              "words 0, 1, 2 and 4");
static_assert(sizeof(sgn_delay_row) == 64 && offsetof(sgn_delay_row, delivered) == 16 &&
                  offsetof(sgn_delay_row, delay_sum_delivered) == 32 && offsetof(sgn_delay_row, delay_max) == 48,
              "a row is four 16-byte stores");
static_assert(sizeof(sgn_delay_info) == 15 * 8 + 2 * kBins * 8, "");
static_assert(INVALID == ~0ull, "an unknown entry's pop time");

enum : uint32_t {
  DL_EMANY = 1u,   // a host has more exits than carry plus pops
  DL_EORDER = 2u,  // an exit before its pop in the host's stream
  DL_EPAIR = 4u,   // a matched pair disagrees in (peer, c), or exits before it was popped
  DL_ESPAN = 8u,   // a span, a record index or a carry place outside its buffer (skipped)
  DL_NERR = 4,
};
// the header of one fold
struct __attribute__((aligned(16))) DlHdr {
  uint32_t err, n_big;          // DL_E*; spans of more than kDlWave records
  uint32_t err_host[DL_NERR];   // the lowest offender of every error bit (HostId)
  uint64_t carry_total;         // k_delay_scan: entries of the new carry
  unsigned long long largest;   // the largest span
  unsigned long long hist[2][kBins];  // this fold's matched exits: delivered, dropped
};
// what the report keeps beside the per-host accumulators
struct DlTot {
  unsigned long long hist[2][kBins];
};
// a carry entry; an unknown one (a packet that stood at the router at sgn_delay_enable) has t == INVALID
struct __attribute__((aligned(8))) DlEnt {
  uint64_t t, c;         // pop time, source event id
  uint32_t peer, hidx;   // source HostId; the owner (HostId - lo)
};
static_assert(sizeof(DlEnt) == 24, "");
// a host's accumulators, and a span's contribution to them
struct __attribute__((aligned(16))) DlAcc {
  uint64_t nd, nx, sd, sx, mx, um;  // delivered, dropped, their delay sums, the largest delay, unmatched
  uint64_t pad[2];
};
static_assert(sizeof(DlAcc) == 64, "");

__device__ __forceinline__ void dl_fail(DlHdr* hdr, uint32_t bit, uint32_t host) {
  atomicOr(&hdr->err, bit);
  atomicMin(&hdr->err_host[__ffs((int)bit) - 1], host);
}
__device__ __forceinline__ bool is_pop(uint32_t kind) { return kind == SGN_TRACE_POP; }
__device__ __forceinline__ bool is_exit(uint32_t kind) { return kind == SGN_TRACE_DELIVER || kind == SGN_TRACE_CODEL_DROP; }
// bin 0: 0; bin k: [2^(k-1), 2^k); the last bin: everything from 2^(kBins - 2) up
__device__ __forceinline__ uint32_t delay_bin(uint64_t d) {
  const uint32_t len = d ? 64u - (uint32_t)__clzll((long long)d) : 0u;
  return len < kBins - 1 ? len : kBins - 1;
}
// the position of the r-th (from 0) set bit of mask; r below the mask's popcount
__device__ __forceinline__ uint32_t select_bit(uint64_t mask, uint32_t r) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t s = 32; s > 0; s >>= 1) {
    const uint32_t cnt = (uint32_t)__popcll((mask >> pos) & ((1ull << s) - 1));
    if (r >= cnt) {
      pos += s;
      r -= cnt;
    }
  }
  return pos;
}

// 1. per owned host (index HostId - lo) its pops and its exits; pops and exits start at 0. A record
// of a host outside the range was refused by the take before. Then the spans: the large ones listed
// (in any order), the largest found.
__global__ __launch_bounds__(kDlThreads) void k_delay_count(const uint64_t* __restrict__ recs, uint64_t n,
                                                            const sgn_trace_span* __restrict__ spans, uint64_t n_spans, uint32_t lo,
                                                            uint32_t nH, unsigned long long* __restrict__ pops,
                                                            unsigned long long* __restrict__ exits, uint32_t* __restrict__ big,
                                                            DlHdr* __restrict__ hdr) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * kDlThreads;
  for (uint64_t b = (uint64_t)blockIdx.x * kDlThreads; b < n; b += stride) {  // (uniform over the workgroup)
    const uint64_t i = b + threadIdx.x;
    uint32_t idx = 0xFFFFFFFFu;
    bool p = false, x = false;
    if (i < n) {
      const uint64_t w0 = recs[i * kRecWords];
      idx = (uint32_t)(w0 >> 32) - lo;
      if (idx < nH) {
        p = is_pop((uint32_t)w0);
        x = is_exit((uint32_t)w0);
      } else {
        idx = 0xFFFFFFFFu;
      }
    }
    const uint32_t first = __shfl(idx, 0);
    const uint64_t bp = __ballot(p), bx = __ballot(x);
    if (__all(idx == first)) {  // the wave's records are of one host: two adds
      if (lane == 0 && first < nH) {
        if (bp) atomicAdd(&pops[first], (unsigned long long)__popcll(bp));
        if (bx) atomicAdd(&exits[first], (unsigned long long)__popcll(bx));
      }
    } else {
      if (p) atomicAdd(&pops[idx], 1ull);
      if (x) atomicAdd(&exits[idx], 1ull);
    }
  }
  unsigned long long largest = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * kDlThreads + threadIdx.x; s < n_spans; s += stride) {
    const uint64_t c = spans[s].count;
    largest = c > largest ? c : largest;
    if (c > kDlWave) {
      const uint32_t k = atomicAdd(&hdr->n_big, 1u);
      if (k < n_spans) big[k] = (uint32_t)s;  // (n_spans <= owned hosts < 2^32)
    }
  }
  largest = wave_max(largest);
  if (lane == 0 && largest) atomicMax(&hdr->largest, largest);
}

struct DlSum {
  uint64_t c;
};
__device__ __forceinline__ DlSum operator+(DlSum a, DlSum b) { return DlSum{a.c + b.c}; }
__device__ __forceinline__ DlSum scan_shfl_up(DlSum v, uint32_t d) { return DlSum{__shfl_up(v.c, d)}; }

// 2. one workgroup: a host's new carry length and the offset of its new segment
__global__ __launch_bounds__(kScanThreads) void k_delay_scan(const uint64_t* __restrict__ len_old, const unsigned long long* __restrict__ pops,
                                                             const unsigned long long* __restrict__ exits, uint32_t lo, uint32_t nH,
                                                             uint64_t* __restrict__ len_new, uint64_t* __restrict__ off_new,
                                                             DlHdr* __restrict__ hdr) {
  const DlSum sum = tiled_scan<DlSum>(
      nH,
      [&](uint32_t h) {
        const uint64_t have = len_old[h] + pops[h], x = exits[h];
        if (x > have) {
          dl_fail(hdr, DL_EMANY, lo + h);
          return DlSum{0};
        }
        return DlSum{have - x};
      },
      [&](uint32_t h, DlSum before, DlSum own) {
        len_new[h] = own.c;
        off_new[h] = before.c;
      });
  if (threadIdx.x == 0) hdr->carry_total = sum.c;
}

// the carry after sgn_delay_enable (or a self-test's standing0): unknown entries
__global__ __launch_bounds__(kDlThreads) void k_delay_fill(const uint64_t* __restrict__ len, const uint64_t* __restrict__ off, uint32_t nH,
                                                           DlEnt* __restrict__ carry, uint64_t total) {
  const uint32_t i = blockIdx.x * kDlThreads + threadIdx.x;
  if (i >= nH) return;
  const uint64_t o = off[i], m = len[i];
  if (o > total || m > total - o) return;
  for (uint64_t k = 0; k < m; k++) carry[o + k] = DlEnt{INVALID, 0, 0, i};
}

// what stands at every owned host's router now (backlog_read.h: sgn_backlog's reader), as pops
// (traced: null, or one word per owned host, 0 for a host sgn_trace_hosts left out: it produces no records)
__global__ __launch_bounds__(kDlThreads) void k_delay_standing(BkArgs a, const uint32_t* __restrict__ traced,
                                                               unsigned long long* __restrict__ pops, DlHdr* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * kDlThreads + threadIdx.x;
  if (i >= a.nH) return;
  if (traced && !traced[i]) return;  // (pops starts at 0)
  BkHost h;
  if (!bk_load(a, i, &h)) {
    dl_fail(hdr, DL_ESPAN, a.lo + i);
    return;
  }
  pops[i] = (unsigned long long)h.cq_len + (h.flags & SGN_BACKLOG_ROUTER_HELD ? 1u : 0u);
}

// 3a. the old carry's survivors to their new places
__global__ __launch_bounds__(kDlThreads) void k_delay_keep(const DlEnt* __restrict__ old_, uint64_t n_old, const unsigned long long* __restrict__ exits,
                                                           const uint64_t* __restrict__ off_old, const uint64_t* __restrict__ len_new,
                                                           const uint64_t* __restrict__ off_new, uint32_t lo, uint32_t nH,
                                                           DlEnt* __restrict__ new_, uint64_t n_new, DlHdr* __restrict__ hdr) {
  for (uint64_t e = (uint64_t)blockIdx.x * kDlThreads + threadIdx.x; e < n_old; e += (uint64_t)gridDim.x * kDlThreads) {
    const DlEnt ent = old_[e];
    if (ent.hidx >= nH) {
      dl_fail(hdr, DL_ESPAN, lo + ent.hidx);
      continue;
    }
    const uint64_t k = e - off_old[ent.hidx], x = exits[ent.hidx];
    if (k < x) continue;  // (matched in this fold)
    const uint64_t d = k - x, at = off_new[ent.hidx] + d;
    if (d >= len_new[ent.hidx] || at >= n_new) {
      dl_fail(hdr, DL_ESPAN, lo + ent.hidx);
      continue;
    }
    new_[at] = ent;
  }
}

// what the two match kernels share: a span's constants
struct DlSpan {
  uint64_t first, m;        // its records
  uint64_t c_old, x;        // the old carry's length, the span's exits
  uint64_t oo, on, ln;      // the old segment's offset, the new one's offset and length
  uint32_t hi, host;
};
struct DlBufs {
  const uint64_t* recs;     // the ordered records
  uint64_t n;
  const sgn_trace_span* spans;
  const uint64_t *len_old, *off_old, *len_new, *off_new;
  const unsigned long long* exits;
  const DlEnt* carry_old;
  DlEnt* carry_new;
  uint64_t n_old, n_new;
  DlAcc* delta;             // one per span
  uint32_t lo, nH;
};
// false (and reported): the span does not lie inside the records or its host is not owned
__device__ __forceinline__ bool dl_span(const DlBufs& B, uint64_t s, DlSpan* q, DlHdr* hdr, bool report) {
  const sgn_trace_span sp = B.spans[s];
  q->first = sp.first;
  q->m = sp.count;
  q->host = sp.host;
  q->hi = sp.host - B.lo;
  if (q->hi >= B.nH || sp.first > B.n || sp.count > B.n - sp.first) {
    if (report) dl_fail(hdr, DL_ESPAN, sp.host);
    return false;
  }
  q->c_old = B.len_old[q->hi];
  q->x = B.exits[q->hi];
  q->oo = B.off_old[q->hi];
  q->on = B.off_new[q->hi];
  q->ln = B.len_new[q->hi];
  if (q->oo > B.n_old || q->c_old > B.n_old - q->oo) {
    if (report) dl_fail(hdr, DL_ESPAN, sp.host);
    return false;
  }
  return true;
}
// pop p of the span is entry c_old + p: it stays in the carry when the span's exits do not reach it
__device__ __forceinline__ void dl_keep_pop(const DlBufs& B, const DlSpan& q, uint64_t p, uint64_t a, uint64_t c, uint32_t peer, DlHdr* hdr) {
  const uint64_t k = q.c_old + p;
  if (k < q.x) return;
  const uint64_t d = k - q.x, at = q.on + d;
  if (d >= q.ln || at >= B.n_new) {
    dl_fail(hdr, DL_ESPAN, q.host);
    return;
  }
  B.carry_new[at] = DlEnt{a, c, peer, q.hi};
}
// an exit (kind, a, peer, c) against its entry
__device__ __forceinline__ void dl_match(uint32_t kind, uint64_t a, uint32_t peer, uint64_t c, uint64_t et, uint32_t epeer, uint64_t ec,
                                         uint32_t host, DlAcc* acc, unsigned long long (*s_hist)[kBins], DlHdr* hdr) {
  if (et == INVALID) {
    acc->um++;
    return;
  }
  if (epeer != peer || ec != c || a < et) {
    dl_fail(hdr, DL_EPAIR, host);
    return;
  }
  const uint64_t d = a - et;
  const uint32_t drop = kind == SGN_TRACE_CODEL_DROP ? 1u : 0u;
  atomicAdd(&s_hist[drop][delay_bin(d)], 1ull);
  if (drop) {
    acc->nx++;
    acc->sx += d;
  } else {
    acc->nd++;
    acc->sd += d;
  }
  acc->mx = d > acc->mx ? d : acc->mx;
}
__device__ __forceinline__ DlAcc wave_acc(const DlAcc& a) {
  DlAcc r;
  r.nd = wave_sum(a.nd);
  r.nx = wave_sum(a.nx);
  r.sd = wave_sum(a.sd);
  r.sx = wave_sum(a.sx);
  r.mx = wave_max(a.mx);
  r.um = wave_sum(a.um);
  r.pad[0] = r.pad[1] = 0;
  return r;
}
__device__ __forceinline__ void hist_zero(unsigned long long (*s_hist)[kBins]) {
  for (uint32_t t = threadIdx.x; t < 2 * kBins; t += blockDim.x) s_hist[t / kBins][t % kBins] = 0;
  __syncthreads();
}
__device__ __forceinline__ void hist_flush(unsigned long long (*s_hist)[kBins], DlHdr* hdr) {
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < 2 * kBins; t += blockDim.x) {
    const unsigned long long v = s_hist[t / kBins][t % kBins];
    if (v) atomicAdd(&hdr->hist[t / kBins][t % kBins], v);
  }
}

// 3b. a wave per span of at most kDlWave records, four spans a workgroup: lane l holds record l
__global__ __launch_bounds__(kDlThreads) void k_delay_match_wave(DlBufs B, uint64_t n_spans, DlHdr* __restrict__ hdr) {
  __shared__ unsigned long long s_hist[2][kBins];
  hist_zero(s_hist);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w0 = (uint64_t)blockIdx.x * (kDlThreads / 64) + (threadIdx.x >> 6);
  for (uint64_t s = w0; s < n_spans; s += (uint64_t)gridDim.x * (kDlThreads / 64)) {
    DlSpan q;
    if (B.spans[s].count > kDlWave) continue;            // (the walker's; uniform over the wave)
    if (!dl_span(B, s, &q, hdr, lane == 0)) continue;
    uint32_t kind = 0, peer = 0;
    uint64_t a = 0, c = 0;
    if (lane < q.m) {
      const uint64_t* w = B.recs + (q.first + lane) * kRecWords;
      const uint64_t w0r = w[0], w1 = w[1];
      kind = (uint32_t)w0r;
      peer = (uint32_t)w1;
      a = w[2];
      c = w[4];
    }
    const bool p = is_pop(kind), x = is_exit(kind);
    const uint64_t bp = __ballot(p), bx = __ballot(x);
    const uint32_t pr = rank_below(bp, lane), xr = rank_below(bx, lane);  // pops, exits before this lane
    if (p) dl_keep_pop(B, q, pr, a, c, peer, hdr);
    // exit xr pairs with entry xr of (old carry ++ the span's pops)
    const bool from_span = x && xr >= q.c_old;
    const uint64_t qq = from_span ? xr - q.c_old : 0;
    const bool found = from_span && qq < pr;  // (its pop stands before it in the stream)
    const uint32_t src = found ? select_bit(bp, (uint32_t)qq) : 0u;
    uint64_t et = __shfl(a, src), ec = __shfl(c, src);  // (every lane: the shuffles read lane src)
    uint32_t epeer = __shfl(peer, src);
    DlAcc acc{};
    if (x) {
      bool have = found;
      if (!from_span) {
        const DlEnt ent = B.carry_old[q.oo + xr];  // (xr < c_old = the old segment's length)
        et = ent.t;
        ec = ent.c;
        epeer = ent.peer;
        have = true;
      }
      if (have) dl_match(kind, a, peer, c, et, epeer, ec, q.host, &acc, s_hist, hdr);
      else dl_fail(hdr, DL_EORDER, q.host);
    }
    const DlAcc r = wave_acc(acc);
    if (lane == 0) B.delta[s] = r;
  }
  hist_flush(s_hist, hdr);
}

// 3c. a workgroup per larger span (the spans `big` lists), walked in chunks of kDlTile records, a
// record a thread: the ranks are the carried base + the waves before + the lanes before. A pop
// leaves its record index at popidx[first + its rank]; an exit whose entry is a pop of the span
// reads it after the chunk's barrier (its pop is in this chunk or an earlier one, else the exit
// came before its pop).
__global__ __launch_bounds__(kDlTile) void k_delay_match_walk(DlBufs B, const uint32_t* __restrict__ big, uint32_t n_big,
                                                              uint64_t* popidx, DlHdr* __restrict__ hdr) {
  __shared__ unsigned long long s_hist[2][kBins];
  __shared__ uint32_t s_wp[kDlTile / 64], s_wx[kDlTile / 64];
  __shared__ DlAcc s_red[kDlTile / 64];
  hist_zero(s_hist);
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  for (uint32_t e = blockIdx.x; e < n_big; e += gridDim.x) {
    const uint64_t s = big[e];
    DlSpan q;
    if (!dl_span(B, s, &q, hdr, threadIdx.x == 0)) continue;  // (uniform over the workgroup)
    uint64_t base_p = 0, base_x = 0;
    DlAcc acc{};
    for (uint64_t c0 = 0; c0 < q.m; c0 += kDlTile) {
      const uint64_t r = c0 + threadIdx.x;
      uint32_t kind = 0, peer = 0;
      uint64_t a = 0, c = 0;
      if (r < q.m) {
        const uint64_t* w = B.recs + (q.first + r) * kRecWords;
        const uint64_t w0r = w[0], w1 = w[1];
        kind = (uint32_t)w0r;
        peer = (uint32_t)w1;
        a = w[2];
        c = w[4];
      }
      const bool p = is_pop(kind), x = is_exit(kind);
      const uint64_t bp = __ballot(p), bx = __ballot(x);
      if (lane == 0) {
        s_wp[wv] = (uint32_t)__popcll(bp);
        s_wx[wv] = (uint32_t)__popcll(bx);
      }
      __syncthreads();
      uint64_t pr = base_p, xr = base_x;
      uint32_t tp = 0, tx = 0;
#pragma unroll
      for (uint32_t v = 0; v < kDlTile / 64; v++) {
        if (v < wv) {
          pr += s_wp[v];
          xr += s_wx[v];
        }
        tp += s_wp[v];
        tx += s_wx[v];
      }
      pr += rank_below(bp, lane);  // pops, exits of the span before this record
      xr += rank_below(bx, lane);
      if (p) {
        if (pr < q.m) popidx[q.first + pr] = q.first + r;
        dl_keep_pop(B, q, pr, a, c, peer, hdr);
      }
      __syncthreads();  // (this chunk's pops are listed; the wave counts were read)
      if (x) {
        uint64_t et = INVALID, ec = 0;
        uint32_t epeer = 0;
        bool have = false;
        if (xr < q.c_old) {
          const DlEnt ent = B.carry_old[q.oo + xr];
          et = ent.t;
          ec = ent.c;
          epeer = ent.peer;
          have = true;
        } else if (xr - q.c_old < pr) {
          const uint64_t i = popidx[q.first + (xr - q.c_old)];
          if (i < B.n) {
            const uint64_t* w = B.recs + i * kRecWords;
            epeer = (uint32_t)w[1];
            et = w[2];
            ec = w[4];
            have = true;
          }
        }
        if (have) dl_match(kind, a, peer, c, et, epeer, ec, q.host, &acc, s_hist, hdr);
        else dl_fail(hdr, DL_EORDER, q.host);
      }
      base_p += tp;
      base_x += tx;
    }
    const DlAcc r = wave_acc(acc);
    if (lane == 0) s_red[wv] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
      DlAcc t = s_red[0];
      for (uint32_t v = 1; v < kDlTile / 64; v++) {
        t.nd += s_red[v].nd;
        t.nx += s_red[v].nx;
        t.sd += s_red[v].sd;
        t.sx += s_red[v].sx;
        t.um += s_red[v].um;
        t.mx = s_red[v].mx > t.mx ? s_red[v].mx : t.mx;
      }
      B.delta[s] = t;
    }
    __syncthreads();  // (the next span writes s_red)
  }
  hist_flush(s_hist, hdr);
}

// 4. the fold's deltas into what the report keeps (a host has one span: no atomics)
__global__ __launch_bounds__(kDlThreads) void k_delay_commit(const sgn_trace_span* __restrict__ spans, uint64_t n_spans,
                                                             const DlAcc* __restrict__ delta, uint32_t lo, uint32_t nH, DlAcc* __restrict__ acc,
                                                             const DlHdr* __restrict__ hdr, DlTot* __restrict__ tot) {
  if (blockIdx.x == 0 && threadIdx.x < 2 * kBins) {
    const unsigned long long v = hdr->hist[threadIdx.x / kBins][threadIdx.x % kBins];
    if (v) tot->hist[threadIdx.x / kBins][threadIdx.x % kBins] += v;
  }
  for (uint64_t s = (uint64_t)blockIdx.x * kDlThreads + threadIdx.x; s < n_spans; s += (uint64_t)gridDim.x * kDlThreads) {
    const uint32_t hi = spans[s].host - lo;
    if (hi >= nH) continue;
    const DlAcc d = delta[s];
    DlAcc a = acc[hi];
    a.nd += d.nd;
    a.nx += d.nx;
    a.sd += d.sd;
    a.sx += d.sx;
    a.um += d.um;
    a.mx = d.mx > a.mx ? d.mx : a.mx;
    acc[hi] = a;
  }
}

// ---- sgn_delay_get: count -> scan -> scatter over the accumulators ----
constexpr uint32_t kGetTotals = 6;
struct __attribute__((aligned(16))) DgHdr {
  uint64_t rows;
  uint64_t total[kGetTotals];
  uint64_t max;
  uint32_t max_host, max_any;
  uint32_t err, err_host;
};
// (any, delay, host) becomes the larger of itself and the other: on equal delays the lower HostId
__device__ __forceinline__ void argmax_fold(uint32_t& any, uint64_t& d, uint32_t& host, uint32_t any2, uint64_t d2, uint32_t host2) {
  if (!any2) return;
  if (!any || d2 > d || (d2 == d && host2 < host)) {
    any = 1;
    d = d2;
    host = host2;
  }
}
__device__ __forceinline__ bool dg_row(const DlAcc& a, uint64_t len) { return (len | a.nd | a.nx | a.um) != 0; }

__global__ __launch_bounds__(kDlThreads) void k_delay_rows_count(const DlAcc* __restrict__ acc, const uint64_t* __restrict__ len, uint32_t lo,
                                                                 uint32_t nH, uint32_t* __restrict__ wave_cnt, uint64_t* __restrict__ wave_max_,
                                                                 uint32_t* __restrict__ wave_host, uint32_t* __restrict__ wave_any) {
  const uint32_t i = blockIdx.x * kDlThreads + threadIdx.x, lane = threadIdx.x & 63u;
  bool row = false;
  uint32_t any = 0, host = lo + i;
  uint64_t d = 0;
  if (i < nH) {
    const DlAcc a = acc[i];
    row = dg_row(a, len[i]);
    any = (a.nd | a.nx) ? 1u : 0u;
    d = a.mx;
  }
  const uint64_t m = __ballot(row);
#pragma unroll
  for (uint32_t x = 1; x < 64; x <<= 1) {
    const uint32_t any2 = __shfl_xor(any, x), host2 = __shfl_xor(host, x);
    const uint64_t d2 = __shfl_xor(d, x);
    argmax_fold(any, d, host, any2, d2, host2);
  }
  if (lane == 0 && i < nH) {
    wave_cnt[i >> 6] = (uint32_t)__popcll(m);
    wave_max_[i >> 6] = d;
    wave_host[i >> 6] = host;
    wave_any[i >> 6] = any;
  }
}

__global__ __launch_bounds__(kScanThreads) void k_delay_rows_scan(const uint32_t* __restrict__ wave_cnt, const uint64_t* __restrict__ wave_max_,
                                                                  const uint32_t* __restrict__ wave_host, const uint32_t* __restrict__ wave_any,
                                                                  uint32_t nW, uint32_t* __restrict__ wave_off, DgHdr* __restrict__ hdr) {
  __shared__ uint64_t s_d[kScanThreads];
  __shared__ uint32_t s_h[kScanThreads], s_a[kScanThreads];
  uint32_t any = 0, host = 0;
  uint64_t d = 0;
  const uint32_t rows = tiled_scan<uint32_t>(
      nW,
      [&](uint32_t j) {
        argmax_fold(any, d, host, wave_any[j], wave_max_[j], wave_host[j]);
        return wave_cnt[j];
      },
      [&](uint32_t j, uint32_t before, uint32_t) { wave_off[j] = before; });
  s_d[threadIdx.x] = d;
  s_h[threadIdx.x] = host;
  s_a[threadIdx.x] = any;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t t = 1; t < kScanThreads; t++) argmax_fold(any, d, host, s_a[t], s_d[t], s_h[t]);
    hdr->rows = rows;
    hdr->max = any ? d : 0;
    hdr->max_host = any ? host : 0;
    hdr->max_any = any;
  }
}

__global__ __launch_bounds__(kDlThreads) void k_delay_rows_scatter(const DlAcc* __restrict__ acc, const uint64_t* __restrict__ len,
                                                                   const uint64_t* __restrict__ off, const DlEnt* __restrict__ carry,
                                                                   uint64_t n_carry, uint32_t lo, uint32_t nH,
                                                                   const uint32_t* __restrict__ wave_off, sgn_delay_row* __restrict__ rows,
                                                                   uint64_t cap, DgHdr* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * kDlThreads + threadIdx.x, lane = threadIdx.x & 63u;
  uint64_t t[kGetTotals];
#pragma unroll
  for (uint32_t k = 0; k < kGetTotals; k++) t[k] = 0;
  bool row = false;
  DlAcc a{};
  uint64_t m_len = 0;
  if (i < nH) {
    a = acc[i];
    m_len = len[i];
    row = dg_row(a, m_len);
  }
  const uint64_t m = __ballot(row);
  if (m == 0) return;  // (the whole wave)
  if (row) {
    t[0] = a.nd;
    t[1] = a.nx;
    t[2] = a.sd;
    t[3] = a.sx;
    t[4] = m_len;
    t[5] = a.um;
    if (rows) {
      uint64_t oldest = INVALID;
      if (m_len && off[i] < n_carry) oldest = carry[off[i]].t;
      const uint64_t j = (uint64_t)wave_off[i >> 6] + rank_below(m, lane);
      if (j < cap) {
        u64x2* p = (u64x2*)(rows + j);
        p[0] = u64x2{(uint64_t)(lo + i), (uint64_t)(uint32_t)m_len | (uint64_t)(uint32_t)a.um << 32};
        p[1] = u64x2{a.nd, a.nx};
        p[2] = u64x2{a.sd, a.sx};
        p[3] = u64x2{a.mx, oldest};
      } else {
        report_fail(&hdr->err, &hdr->err_host, 1u, lo + i);
      }
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kGetTotals; k++) {
    const uint64_t s = wave_sum(t[k]);
    if (lane == 0 && s) atomicAdd((unsigned long long*)&hdr->total[k], (unsigned long long)s);
  }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
namespace {

// what the report keeps for its lifetime, sized by the owned hosts
struct DlLay {
  size_t hdr, tot, ghdr, acc, len[2], off[2], pops, exits, wcnt, woff, wmax, whost, wany, bytes;
};
DlLay dl_lay(uint32_t nH) {
  const size_t nW = ((size_t)nH + 63) / 64;
  ScratchLay s;
  DlLay l;
  l.hdr = s.take(sizeof(DlHdr), 128);
  l.tot = s.take(sizeof(DlTot), 128);
  l.ghdr = s.take(sizeof(DgHdr), 128);
  l.acc = s.take((size_t)nH * sizeof(DlAcc), 128);
  for (int k = 0; k < 2; k++) l.len[k] = s.take((size_t)nH * 8, 128);
  for (int k = 0; k < 2; k++) l.off[k] = s.take((size_t)nH * 8, 128);
  l.pops = s.take((size_t)nH * 8, 128);
  l.exits = s.take((size_t)nH * 8, 8);  // (pops and exits adjacent: one memset to zero)
  l.wcnt = s.take(nW * 4, 128);
  l.woff = s.take(nW * 4, 128);
  l.wmax = s.take(nW * 8, 128);
  l.whost = s.take(nW * 4, 128);
  l.wany = s.take(nW * 4, 128);
  l.bytes = s.take(0, 128);
  return l;
}
// the scratch of one fold: a delta row and a list place per span, a pop index per record
struct DfLay {
  size_t delta, big, popidx, bytes;
};
DfLay df_lay(uint64_t n_spans, uint64_t n) {
  ScratchLay s;
  DfLay l;
  l.delta = s.take((size_t)n_spans * sizeof(DlAcc), 128);
  l.big = s.take((size_t)n_spans * 4, 128);
  l.popidx = s.take((size_t)n * 8, 128);
  l.bytes = s.take(0, 128);
  return l;
}

}  // namespace

struct sgn::DelayState {
  uint32_t lo = 0, nH = 0;
  DlLay L{};
  char* mem = nullptr;
  DlEnt* carry[2] = {nullptr, nullptr};  // cur: the carry; the other: the next fold's target
  uint64_t carry_cap[2] = {0, 0};
  uint64_t carry_n = 0;
  int cur = 0;
  void* fold_mem = nullptr;
  size_t fold_bytes = 0;
  void* rows_mem = nullptr;
  uint64_t rows_cap = 0;
  uint64_t pos = 0;  // the trace position folded up to
  uint64_t folds = 0, records = 0, rounds = 0, ws = 0, we = 0;
  ReportEvents<8> ev;
  // between prepare and commit
  bool pending = false;
  DelayFoldIn pend{};
  uint64_t pend_total = 0;
  sgn_delay_timing pend_timing{};

  uint64_t* len(int k) const { return (uint64_t*)(mem + L.len[k]); }
  uint64_t* off(int k) const { return (uint64_t*)(mem + L.off[k]); }
  ~DelayState() {
    if (mem) (void)hipFree(mem);
    for (DlEnt* c : carry)
      if (c) (void)hipFree(c);
    if (fold_mem) (void)hipFree(fold_mem);
    if (rows_mem) (void)hipFree(rows_mem);
  }
};

namespace {

sgn_delay_timing timing_zero() {
  sgn_delay_timing t{};
  t.wave_max = kDlWave;
  t.tile = kDlTile;
  return t;
}

int dl_bad(sgn_ctx* ctx, const char* what, const DlHdr& h) {
  const uint32_t bit = h.err & (0u - h.err);  // the lowest error bit
  const char* why = bit == DL_EMANY    ? "more exits than packets popped into the router: host "
                    : bit == DL_EORDER ? "an exit before its pop: host "
                    : bit == DL_EPAIR  ? "an exit and its pop disagree in (peer, c), or the exit is the earlier: host "
                                       : "a span or a carry place outside its buffer: host ";
  const uint32_t host = h.err_host[__builtin_ctz(bit)];
  return set_error(ctx, SGN_EDEVICE, std::string(what) + ": " + why + std::to_string(host) + " (nothing was folded)");
}

// the other carry buffer, large enough for n entries (the current one is untouched)
int carry_ensure(sgn_ctx* ctx, DelayState* st, uint64_t n, const char* what) {
  const int o = st->cur ^ 1;
  if (st->carry_cap[o] >= n) return 0;
  const uint64_t cap = std::max<uint64_t>(n + n / 2, 1024);
  void* p = nullptr;
  if (hipMalloc(&p, cap * sizeof(DlEnt)) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(ctx, SGN_ENOMEM, std::string("device allocation failed (") + what + ": the carry)");
  }
  if (st->carry[o]) (void)hipFree(st->carry[o]);
  st->carry[o] = (DlEnt*)p;
  st->carry_cap[o] = cap;
  return 0;
}

// a new report for hosts [lo, lo + nH): everything zero, an empty carry
int state_make(sgn_ctx* ctx, uint32_t lo, uint32_t nH, const char* what, DelayState** out) {
  *out = nullptr;
  DelayState* st = new DelayState;
  st->lo = lo;
  st->nH = nH;
  st->L = dl_lay(nH);
  if (hipMalloc((void**)&st->mem, st->L.bytes) != hipSuccess) {
    (void)hipGetLastError();
    st->mem = nullptr;
    delete st;
    return set_error(ctx, SGN_ENOMEM, std::string("device allocation failed (") + what + ")");
  }
  if (!st->ev.make() || hipMemsetAsync(st->mem, 0, st->L.bytes, ctx->stream) != hipSuccess) {
    delete st;
    return set_error(ctx, SGN_EDEVICE, std::string("hipEventCreate failed (") + what + ")");
  }
  *out = st;
  return 0;
}

// the carry from the per-host counts in `pops` (already on the device): so many unknown entries
int state_seed(sgn_ctx* ctx, DelayState* st, const char* what) {
  const DlLay& L = st->L;
  hipStream_t s = ctx->stream;
  DlHdr* d_hdr = (DlHdr*)(st->mem + L.hdr);
  const int o = st->cur ^ 1;
  hipLaunchKernelGGL(k_delay_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint64_t*)st->len(st->cur),
                     (const unsigned long long*)(st->mem + L.pops), (const unsigned long long*)(st->mem + L.exits), st->lo, st->nH,
                     st->len(o), st->off(o), d_hdr);
  DlHdr h{};
  if (int rc = read_header(ctx, d_hdr, &h)) return rc;
  if (h.err) return dl_bad(ctx, what, h);
  if (int rc = carry_ensure(ctx, st, h.carry_total, what)) return rc;
  if (h.carry_total && st->nH)
    hipLaunchKernelGGL(k_delay_fill, dim3((st->nH + kDlThreads - 1) / kDlThreads), dim3(kDlThreads), 0, s, (const uint64_t*)st->len(o),
                       (const uint64_t*)st->off(o), st->nH, st->carry[o], h.carry_total);
  SGN_HIP(ctx, hipGetLastError());
  SGN_HIP(ctx, hipStreamSynchronize(s));
  st->cur = o;
  st->carry_n = h.carry_total;
  return 0;
}

int state_get(sgn_ctx* ctx, DelayState* st, const char* what, sgn_delay_row* out, uint64_t cap, uint64_t* n_out, sgn_delay_info* info) {
  const DlLay& L = st->L;
  char* m = st->mem;
  hipStream_t s = ctx->stream;
  const uint32_t nH = st->nH, nW = (nH + 63) / 64, blocks = (nH + kDlThreads - 1) / kDlThreads;
  DgHdr* d_g = (DgHdr*)(m + L.ghdr);
  const DlAcc* d_acc = (const DlAcc*)(m + L.acc);
  DgHdr g{};
  if (nH) {
    SGN_HIP(ctx, hipMemsetAsync(d_g, 0, sizeof(DgHdr), s));
    hipLaunchKernelGGL(k_delay_rows_count, dim3(blocks), dim3(kDlThreads), 0, s, d_acc, (const uint64_t*)st->len(st->cur), st->lo, nH,
                       (uint32_t*)(m + L.wcnt), (uint64_t*)(m + L.wmax), (uint32_t*)(m + L.whost), (uint32_t*)(m + L.wany));
    hipLaunchKernelGGL(k_delay_rows_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint32_t*)(m + L.wcnt), (const uint64_t*)(m + L.wmax),
                       (const uint32_t*)(m + L.whost), (const uint32_t*)(m + L.wany), nW, (uint32_t*)(m + L.woff), d_g);
    if (int rc = read_header(ctx, d_g, &g)) return rc;
    if (g.rows > nH) return set_error(ctx, SGN_EDEVICE, std::string(what) + ": the wave counts add up to more rows than hosts");
  }
  const uint64_t rows = g.rows;
  const bool want_rows = out && cap >= rows;  // (the row total against the caller's capacity, before the scatter)
  if (want_rows && rows > st->rows_cap) {
    void* p = nullptr;
    if (hipMalloc(&p, rows * sizeof(sgn_delay_row)) != hipSuccess) {
      (void)hipGetLastError();
      return set_error(ctx, SGN_ENOMEM, std::string("device allocation failed (") + what + ": the rows)");
    }
    if (st->rows_mem) (void)hipFree(st->rows_mem);
    st->rows_mem = p;
    st->rows_cap = rows;
  }
  if (rows) {
    hipLaunchKernelGGL(k_delay_rows_scatter, dim3(blocks), dim3(kDlThreads), 0, s, d_acc, (const uint64_t*)st->len(st->cur),
                       (const uint64_t*)st->off(st->cur), (const DlEnt*)st->carry[st->cur], st->carry_n, st->lo, nH,
                       (const uint32_t*)(m + L.woff), want_rows ? (sgn_delay_row*)st->rows_mem : (sgn_delay_row*)nullptr, rows, d_g);
    if (int rc = read_header(ctx, d_g, &g)) return rc;
    if (g.err) return set_error(ctx, SGN_EDEVICE, std::string(what) + ": a row outside the row buffer: host " + std::to_string(g.err_host));
  }
  sgn_delay_info in{};
  in.rounds = st->rounds;
  in.window_start = st->ws;
  in.window_end = st->we;
  in.folds = st->folds;
  in.records = st->records;
  in.hosts = nH;
  in.rows = rows;
  for (uint32_t k = 0; k < kGetTotals; k++) in.total[k] = g.total[k];
  in.delay_max = g.max;
  in.delay_max_host = g.max_host;
  DlTot tot{};
  SGN_HIP(ctx, hipMemcpyAsync(&tot, m + L.tot, sizeof(DlTot), hipMemcpyDeviceToHost, s));
  SGN_HIP(ctx, hipStreamSynchronize(s));
  for (uint32_t k = 0; k < kBins; k++) {
    in.hist_delivered[k] = tot.hist[0][k];
    in.hist_dropped[k] = tot.hist[1][k];
  }
  if (info) *info = in;
  if (n_out) *n_out = rows;
  if (out && cap < rows)
    return set_error(ctx, SGN_ERANGE, std::string(what) + ": " + std::to_string(rows) + " hosts have a row, the caller's array holds " +
                                          std::to_string(cap) + " (nothing was written to it)");
  if (want_rows && rows) {
    SGN_HIP(ctx, hipMemcpyAsync(out, st->rows_mem, rows * sizeof(sgn_delay_row), hipMemcpyDeviceToHost, s));
    SGN_HIP(ctx, hipStreamSynchronize(s));
  }
  return 0;
}

int state_clear(sgn_ctx* ctx, DelayState* st) {
  SGN_HIP(ctx, hipMemsetAsync(st->mem + st->L.tot, 0, sizeof(DlTot), ctx->stream));
  SGN_HIP(ctx, hipMemsetAsync(st->mem + st->L.acc, 0, (size_t)st->nH * sizeof(DlAcc), ctx->stream));
  SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  st->folds = st->records = 0;
  return 0;
}

}  // namespace

namespace sgn {

int delay_fold_prepare(sgn_ctx* ctx, DelayState* st, const DelayFoldIn& in, const char* what) {
  st->pending = false;
  if (in.lo != st->lo || in.nH != st->nH) return set_error(ctx, SGN_ESTATE, std::string(what) + ": the report was enabled for other hosts");
  const DlLay& L = st->L;
  char* m = st->mem;
  hipStream_t s = ctx->stream;
  const DfLay F = df_lay(in.n_spans, in.n);
  if (st->fold_bytes < F.bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, F.bytes) != hipSuccess) {
      (void)hipGetLastError();
      return set_error(ctx, SGN_ENOMEM, std::string("device allocation failed (") + what + ": the fold's scratch)");
    }
    if (st->fold_mem) (void)hipFree(st->fold_mem);
    st->fold_mem = p;
    st->fold_bytes = F.bytes;
  }
  char* f = (char*)st->fold_mem;
  DlHdr* d_hdr = (DlHdr*)(m + L.hdr);
  unsigned long long* d_pops = (unsigned long long*)(m + L.pops);
  unsigned long long* d_exits = (unsigned long long*)(m + L.exits);
  uint32_t* d_big = (uint32_t*)(f + F.big);
  const int c = st->cur, o = c ^ 1;
  const ReportEvents<8>& E = st->ev;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(kDlMaxBlocks, (in.n + kDlThreads - 1) / kDlThreads);

  DlHdr h0{};
  for (uint32_t& e : h0.err_host) e = 0xFFFFFFFFu;
  SGN_HIP(ctx, hipMemcpyAsync(d_hdr, &h0, sizeof(DlHdr), hipMemcpyHostToDevice, s));
  SGN_HIP(ctx, hipMemsetAsync(d_pops, 0, L.exits + (size_t)st->nH * 8 - L.pops, s));  // pops, exits
  (void)hipEventRecord(E[0], s);
  hipLaunchKernelGGL(k_delay_count, dim3(blocks), dim3(kDlThreads), 0, s, in.staging, in.n, in.spans, in.n_spans, st->lo, st->nH, d_pops,
                     d_exits, d_big, d_hdr);
  (void)hipEventRecord(E[1], s);
  hipLaunchKernelGGL(k_delay_scan, dim3(1), dim3(kScanThreads), 0, s, (const uint64_t*)st->len(c), (const unsigned long long*)d_pops,
                     (const unsigned long long*)d_exits, st->lo, st->nH, st->len(o), st->off(o), d_hdr);
  (void)hipEventRecord(E[2], s);
  DlHdr h{};
  if (int rc = read_header(ctx, d_hdr, &h)) return rc;
  if (h.err) return dl_bad(ctx, what, h);
  if (h.n_big > in.n_spans || h.largest > in.n)
    return set_error(ctx, SGN_EDEVICE, std::string(what) + ": the span classes do not add up (nothing was folded)");
  if (int rc = carry_ensure(ctx, st, h.carry_total, what)) return rc;  // (the size is known before anything is written)
  DlBufs B;
  B.recs = in.staging;
  B.n = in.n;
  B.spans = in.spans;
  B.len_old = st->len(c);
  B.off_old = st->off(c);
  B.len_new = st->len(o);
  B.off_new = st->off(o);
  B.exits = d_exits;
  B.carry_old = st->carry[c];
  B.carry_new = st->carry[o];
  B.n_old = st->carry_n;
  B.n_new = h.carry_total;
  B.delta = (DlAcc*)(f + F.delta);
  B.lo = st->lo;
  B.nH = st->nH;
  (void)hipEventRecord(E[3], s);
  if (st->carry_n)
    hipLaunchKernelGGL(k_delay_keep, dim3((uint32_t)std::min<uint64_t>(kDlMaxBlocks, (st->carry_n + kDlThreads - 1) / kDlThreads)),
                       dim3(kDlThreads), 0, s, (const DlEnt*)st->carry[c], st->carry_n, (const unsigned long long*)d_exits,
                       (const uint64_t*)st->off(c), (const uint64_t*)st->len(o), (const uint64_t*)st->off(o), st->lo, st->nH,
                       st->carry[o], h.carry_total, d_hdr);
  (void)hipEventRecord(E[4], s);
  if (in.n_spans > h.n_big) {
    const uint64_t wave_blocks = std::min<uint64_t>((in.n_spans + kDlThreads / 64 - 1) / (kDlThreads / 64), 1u << 16);
    hipLaunchKernelGGL(k_delay_match_wave, dim3((uint32_t)wave_blocks), dim3(kDlThreads), 0, s, B, in.n_spans, d_hdr);
  }
  if (h.n_big)
    hipLaunchKernelGGL(k_delay_match_walk, dim3(std::min<uint32_t>(h.n_big, 1u << 16)), dim3(kDlTile), 0, s, B, (const uint32_t*)d_big,
                       h.n_big, (uint64_t*)(f + F.popidx), d_hdr);
  (void)hipEventRecord(E[5], s);
  if (int rc = read_header(ctx, d_hdr, &h)) return rc;
  if (h.err) return dl_bad(ctx, what, h);
  st->pending = true;
  st->pend = in;
  st->pend_total = h.carry_total;
  sgn_delay_timing T = timing_zero();
  T.records = in.n;
  T.hosts = in.n_spans;
  T.largest_span = h.largest;
  T.carry_entries = h.carry_total;
  T.spans_by_class[0] = in.n_spans - h.n_big;
  T.spans_by_class[1] = h.n_big;
  st->pend_timing = T;
  return 0;
}

int delay_fold_commit(sgn_ctx* ctx, DelayState* st, uint64_t n_records) {
  if (!st->pending) return set_error(ctx, SGN_ESTATE, "the delay report has no prepared fold");
  st->pending = false;
  const DlLay& L = st->L;
  const DelayFoldIn& in = st->pend;
  hipStream_t s = ctx->stream;
  const ReportEvents<8>& E = st->ev;
  const DfLay F = df_lay(in.n_spans, in.n);
  (void)hipEventRecord(E[6], s);
  hipLaunchKernelGGL(k_delay_commit, dim3((uint32_t)std::min<uint64_t>(kDlMaxBlocks, (in.n_spans + kDlThreads - 1) / kDlThreads + 1)),
                     dim3(kDlThreads), 0, s, in.spans, in.n_spans, (const DlAcc*)((char*)st->fold_mem + F.delta), st->lo, st->nH,
                     (DlAcc*)(st->mem + L.acc), (const DlHdr*)(st->mem + L.hdr), (DlTot*)(st->mem + L.tot));
  (void)hipEventRecord(E[7], s);
  SGN_HIP(ctx, hipGetLastError());
  SGN_HIP(ctx, hipStreamSynchronize(s));
  st->cur ^= 1;
  st->carry_n = st->pend_total;
  st->records += n_records;
  sgn_delay_timing& T = st->pend_timing;
  T.kernel_ms[0] = elapsed_ms(E[0], E[1]);
  T.kernel_ms[1] = elapsed_ms(E[1], E[2]);
  T.kernel_ms[2] = elapsed_ms(E[3], E[4]);
  T.kernel_ms[3] = elapsed_ms(E[4], E[5]);
  T.kernel_ms[4] = elapsed_ms(E[6], E[7]);
  ctx->dl_timing = T;
  return 0;
}

int delay_position_check(sgn_ctx* ctx, const char* what) {
  if (ctx->dl->pos == ctx->trace_base) return 0;
  return set_error(ctx, SGN_ESTATE, std::string(what) + ": the delay report has folded the trace up to record " +
                                        std::to_string(ctx->dl->pos) + ", the context has taken " + std::to_string(ctx->trace_base) +
                                        " (a restore moved it: sgn_delay_enable starts the report again; nothing changed)");
}

void delay_position_set(sgn_ctx* ctx, uint64_t pos, bool folded) {
  DelayState* st = ctx->dl;
  st->pos = pos;
  if (!folded) return;
  st->folds++;
  st->rounds = ctx->h_ctrl->rounds;
  st->ws = ctx->h_ctrl->ws;
  st->we = ctx->h_ctrl->we;
}

void delay_release(sgn_ctx* ctx) {
  delete ctx->dl;
  ctx->dl = nullptr;
  ctx->dl_timing = timing_zero();
}

}  // namespace sgn

extern "C" {

int sgn_delay_enable(sgn_ctx* ctx) {
  if (!ctx) return SGN_EINVAL;
  const char* what = "sgn_delay_enable";
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (!ctx->trace_buf) return set_error(ctx, SGN_ESTATE, std::string(what) + ": the simulation keeps no trace (sgn_trace_enable)");
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = sync_ctrl(ctx)) return rc;
  if (ctx->h_ctrl->trace_n != ctx->trace_base)
    return set_error(ctx, SGN_ESTATE, std::string(what) + ": trace records are pending (take them first: the record stream and the "
                                                          "device state then meet at one round edge)");
  const DevSim& S = ctx->S;
  DelayState* st = nullptr;
  if (int rc = state_make(ctx, S.lo, S.nH, what, &st)) return rc;
  // what stands at every traced host's router now, as unknown entries
  DlHdr h0{};
  for (uint32_t& e : h0.err_host) e = 0xFFFFFFFFu;
  uint32_t* d_traced = nullptr;
  std::vector<uint32_t> traced;
  int rc = 0;
  if (!ctx->trace_hosts.empty() && S.nH) {
    traced.assign(S.nH, 0u);
    for (uint32_t h : ctx->trace_hosts)
      if (h >= S.lo && h - S.lo < S.nH) traced[h - S.lo] = 1u;
    if (hipMalloc((void**)&d_traced, (size_t)S.nH * 4) != hipSuccess) {
      (void)hipGetLastError();
      d_traced = nullptr;
      rc = set_error(ctx, SGN_ENOMEM, std::string("device allocation failed (") + what + ")");
    } else if (hipMemcpyAsync(d_traced, traced.data(), (size_t)S.nH * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
      rc = set_error(ctx, SGN_EDEVICE, std::string(what) + ": the upload of the traced hosts failed");
    }
  }
  if (!rc && hipMemcpyAsync(st->mem + st->L.hdr, &h0, sizeof(DlHdr), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    rc = set_error(ctx, SGN_EDEVICE, std::string(what) + ": the upload of the header failed");
  if (!rc && S.nH)
    hipLaunchKernelGGL(k_delay_standing, dim3((S.nH + kDlThreads - 1) / kDlThreads), dim3(kDlThreads), 0, ctx->stream, bk_args(ctx),
                       (const uint32_t*)d_traced, (unsigned long long*)(st->mem + st->L.pops), (DlHdr*)(st->mem + st->L.hdr));
  if (!rc) rc = state_seed(ctx, st, what);  // (the stream is idle afterwards)
  if (rc) (void)hipStreamSynchronize(ctx->stream);
  if (d_traced) (void)hipFree(d_traced);
  if (rc) {
    delete st;
    return rc;
  }
  delete ctx->dl;
  ctx->dl = st;
  ctx->dl_timing = timing_zero();
  st->pos = ctx->trace_base;
  st->rounds = ctx->h_ctrl->rounds;
  st->ws = ctx->h_ctrl->ws;
  st->we = ctx->h_ctrl->we;
  return 0;
}

int sgn_delay_fold(sgn_ctx* ctx, sgn_delay_info* out) {
  if (!ctx) return SGN_EINVAL;
  const auto t_begin = std::chrono::steady_clock::now();
  if (int rc = trace_take_common(ctx, "sgn_delay_fold", true, nullptr, 0, nullptr, nullptr, 0, nullptr)) return rc;
  if (out)
    if (int rc = state_get(ctx, ctx->dl, "sgn_delay_fold", nullptr, 0, nullptr, out)) return rc;
  ctx->dl_timing.total_ms = ms_since(t_begin);
  return 0;
}

int sgn_delay_get(sgn_ctx* ctx, sgn_delay_row* out, uint64_t cap, uint64_t* n_out, sgn_delay_info* info) {
  if (n_out) *n_out = 0;
  if (!ctx) return SGN_EINVAL;
  if (!n_out || !info || (!out && cap)) return set_error(ctx, SGN_EINVAL, "sgn_delay_get: null argument");
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (!ctx->dl) return set_error(ctx, SGN_ESTATE, "sgn_delay_get: the report is not enabled (sgn_delay_enable)");
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  return state_get(ctx, ctx->dl, "sgn_delay_get", out, cap, n_out, info);
}

int sgn_delay_clear(sgn_ctx* ctx) {
  if (!ctx) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (!ctx->dl) return set_error(ctx, SGN_ESTATE, "sgn_delay_clear: the report is not enabled (sgn_delay_enable)");
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  return state_clear(ctx, ctx->dl);
}

int sgn_delay_timing_get(sgn_ctx* ctx, sgn_delay_timing* out) {
  if (!ctx || !out) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_delay_timing_get: null argument") : SGN_EINVAL;
  *out = ctx->dl_timing;
  out->wave_max = kDlWave;
  out->tile = kDlTile;
  return 0;
}

int sgn_selftest_delay_fold(sgn_ctx* ctx, const sgn_trace_rec* recs, const uint64_t* piece_ends, uint32_t n_pieces, uint32_t host_lo,
                            uint32_t n_hosts, const uint32_t* standing0, sgn_delay_row* rows, uint64_t cap, uint64_t* n_rows,
                            sgn_delay_info* info) {
  if (n_rows) *n_rows = 0;
  if (!ctx) return SGN_EINVAL;
  const char* what = "sgn_selftest_delay_fold";
  if (!n_rows || !info || (!rows && cap) || (n_pieces && !piece_ends) || (n_pieces && piece_ends[n_pieces - 1] && !recs))
    return set_error(ctx, SGN_EINVAL, std::string(what) + ": null argument");
  for (uint32_t i = 1; i < n_pieces; i++)
    if (piece_ends[i] < piece_ends[i - 1]) return set_error(ctx, SGN_EINVAL, std::string(what) + ": piece_ends must ascend");
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  ctx->dl_timing = timing_zero();
  DelayState* st = nullptr;
  if (int rc = state_make(ctx, host_lo, n_hosts, what, &st)) return rc;
  int rc = 0;
  if (standing0 && n_hosts) {
    const std::vector<unsigned long long> p(standing0, standing0 + n_hosts);
    DlHdr h0{};
    for (uint32_t& e : h0.err_host) e = 0xFFFFFFFFu;
    if (hipMemcpyAsync(st->mem + st->L.pops, p.data(), (size_t)n_hosts * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(st->mem + st->L.hdr, &h0, sizeof(DlHdr), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
      rc = set_error(ctx, SGN_EDEVICE, std::string(what) + ": the upload of standing0 failed");
    if (!rc) rc = state_seed(ctx, st, what);  // (the stream is idle afterwards: p may go)
    if (rc) (void)hipStreamSynchronize(ctx->stream);
  }
  uint64_t from = 0;
  for (uint32_t i = 0; i < n_pieces && !rc; i++) {
    const uint64_t n = piece_ends[i] - from;
    if (n) {
      rc = take_upload(ctx, what, recs + from, n, n_hosts);
      if (!rc) rc = take_run(ctx, what, nullptr, n, n, host_lo, n_hosts, true, nullptr, 0, nullptr, nullptr, 0, nullptr, st);
    }
    st->folds++;
    from = piece_ends[i];
  }
  if (!rc) rc = state_get(ctx, st, what, rows, cap, n_rows, info);
  delete st;
  return rc;
}

}  // extern "C"

uint64_t sgn::layout_sig_delay() { return kLayoutSig; }
