// backlog.hip — the backlog report: per-host standing queues and in-flight packets (sgn_backlog).
//
// What stands in the network at a round edge is already in device memory and final at every launch
// boundary: the CoDel queue's length, bytes and head run and the send queue's ring position in the
// host record, the head run's enqueue time in the CoDel page pool, the queued trains in the send
// ring, the packets in flight in the event calendar. The report reads them in four launches on
// the context's stream — the count / scan / scatter shape of sample.hip behind a calendar pass:
//   1. k_backlog_calendar  one workgroup per host group (the hosts_per_wave consecutive slots that
//                          share the group's slabs): its waves walk the group's slab of every
//                          bucket, pool part and extension part, and accumulate per destination
//                          slot packets, submitted datagrams, earliest and latest delivery time in
//                          LDS (ds add / min / max); one 32-byte line per slot goes to scratch;
//   2. k_backlog_count     one lane per owned HostId (sid_of -> slot): the queues' bookkeeping and
//                          the slot's calendar line decide "has a row"; ballot, one count per wave,
//                          and the wave's candidates for the two maxima;
//   3. k_backlog_scan      one workgroup: an exclusive scan of the wave counts, the row total, and
//                          the fold of the waves' maxima (ascending, so ties keep the lowest
//                          HostId); the host checks the row total against the caller's capacity;
//   4. k_backlog_scatter   the same flags again; a host with a row walks its send ring, joins the
//                          calendar line and stores the row as four 16-byte stores; the eight
//                          totals are summed over the wave and added with one 64-bit atomic per
//                          wave and total.
// Nothing of the round path is touched: the kernels read the simulation's buffers and write only
// the report's scratch. Every index that comes out of a buffer (a fill word, an extension word, a
// bucket's slab id, a run's destination, a queue head) is bounded before it is used; a word that
// points outside is recorded in the header (error bit, first offender) and skipped.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "backlog_read.h"
#include "report_common.h"
#include "sgn_workload.h"

using namespace sgn;
using namespace sgn::report;  // the scan (kScanTile = 1024 waves a tile), the wave reductions, the host scaffolding
using namespace sgn::backlog_read;  // BkArgs, BkHost, bk_load, bk_args: shared with delay.hip

// ---- device side ----------------------------------------------------------------------------
namespace {

constexpr uint32_t kCalThreads = 256;      // k_backlog_calendar: four waves, a bucket each
constexpr uint32_t kBkThreads = 256;       // k_backlog_count, _scatter: one lane per host
constexpr uint32_t kTotals = 8;
constexpr uint64_t kStageRows = 1u << 16;  // rows per piece of the device-to-host copy (4 MB)

static_assert(sizeof(sgn_backlog_row) == 64 && offsetof(sgn_backlog_row, router_bytes) == 16 &&
                  offsetof(sgn_backlog_row, router_oldest) == 32 && offsetof(sgn_backlog_row, inflight_earliest) == 48,
              "a row is four 16-byte stores: {host | flags, router | send packets}, {router, send bytes}, "
              "{router_oldest, inflight | submit}, {earliest, latest}");
static_assert(sizeof(sgn_backlog_info) == 144, "");
static_assert(INVALID == ~0ull, "an empty minimum is INVALID");

enum : uint32_t {
  BK_ESLOT = 1u,   // a host's slot lies outside the shard (nothing of it was read)
  BK_ESLAB = 2u,   // a bucket's slab id, a fill word or an extension word points outside the calendar
  BK_EDST = 4u,    // a run's destination is not a slot of the group whose slab holds it
  BK_EQUEUE = 8u,  // a queue head or length outside its pool / ring
  BK_EROW = 16u,   // the scatter met a row outside the row buffer (skipped)
};
struct __attribute__((aligned(16))) BkHdr {
  uint64_t rows;               // k_backlog_scan: hosts with a row
  uint32_t err, pad0;          // BK_E*
  uint64_t err_info;           // the first offender: a slab index (BK_ESLAB, BK_EDST) or a HostId
  uint64_t total[kTotals];     // k_backlog_scatter: sgn_backlog_info::total
  uint64_t max_router;         // k_backlog_scan: the largest CoDel queue, and its host
  uint64_t min_oldest;         // ... the oldest head of any CoDel queue (INVALID: none), and its host
  uint32_t max_router_host, min_oldest_host;
  uint64_t inflight_earliest;  // k_backlog_scatter (atomic min; k_backlog_scan sets INVALID)
  uint64_t calendar_runs;      // k_backlog_calendar: runs read
};
static_assert(sizeof(BkHdr) == 128, "");

// a slot's line of the calendar pass
struct __attribute__((aligned(16))) BkCal {
  uint32_t packets, submit;
  uint64_t earliest, latest;  // INVALID / 0 when packets == 0
  uint64_t pad;
};
static_assert(sizeof(BkCal) == 32, "");

// 1. the calendar pass. A group's pending runs are in its slab of each of the NB buckets (between
// rounds the spare slab set is empty): the workgroup's waves take the buckets in turn, a wave's
// lanes the slab's runs. A run addresses a slot of this group (the calendar is laid out by the
// destination's group); its packets are the high 16 bits of EvRec::pc. EXTERNAL traffic: a run
// whose source is its own destination is a datagram a CPU application submitted, waiting for the
// host to reach its send time — counted apart, not in flight.
__global__ __launch_bounds__(kCalThreads) void k_backlog_calendar(BkArgs a, BkCal* __restrict__ cal, BkHdr* __restrict__ hdr) {
  __shared__ uint32_t s_pk[GROUP_MAX], s_sub[GROUP_MAX];
  __shared__ uint64_t s_min[GROUP_MAX], s_max[GROUP_MAX];
  __shared__ uint32_t s_runs;
  const uint32_t g = blockIdx.x, gsz = 1u << a.gsh;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  if (threadIdx.x < GROUP_MAX) {
    s_pk[threadIdx.x] = s_sub[threadIdx.x] = 0;
    s_min[threadIdx.x] = INVALID;
    s_max[threadIdx.x] = 0;
  }
  if (threadIdx.x == 0) s_runs = 0;
  __syncthreads();
  const uint32_t slot0 = g << a.gsh;
  uint32_t runs = 0;
  for (uint32_t b = wv; b < a.NB; b += kCalThreads / 64) {
    const uint32_t sl = a.bucket_slab[b];
    if (sl > a.NB) {  // (NB + 1 slab sets)
      if (lane == 0) report_fail(&hdr->err, &hdr->err_info, BK_ESLAB, (uint64_t)b);
      continue;
    }
    const uint64_t idx = (uint64_t)sl * a.G + g;  // (< (NB + 1) * G: sl <= NB, g < G)
    const uint32_t fill = a.slab_n[idx];
    if (fill == 0) continue;
    const uint64_t x = a.ext && fill > a.CAP ? a.ext[idx] : 0ull;
    const uint32_t np = min(fill, a.CAP);
    uint32_t ne = min(fill - np, (uint32_t)(x >> 40));
    const uint64_t eo = x & EXT_OFF_MASK;
    // a fill above the slab's room (runs in the spill area: the host resolves them before the call)
    // or an extension outside its pool: reported; what lies inside the buffers is still read
    if (fill - np != ne || (ne && (eo > a.ext_total || ne > a.ext_total - eo))) {
      if (lane == 0) report_fail(&hdr->err, &hdr->err_info, BK_ESLAB, idx);
      if (ne && (eo > a.ext_total || ne > a.ext_total - eo)) ne = 0;
    }
    for (uint32_t j = lane; j < np + ne; j += 64) {
      const EvRec* e = j < np ? a.pool + idx * a.CAP + j : a.ext_pool + eo + (j - np);
      const u64x2 lo2 = *(const u64x2*)e, hi2 = *((const u64x2*)e + 1);  // {time, eid}, {src | dst << 32, pc | tag << 32}
      const uint64_t time = lo2.x;
      const uint32_t src = (uint32_t)hi2.x, dst = (uint32_t)(hi2.x >> 32), pc = (uint32_t)hi2.y;
      const uint32_t k = dst - a.lo - slot0;  // the slot within the group
      if (k >= gsz || slot0 + k >= a.nH) {
        report_fail(&hdr->err, &hdr->err_info, BK_EDST, idx);
        continue;
      }
      const uint32_t n = pc >> 16;
      if (a.tkind == SGN_TRAFFIC_EXTERNAL && src == a.host_of[slot0 + k]) {
        atomicAdd(&s_sub[k], n);
      } else {
        atomicAdd(&s_pk[k], n);
        atomicMin((unsigned long long*)&s_min[k], (unsigned long long)time);
        atomicMax((unsigned long long*)&s_max[k], (unsigned long long)time);
      }
    }
    runs += np + ne;  // (uniform over the wave)
  }
  if (lane == 0 && runs) atomicAdd(&s_runs, runs);
  __syncthreads();
  if (threadIdx.x < gsz && slot0 + threadIdx.x < a.nH) {
    u64x2* p = (u64x2*)(cal + slot0 + threadIdx.x);
    p[0] = u64x2{(uint64_t)s_pk[threadIdx.x] | (uint64_t)s_sub[threadIdx.x] << 32, s_min[threadIdx.x]};
    p[1] = u64x2{s_max[threadIdx.x], 0ull};
  }
  if (threadIdx.x == 0 && s_runs) atomicAdd((unsigned long long*)&hdr->calendar_runs, (unsigned long long)s_runs);
}

__device__ __forceinline__ bool bk_has_row(const BkHost& h, const BkCal& c) {
  return (h.flags | h.cq_len | h.fq_len | c.packets | c.submit) != 0 || h.cq_bytes != 0;
}
__device__ __forceinline__ BkCal bk_cal(const BkCal* cal, uint32_t slot) {
  const u64x2 p0 = *(const u64x2*)(cal + slot), p1 = *((const u64x2*)(cal + slot) + 1);
  BkCal c;
  c.packets = (uint32_t)p0.x;
  c.submit = (uint32_t)(p0.x >> 32);
  c.earliest = p0.y;
  c.latest = p1.x;
  c.pad = 0;
  return c;
}
// the enqueue time of the CoDel queue's head run; INVALID for an empty queue (or a head outside the pool)
__device__ __forceinline__ uint64_t bk_oldest(const BkArgs& a, const BkHost& h, uint32_t host, BkHdr* hdr) {
  if (h.cq_len == 0) return INVALID;
  if (h.cq_head >= (uint64_t)a.cq_pages * CQ_PAGE) {
    report_fail(&hdr->err, &hdr->err_info, BK_EQUEUE, host);
    return INVALID;
  }
  return a.codel[h.cq_head].enqueue_ts;
}

// 2. per wave (64 consecutive HostIds): the hosts with a row, the largest CoDel queue
// (packets << 32 | ~HostId: the maximum is the lowest HostId of the largest queue; 0: none) and
// the oldest queue head with its host
__global__ __launch_bounds__(kBkThreads) void k_backlog_count(BkArgs a, const BkCal* __restrict__ cal, uint32_t* __restrict__ wave_cnt,
                                                              uint64_t* __restrict__ wave_maxq, uint64_t* __restrict__ wave_old,
                                                              uint32_t* __restrict__ wave_old_host, BkHdr* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * kBkThreads + threadIdx.x, lane = threadIdx.x & 63u;
  bool row = false;
  uint64_t maxq = 0, old = INVALID;
  if (i < a.nH) {
    BkHost h;
    if (bk_load(a, i, &h)) {
      row = bk_has_row(h, bk_cal(cal, h.slot));
      if (h.cq_len) maxq = (uint64_t)h.cq_len << 32 | (uint32_t)~(a.lo + i);
      old = bk_oldest(a, h, a.lo + i, hdr);
    } else {
      report_fail(&hdr->err, &hdr->err_info, BK_ESLOT, a.lo + i);
    }
  }
  const uint64_t m = __ballot(row);
  uint32_t oh = a.lo + i;  // (lanes ascend by HostId: on equal times the lower lane's host stays)
  maxq = wave_max(maxq);
  wave_argmin(old, oh);
  if (lane == 0 && i < a.nH) {
    wave_cnt[i >> 6] = (uint32_t)__popcll(m);
    wave_maxq[i >> 6] = maxq;
    wave_old[i >> 6] = old;
    wave_old_host[i >> 6] = oh;
  }
}

// 3. one workgroup scans the nW wave counts (tiled_scan): wave_off[w] = hosts with a row in the waves
// before w; and folds the waves' maxima
__global__ __launch_bounds__(kScanThreads) void k_backlog_scan(const uint32_t* __restrict__ wave_cnt, const uint64_t* __restrict__ wave_maxq,
                                                               const uint64_t* __restrict__ wave_old,
                                                               const uint32_t* __restrict__ wave_old_host, uint32_t nW,
                                                               uint32_t* __restrict__ wave_off, BkHdr* __restrict__ hdr) {
  __shared__ uint64_t s_maxq[kScanThreads], s_old[kScanThreads];
  __shared__ uint32_t s_oh[kScanThreads];
  uint64_t maxq = 0, old = INVALID;
  uint32_t oh = 0xFFFFFFFFu;
  const uint32_t rows = tiled_scan<uint32_t>(
      nW,
      [&](uint32_t j) {
        const uint64_t mq = wave_maxq[j];
        maxq = mq > maxq ? mq : maxq;
        argmin_fold(old, oh, wave_old[j], wave_old_host[j]);
        return wave_cnt[j];
      },
      [&](uint32_t j, uint32_t before, uint32_t) { wave_off[j] = before; });
  s_maxq[threadIdx.x] = maxq;
  s_old[threadIdx.x] = old;
  s_oh[threadIdx.x] = oh;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t t = 1; t < kScanThreads; t++) {
      maxq = s_maxq[t] > maxq ? s_maxq[t] : maxq;
      argmin_fold(old, oh, s_old[t], s_oh[t]);
    }
    hdr->rows = rows;
    hdr->max_router = maxq >> 32;
    hdr->max_router_host = maxq ? ~(uint32_t)maxq : 0u;
    hdr->min_oldest = old;
    hdr->min_oldest_host = old != INVALID ? oh : 0u;
    hdr->inflight_earliest = INVALID;
  }
}

// 4. rows and totals. The flags are those of k_backlog_count (nothing ran in between), so every row
// lies in [0, hdr->rows); rows == null is the totals-only form. A row outside the buffer is skipped
// and reported, never stored.
__global__ __launch_bounds__(kBkThreads) void k_backlog_scatter(BkArgs a, const BkCal* __restrict__ cal, const uint32_t* __restrict__ wave_off,
                                                                sgn_backlog_row* __restrict__ rows, uint64_t cap, BkHdr* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * kBkThreads + threadIdx.x, lane = threadIdx.x & 63u;
  uint64_t t[kTotals];
#pragma unroll
  for (uint32_t k = 0; k < kTotals; k++) t[k] = 0;
  uint64_t earliest = INVALID;
  bool row = false;
  BkHost h{};
  BkCal c{};
  if (i < a.nH && bk_load(a, i, &h)) {
    c = bk_cal(cal, h.slot);
    row = bk_has_row(h, c);
  }
  const uint64_t m = __ballot(row);
  if (m == 0) return;  // (the whole wave: nothing to write, nothing to add)
  if (row) {
    const uint32_t host = a.lo + i;
    const uint64_t oldest = bk_oldest(a, h, host, hdr);
    // the send ring: fq_len entries from fq_head, wrapping at fifo_cap; an entry is a train of
    // `count` datagrams, all but the last of one payload size
    uint32_t sp = 0;
    uint64_t sb = 0;
    if (h.fq_len > a.fifo_cap || h.fq_head >= a.fifo_cap) {
      report_fail(&hdr->err, &hdr->err_info, BK_EQUEUE, host);
    } else {
      const FifoEnt* ring = a.fifo + (size_t)h.slot * a.fifo_cap;
      uint32_t idx = h.fq_head;
      for (uint32_t k = 0; k < h.fq_len; k++) {
        const uint4 v = *(const uint4*)(ring + idx);  // {dst, pay, count, tag}
        const uint64_t hb = sgn_header_bytes(v.w);
        if (v.z) {
          sp += v.z;
          sb += (uint64_t)(v.z - 1) * ((v.y & 0xFFFFu) + hb) + ((v.y >> 16) + hb);
        }
        idx = idx + 1 == a.fifo_cap ? 0 : idx + 1;
      }
    }
    t[0] = h.cq_len;
    t[1] = h.cq_bytes;
    t[2] = h.flags & SGN_BACKLOG_ROUTER_HELD ? 1 : 0;
    t[3] = sp;
    t[4] = sb;
    t[5] = h.flags & SGN_BACKLOG_OUT_HELD ? 1 : 0;
    t[6] = c.packets;
    t[7] = c.submit;
    earliest = c.packets ? c.earliest : INVALID;
    if (rows) {
      const uint64_t j = (uint64_t)wave_off[i >> 6] + rank_below(m, lane);
      if (j < cap) {
        u64x2* p = (u64x2*)(rows + j);
        p[0] = u64x2{(uint64_t)host | (uint64_t)h.flags << 32, (uint64_t)h.cq_len | (uint64_t)sp << 32};
        p[1] = u64x2{h.cq_bytes, sb};
        p[2] = u64x2{oldest, (uint64_t)c.packets | (uint64_t)c.submit << 32};
        p[3] = u64x2{earliest, c.packets ? c.latest : 0ull};
      } else {
        report_fail(&hdr->err, &hdr->err_info, BK_EROW, host);
      }
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kTotals; k++) {
    const uint64_t s = wave_sum(t[k]);
    if (lane == 0 && s) atomicAdd((unsigned long long*)&hdr->total[k], (unsigned long long)s);
  }
  earliest = wave_min(earliest);
  if (lane == 0 && earliest != INVALID) atomicMin((unsigned long long*)&hdr->inflight_earliest, (unsigned long long)earliest);
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
namespace {

// the scratch of a report: header, per-slot calendar lines, per-wave words, rows
struct BkLay {
  size_t hdr, cal, cnt, off, maxq, old, oldh, rows, bytes;
};
BkLay bk_lay(uint32_t nH) {
  const size_t nW = ((size_t)nH + 63) / 64;
  ScratchLay s;  // (every piece on a 128-byte line of its own)
  BkLay l;
  l.hdr = s.take(sizeof(BkHdr), 128);
  l.cal = s.take((size_t)nH * sizeof(BkCal), 128);
  l.cnt = s.take(nW * 4, 128);
  l.off = s.take(nW * 4, 128);
  l.maxq = s.take(nW * 8, 128);
  l.old = s.take(nW * 8, 128);
  l.oldh = s.take(nW * 4, 128);
  l.rows = s.take((size_t)nH * sizeof(sgn_backlog_row), 128);
  l.bytes = s.take(0, 128);
  return l;
}
size_t bk_stage_bytes(uint32_t nH) { return sizeof(BkHdr) + std::min<uint64_t>(std::max<uint32_t>(nH, 1u), kStageRows) * sizeof(sgn_backlog_row); }

int bk_bad(sgn_ctx* ctx, const BkHdr& h) {
  const char* why = h.err & BK_ESLOT    ? "a host's slot lies outside the shard: host "
                    : h.err & BK_ESLAB  ? "a calendar word points outside the calendar: slab "
                    : h.err & BK_EDST   ? "a run outside its destination's group: slab "
                    : h.err & BK_EQUEUE ? "a queue head outside its pool: host "
                                        : "a row outside the row buffer: host ";
  return set_error(ctx, SGN_EDEVICE, std::string("sgn_backlog: ") + why + std::to_string(h.err_info));
}

int bk_ensure(sgn_ctx* ctx) {
  if (ctx->bk_scratch) return 0;
  const uint32_t nH = ctx->S.nH;
  bool ok = hipMalloc(&ctx->bk_scratch, bk_lay(nH).bytes) == hipSuccess;
  ok = ok && hipHostMalloc(&ctx->bk_stage, bk_stage_bytes(nH), hipHostMallocDefault) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    backlog_release(ctx);
    return set_error(ctx, SGN_ENOMEM, "allocation failed (sgn_backlog)");
  }
  if (!ctx->bk_ev.make()) {
    backlog_release(ctx);
    return set_error(ctx, SGN_EDEVICE, "hipEventCreate failed (sgn_backlog)");
  }
  return 0;
}

}  // namespace

namespace sgn {

void backlog_release(sgn_ctx* ctx) {
  if (ctx->bk_scratch) (void)hipFree(ctx->bk_scratch);
  if (ctx->bk_stage) (void)hipHostFree(ctx->bk_stage);
  ctx->bk_scratch = ctx->bk_stage = nullptr;
  ctx->bk_ev.release();
  ctx->bk_timed = false;
  ctx->bk_timing = sgn_backlog_timing{};
}

}  // namespace sgn

extern "C" {

int sgn_backlog(sgn_ctx* ctx, sgn_backlog_row* out, uint64_t cap, uint64_t* n_out, sgn_backlog_info* info) {
  if (n_out) *n_out = 0;
  if (!ctx) return SGN_EINVAL;
  if (!n_out || !info || (!out && cap)) return set_error(ctx, SGN_EINVAL, "sgn_backlog: null argument");
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  const auto t_begin = std::chrono::steady_clock::now();
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  int rc = sync_ctrl(ctx);  // (the stream is idle; the round count, the window, the hold flags)
  if (rc) return rc;
  const bool sharded = ctx->nranks > 1 || ctx->comm_local;
  if (ctx->h_ctrl->hold || ctx->h_ctrl->spill_n || (sharded && ctx->h_ctrl->xspill)) {
    if (sharded)
      return set_error(ctx, SGN_ESTATE, "sgn_backlog: the round edge is held and one shard cannot resolve it: the next "
                                        "collective run or save call does (nothing was read)");
    // a resolved round edge, as sgn_snapshot_save makes one: every pending run in a slab or its extension
    ctx->ctrl_fresh = false;
    if ((rc = resolve_hold(ctx)) || (rc = sync_ctrl(ctx))) return rc;
    ctx->paused = false;
    if (ctx->h_ctrl->spill_n) return set_error(ctx, SGN_ESTATE, "sgn_backlog: the calendar's spill area is not empty");
  }
  const Ctrl& c = *ctx->h_ctrl;
  if ((rc = bk_ensure(ctx))) return rc;
  const uint32_t nH = ctx->S.nH, nW = (nH + 63) / 64;
  const BkLay L = bk_lay(nH);
  char* m = (char*)ctx->bk_scratch;
  BkHdr* d_hdr = (BkHdr*)(m + L.hdr);
  BkCal* d_cal = (BkCal*)(m + L.cal);
  uint32_t* d_cnt = (uint32_t*)(m + L.cnt);
  uint32_t* d_off = (uint32_t*)(m + L.off);
  uint64_t* d_maxq = (uint64_t*)(m + L.maxq);
  uint64_t* d_old = (uint64_t*)(m + L.old);
  uint32_t* d_oldh = (uint32_t*)(m + L.oldh);
  sgn_backlog_row* d_rows = (sgn_backlog_row*)(m + L.rows);
  BkHdr* h = (BkHdr*)ctx->bk_stage;  // (pinned: the header, then a piece of the rows)
  sgn_backlog_row* h_rows = (sgn_backlog_row*)((char*)ctx->bk_stage + sizeof(BkHdr));
  const BkArgs a = bk_args(ctx);
  hipStream_t st = ctx->stream;
  const ReportEvents<8>& ev = ctx->bk_ev;
  const uint32_t blocks = (nH + kBkThreads - 1) / kBkThreads;
  std::memset(h, 0, sizeof(BkHdr));
  h->inflight_earliest = INVALID;
  if (nH) {
    SGN_HIP(ctx, hipMemsetAsync(d_hdr, 0, sizeof(BkHdr), st));
    (void)hipEventRecord(ev[0], st);
    hipLaunchKernelGGL(k_backlog_calendar, dim3(a.G), dim3(kCalThreads), 0, st, a, d_cal, d_hdr);
    (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(k_backlog_count, dim3(blocks), dim3(kBkThreads), 0, st, a, (const BkCal*)d_cal, d_cnt, d_maxq, d_old, d_oldh, d_hdr);
    (void)hipEventRecord(ev[2], st);
    hipLaunchKernelGGL(k_backlog_scan, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t*)d_cnt, (const uint64_t*)d_maxq,
                       (const uint64_t*)d_old, (const uint32_t*)d_oldh, nW, d_off, d_hdr);
    (void)hipEventRecord(ev[3], st);
    if ((rc = read_header(ctx, d_hdr, h))) return rc;
    if (h->err) return bk_bad(ctx, *h);
    if (h->rows > nH) return set_error(ctx, SGN_EDEVICE, "sgn_backlog: the wave counts add up to more rows than hosts");
  }
  const uint64_t rows = h->rows;
  const bool want_rows = out && cap >= rows;  // (the row total against the caller's capacity, before the scatter)
  if (rows) {
    (void)hipEventRecord(ev[4], st);
    hipLaunchKernelGGL(k_backlog_scatter, dim3(blocks), dim3(kBkThreads), 0, st, a, (const BkCal*)d_cal, (const uint32_t*)d_off,
                       want_rows ? d_rows : (sgn_backlog_row*)nullptr, (uint64_t)nH, d_hdr);
    (void)hipEventRecord(ev[5], st);
    if ((rc = read_header(ctx, d_hdr, h))) return rc;
    if (h->err) return bk_bad(ctx, *h);
  }
  sgn_backlog_info in{};
  in.rounds = c.rounds;
  in.window_start = c.ws;
  in.window_end = c.we;
  in.hosts = nH;
  in.rows = rows;
  for (uint32_t k = 0; k < kTotals; k++) in.total[k] = h->total[k];
  in.max_router_packets = h->max_router;
  in.max_router_host = h->max_router_host;
  if (h->min_oldest != INVALID) {
    in.max_sojourn_ns = c.ws > h->min_oldest ? c.ws - h->min_oldest : 0;
    in.max_sojourn_host = h->min_oldest_host;
  }
  in.inflight_earliest = h->inflight_earliest;
  const uint64_t calendar_runs = h->calendar_runs;
  *info = in;
  *n_out = rows;
  sgn_backlog_timing T{};
  if (nH) T.kernel_ms[0] = elapsed_ms(ev[0], ev[1]);
  if (nH) T.kernel_ms[1] = elapsed_ms(ev[1], ev[2]);
  if (nH) T.kernel_ms[2] = elapsed_ms(ev[2], ev[3]);
  if (rows) T.kernel_ms[3] = elapsed_ms(ev[4], ev[5]);
  T.hosts = nH;
  T.rows = rows;
  T.calendar_runs = calendar_runs;
  if (out && cap < rows) {
    T.total_ms = ms_since(t_begin);
    ctx->bk_timing = T;
    ctx->bk_timed = true;
    return set_error(ctx, SGN_ERANGE, "sgn_backlog: " + std::to_string(rows) + " hosts have a row, the caller's array holds " +
                                          std::to_string(cap) + " (nothing was written to it)");
  }
  if (want_rows && rows) {  // piece by piece through the pinned buffer
    (void)hipEventRecord(ev[6], st);
    for (uint64_t r0 = 0; r0 < rows; r0 += kStageRows) {
      const uint64_t n = std::min<uint64_t>(kStageRows, rows - r0);
      SGN_HIP(ctx, hipMemcpyAsync(h_rows, d_rows + r0, n * sizeof(sgn_backlog_row), hipMemcpyDeviceToHost, st));
      SGN_HIP(ctx, hipStreamSynchronize(st));
      std::memcpy(out + r0, h_rows, n * sizeof(sgn_backlog_row));
    }
    (void)hipEventRecord(ev[7], st);
    SGN_HIP(ctx, hipStreamSynchronize(st));
    T.copy_ms = elapsed_ms(ev[6], ev[7]);
  }
  T.total_ms = ms_since(t_begin);
  ctx->bk_timing = T;
  ctx->bk_timed = true;
  return 0;
}

int sgn_backlog_timing_get(sgn_ctx* ctx, sgn_backlog_timing* out) {
  if (!ctx || !out) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_backlog_timing_get: null argument") : SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (!ctx->bk_timed) return set_error(ctx, SGN_ESTATE, "sgn_backlog_timing_get: no sgn_backlog since sgn_sim_init");
  *out = ctx->bk_timing;
  return 0;
}

}  // extern "C"

uint64_t sgn::layout_sig_backlog() { return kLayoutSig; }
