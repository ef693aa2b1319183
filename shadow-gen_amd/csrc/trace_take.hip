// trace_take.hip — the trace taken out in ordered pieces (sgn_trace_pending, sgn_trace_take).
//
// The round kernel appends trace records wherever its atomic counter puts them, so the buffer is
// in no order. A take hands the caller every record produced since the last take, sorted by
// (host, seq), and frees the whole buffer. No comparison sort: a host's seq is a counter of its
// own, so the records one take holds of a host carry CONSECUTIVE seq values, and a record's place
// in the output follows from three per-host numbers —
//   1. k_take_count  one pass over the pending records: per owned host the record count and the
//                    smallest and largest seq (atomics on dense per-host arrays);
//   2. k_take_scan   an exclusive scan of the counts over the hosts (HostId order): each host's
//                    offset, the spans {host, first, count} of the hosts with records, and the
//                    check count == max seq - min seq + 1 that the scatter relies on;
//   3. k_take_scatter  record r of host h goes to staging[off[h] + r.seq - min_seq[h]];
// then one device-to-host copy of the staging buffer. The kernels keep nothing between takes (no
// per-host cursor a snapshot restore would have to rewind): the only state is the context's count
// of records taken so far, sgn_ctx::trace_base.
//
// The buffer is never compacted. Ctrl::trace_n stays the count of records ever produced, and the
// kernels' view of the buffer moves instead: record p lives at trace_buf[p - trace_base], so
// DevSim::trace = trace_buf - trace_base and DevSim::trace_cap = trace_base + capacity
// (trace_view_set), and HostExec::trace() runs unchanged.
//
// A record is 56 bytes (sgn_trace_rec: four u32 and five u64), seven 8-byte words, so record i of
// a 16-byte aligned buffer starts 16-byte aligned for even i and 8 bytes past that for odd i.
// Four lanes read one record: three 16-byte loads and one 8-byte load (the last word of an even
// record, the first of an odd one). A record's place in the staging buffer has its own parity, so
// the scatter stores 8-byte words.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "report_common.h"

using namespace sgn;
using namespace sgn::report;  // the scan (kScanTile = 1024 hosts a tile), report_fail, the host scaffolding

// ---- device side ----------------------------------------------------------------------------
namespace {

constexpr uint32_t kTakeThreads = 256;                   // k_take_count, k_take_scatter: 64 records a pass
constexpr uint32_t kTakeRecs = kTakeThreads / 4;
constexpr uint32_t kTakeMaxBlocks = 2048;                // grid-stride above that
constexpr uint32_t kRecWords = sizeof(sgn_trace_rec) / 8;
static_assert(sizeof(sgn_trace_rec) == 56 && alignof(sgn_trace_rec) == 8, "a record is seven 8-byte words");
static_assert(offsetof(sgn_trace_rec, host) == 4 && offsetof(sgn_trace_rec, seq) == 40, "word 0 holds the host, word 5 the seq");
static_assert(sizeof(sgn_trace_span) == 24, "");

enum : uint32_t {
  TAKE_EHOST = 1u,   // a record of a host this shard does not own
  TAKE_ESEQ = 2u,    // a host's records do not carry consecutive seq
  TAKE_ERANGE = 4u,  // the scatter met a record outside its host's span (skipped)
};
struct __attribute__((aligned(16))) TakeHdr {
  uint64_t total, n_spans;  // k_take_scan: records counted, hosts with records
  uint32_t err, err_host;   // TAKE_E*, and the first offender (HostId)
  uint64_t pad[5];
};
static_assert(sizeof(TakeHdr) == 64, "");

// lane k (0..3) of the four that read record i: one or two of its words, w[0..nw), from word wi on
struct Piece {
  uint64_t w0, w1;
  uint32_t wi, nw;
};
__device__ __forceinline__ Piece load_piece(const sgn_trace_rec* __restrict__ recs, uint64_t i, uint32_t k) {
  const char* p = (const char*)(recs + i);
  Piece q;
  if ((i & 1) == 0) {  // 16-byte aligned: words {0,1} {2,3} {4,5} {6}
    if (k < 3) {
      const u64x2 v = *(const u64x2*)(p + 16 * k);
      q = Piece{v.x, v.y, 2 * k, 2u};
    } else {
      q = Piece{*(const uint64_t*)(p + 48), 0, 6u, 1u};
    }
  } else {  // 8 bytes past: words {0} {1,2} {3,4} {5,6}
    if (k == 0) {
      q = Piece{*(const uint64_t*)p, 0, 0u, 1u};
    } else {
      const u64x2 v = *(const u64x2*)(p + 16 * k - 8);
      q = Piece{v.x, v.y, 2 * k - 1, 2u};
    }
  }
  return q;
}
// the record's host (word 0's high half: lane 0 has it) and seq (word 5: lane 2's second word of an
// even record, lane 3's first of an odd one), to all four lanes; every lane of the wave calls it
__device__ __forceinline__ void piece_key(const Piece& q, uint64_t i, uint32_t* host, uint64_t* seq) {
  const uint64_t w0 = __shfl(q.w0, 0, 4);
  const uint64_t se = __shfl(q.w1, 2, 4), so = __shfl(q.w0, 3, 4);
  *host = (uint32_t)(w0 >> 32);
  *seq = (i & 1) ? so : se;
}

// 1. per owned host (index HostId - lo): records, smallest and largest seq.
// cnt and mx start at 0, mn at all ones (the host code's memsets).
__global__ __launch_bounds__(kTakeThreads) void k_take_count(const sgn_trace_rec* __restrict__ recs, uint64_t n, uint32_t lo,
                                                             uint32_t nH, unsigned long long* __restrict__ cnt,
                                                             unsigned long long* __restrict__ mn,
                                                             unsigned long long* __restrict__ mx, TakeHdr* __restrict__ hdr) {
  const uint32_t k = threadIdx.x & 3u, r = threadIdx.x >> 2;
  for (uint64_t b = (uint64_t)blockIdx.x * kTakeRecs; b < n; b += (uint64_t)gridDim.x * kTakeRecs) {
    const uint64_t i = b + r;
    const bool valid = i < n;
    const Piece q = valid ? load_piece(recs, i, k) : Piece{0, 0, 0u, 0u};
    uint32_t host;
    uint64_t seq;
    piece_key(q, i, &host, &seq);
    if (!valid || k != 0) continue;
    const uint32_t idx = host - lo;
    if (idx >= nH) {
      report_fail(&hdr->err, &hdr->err_host, TAKE_EHOST, host);
      continue;
    }
    atomicAdd(&cnt[idx], 1ull);
    atomicMin(&mn[idx], (unsigned long long)seq);
    atomicMax(&mx[idx], (unsigned long long)seq);
  }
}

// what k_take_scan scans: a host's records, and 1 for a host that has any
struct TakeSum {
  uint64_t c;
  uint32_t s;
};
__device__ __forceinline__ TakeSum operator+(TakeSum a, TakeSum b) { return TakeSum{a.c + b.c, a.s + b.s}; }
__device__ __forceinline__ TakeSum scan_shfl_up(TakeSum v, uint32_t d) { return TakeSum{__shfl_up(v.c, d), __shfl_up(v.s, d)}; }

// 2. one workgroup scans (records, hosts with records) over the hosts (tiled_scan): off[h] = records
// of the hosts before h, and a span for every host with records (ascending HostId).
__global__ __launch_bounds__(kScanThreads) void k_take_scan(const unsigned long long* __restrict__ cnt,
                                                            const unsigned long long* __restrict__ mn,
                                                            const unsigned long long* __restrict__ mx, uint32_t lo, uint32_t nH,
                                                            uint64_t* __restrict__ off, sgn_trace_span* __restrict__ spans,
                                                            uint64_t span_cap, TakeHdr* __restrict__ hdr) {
  const TakeSum sum = tiled_scan<TakeSum>(
      nH,
      [&](uint32_t h) {
        const uint64_t c = cnt[h];
        if (c && mx[h] - mn[h] + 1 != c) report_fail(&hdr->err, &hdr->err_host, TAKE_ESEQ, lo + h);
        return TakeSum{c, c ? 1u : 0u};
      },
      [&](uint32_t h, TakeSum before, TakeSum own) {
        off[h] = before.c;
        if (own.c && before.s < span_cap) spans[before.s] = sgn_trace_span{lo + h, 0u, before.c, own.c};
      });
  if (threadIdx.x == 0) {
    hdr->total = sum.c;
    hdr->n_spans = sum.s;
  }
}

// 3. every record to its place. A record outside its host's span — impossible once k_take_scan
// found every host's seq consecutive — is skipped and reported, never stored.
__global__ __launch_bounds__(kTakeThreads) void k_take_scatter(const sgn_trace_rec* __restrict__ recs, uint64_t n, uint32_t lo,
                                                               uint32_t nH, const unsigned long long* __restrict__ cnt,
                                                               const unsigned long long* __restrict__ mn,
                                                               const uint64_t* __restrict__ off, uint64_t* __restrict__ staging,
                                                               TakeHdr* __restrict__ hdr) {
  const uint32_t k = threadIdx.x & 3u, r = threadIdx.x >> 2;
  for (uint64_t b = (uint64_t)blockIdx.x * kTakeRecs; b < n; b += (uint64_t)gridDim.x * kTakeRecs) {
    const uint64_t i = b + r;
    const bool valid = i < n;
    const Piece q = valid ? load_piece(recs, i, k) : Piece{0, 0, 0u, 0u};
    uint32_t host;
    uint64_t seq;
    piece_key(q, i, &host, &seq);
    if (!valid) continue;
    const uint32_t idx = host - lo;
    uint64_t j = ~0ull;
    if (idx < nH) {
      const uint64_t d = seq - mn[idx];
      if (d < cnt[idx]) j = off[idx] + d;
    }
    if (j >= n) {
      if (k == 0) report_fail(&hdr->err, &hdr->err_host, TAKE_ERANGE, host);
      continue;
    }
    uint64_t* dst = staging + j * kRecWords + q.wi;
    dst[0] = q.w0;
    if (q.nw == 2) dst[1] = q.w1;
  }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
namespace {

// the scratch of one take: header, per-host words, spans, the staging records, and the upload area
// of a take whose records come from the host (the delay report's self-test)
struct TakeLay {
  size_t hdr, cnt, mx, mn, off, spans, staging, up, bytes;
};
TakeLay take_lay(uint32_t nH, uint64_t n_spans, uint64_t n, uint64_t n_up) {
  ScratchLay s;
  TakeLay l;
  l.hdr = s.take(sizeof(TakeHdr), 16);
  l.cnt = s.take((size_t)nH * 8, 8);
  l.mx = s.take((size_t)nH * 8, 8);  // (header, cnt and mx adjacent: one memset to zero)
  l.mn = s.take((size_t)nH * 8, 8);
  l.off = s.take((size_t)nH * 8, 8);
  l.spans = s.take((size_t)n_spans * sizeof(sgn_trace_span), 16);
  l.staging = s.take((size_t)n * sizeof(sgn_trace_rec), 16);
  l.up = s.take((size_t)n_up * sizeof(sgn_trace_rec), 16);
  l.bytes = s.bytes;
  return l;
}
int take_precheck(sgn_ctx* ctx, const char* what) {
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (!ctx->trace_buf) return set_error(ctx, SGN_ESTATE, std::string(what) + ": the simulation keeps no trace (sgn_trace_enable)");
  return 0;
}
int take_ensure(sgn_ctx* ctx, const char* what, size_t bytes) {
  if (ctx->take_bytes >= bytes) return 0;
  if (ctx->take_mem) (void)hipFree(ctx->take_mem);
  ctx->take_mem = nullptr;
  ctx->take_bytes = 0;
  if (hipMalloc(&ctx->take_mem, bytes) != hipSuccess) {
    ctx->take_mem = nullptr;
    (void)hipGetLastError();
    return set_error(ctx, SGN_ENOMEM, std::string("device allocation failed (") + what + ")");
  }
  ctx->take_bytes = bytes;
  return 0;
}

}  // namespace

namespace sgn {

static_assert(offsetof(DevSim, trace_cap) == offsetof(DevSim, trace) + 8, "trace_view_set uploads both words at once");

int trace_view_set(sgn_ctx* ctx, uint64_t base) {
  DevSim& S = ctx->S;
  ctx->trace_base = base;
  ctx->trace_held = base;  // (records past the position were laid out for the old cursor)
  // (unsigned arithmetic: the kernel adds pos * sizeof(record) back, pos >= base)
  S.trace = (decltype(S.trace))((uintptr_t)ctx->trace_buf - (uintptr_t)(base * sizeof(sgn_trace_rec)));
  S.trace_cap = base + ctx->trace_cap;
  SGN_HIP(ctx, hipMemcpy((char*)ctx->d_S + offsetof(DevSim, trace), (const char*)&S + offsetof(DevSim, trace), 16,
                         hipMemcpyHostToDevice));
  drop_graph(ctx);  // (a captured batch was made for the DevSim of its time)
  return 0;
}

int take_upload(sgn_ctx* ctx, const char* what, const sgn_trace_rec* recs, uint64_t n, uint32_t nH) {
  const TakeLay L = take_lay(nH, std::min<uint64_t>(nH, n), n, n);
  if (int rc = take_ensure(ctx, what, L.bytes)) return rc;
  SGN_HIP(ctx, hipMemcpyAsync((char*)ctx->take_mem + L.up, recs, n * sizeof(sgn_trace_rec), hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

int take_run(sgn_ctx* ctx, const char* what, const sgn_trace_rec* d_src, uint64_t n, uint64_t n_up, uint32_t lo, uint32_t nH,
             bool discard, sgn_trace_rec* out, uint64_t cap, uint64_t* n_out, sgn_trace_span* spans, uint64_t span_cap,
             uint64_t* n_spans, DelayState* dl) {
  const auto t_begin = std::chrono::steady_clock::now();
  const uint64_t sp_cap = std::min<uint64_t>(nH, n);  // (at most one span per host and per record)
  const TakeLay L = take_lay(nH, sp_cap, n, n_up);
  if (int rc = take_ensure(ctx, what, L.bytes)) return rc;
  char* m = (char*)ctx->take_mem;
  if (!d_src) d_src = (const sgn_trace_rec*)(m + L.up);
  TakeHdr* d_hdr = (TakeHdr*)(m + L.hdr);
  unsigned long long* d_cnt = (unsigned long long*)(m + L.cnt);
  unsigned long long* d_mx = (unsigned long long*)(m + L.mx);
  unsigned long long* d_mn = (unsigned long long*)(m + L.mn);
  uint64_t* d_off = (uint64_t*)(m + L.off);
  sgn_trace_span* d_spans = (sgn_trace_span*)(m + L.spans);
  uint64_t* d_staging = (uint64_t*)(m + L.staging);
  ReportEvents<6> E;  // (created per take and destroyed on every way out)
  if (!E.make()) return set_error(ctx, SGN_EDEVICE, std::string("hipEventCreate failed (") + what + ")");
  hipStream_t st = ctx->stream;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(kTakeMaxBlocks, (n + kTakeRecs - 1) / kTakeRecs);
  const std::string pre = std::string(what) + ": ";

  SGN_HIP(ctx, hipMemsetAsync(m + L.hdr, 0, L.mn - L.hdr, st));  // header, cnt, mx
  SGN_HIP(ctx, hipMemsetAsync(d_mn, 0xFF, (size_t)nH * 8, st));
  (void)hipEventRecord(E[0], st);
  hipLaunchKernelGGL(k_take_count, dim3(blocks), dim3(kTakeThreads), 0, st, d_src, n, lo, nH, d_cnt, d_mn, d_mx, d_hdr);
  (void)hipEventRecord(E[1], st);
  hipLaunchKernelGGL(k_take_scan, dim3(1), dim3(kScanThreads), 0, st, (const unsigned long long*)d_cnt,
                     (const unsigned long long*)d_mn, (const unsigned long long*)d_mx, lo, nH, d_off, d_spans, sp_cap, d_hdr);
  (void)hipEventRecord(E[2], st);
  TakeHdr h{};
  if (int rc = read_header(ctx, d_hdr, &h)) return rc;
  auto bad = [&](const TakeHdr& x) {
    const char* why = x.err & TAKE_EHOST  ? "a record of a host this shard does not own: host "
                      : x.err & TAKE_ESEQ ? "the pending records do not carry consecutive seq: host "
                                          : "a record outside its host's span: host ";
    return set_error(ctx, SGN_EDEVICE, pre + why + std::to_string(x.err_host) + " (nothing was taken)");
  };
  if (h.err) return bad(h);
  if (h.total != n || h.n_spans > sp_cap)
    return set_error(ctx, SGN_EDEVICE, pre + "the per-host counts add up to " + std::to_string(h.total) + " of " +
                                           std::to_string(n) + " pending records (nothing was taken)");
  if (!discard && (cap < n || (spans && span_cap < h.n_spans))) {
    *n_out = n;
    if (n_spans) *n_spans = h.n_spans;
    return set_error(ctx, SGN_ERANGE, pre + std::to_string(n) + " records of " + std::to_string(h.n_spans) +
                                          " hosts are pending, the caller's arrays are smaller (nothing was taken)");
  }
  (void)hipEventRecord(E[3], st);
  hipLaunchKernelGGL(k_take_scatter, dim3(blocks), dim3(kTakeThreads), 0, st, d_src, n, lo, nH, (const unsigned long long*)d_cnt,
                     (const unsigned long long*)d_mn, (const uint64_t*)d_off, d_staging, d_hdr);
  (void)hipEventRecord(E[4], st);
  if (int rc = read_header(ctx, d_hdr, &h)) return rc;
  if (h.err) return bad(h);
  if (dl) {  // the report reads the ordered records where they are; nothing it keeps changes before the commit
    const DelayFoldIn in{d_staging, d_spans, d_cnt, d_off, n, h.n_spans, lo, nH};
    if (int rc = delay_fold_prepare(ctx, dl, in, what)) return rc;
  }
  if (!discard) {
    SGN_HIP(ctx, hipMemcpyAsync(out, d_staging, n * sizeof(sgn_trace_rec), hipMemcpyDeviceToHost, st));
    if (spans && h.n_spans)
      SGN_HIP(ctx, hipMemcpyAsync(spans, d_spans, h.n_spans * sizeof(sgn_trace_span), hipMemcpyDeviceToHost, st));
  }
  (void)hipEventRecord(E[5], st);
  SGN_HIP(ctx, hipStreamSynchronize(st));
  if (dl) {
    if (int rc = delay_fold_commit(ctx, dl, n)) return rc;
    sgn_delay_timing& D = ctx->dl_timing;
    D.order_ms[0] = elapsed_ms(E[0], E[1]);
    D.order_ms[1] = elapsed_ms(E[1], E[2]);
    D.order_ms[2] = elapsed_ms(E[3], E[4]);
    D.total_ms = ms_since(t_begin);
  }
  if (n_out) *n_out = n;
  if (n_spans) *n_spans = h.n_spans;
  sgn_trace_take_timing& T = ctx->take_timing;
  T.kernel_ms[0] = elapsed_ms(E[0], E[1]);
  T.kernel_ms[1] = elapsed_ms(E[1], E[2]);
  T.kernel_ms[2] = elapsed_ms(E[3], E[4]);
  T.copy_ms = discard ? 0.0 : elapsed_ms(E[4], E[5]);
  T.records = n;
  T.hosts = h.n_spans;
  T.total_ms = ms_since(t_begin);
  return 0;
}

int trace_take_common(sgn_ctx* ctx, const char* what, bool discard, sgn_trace_rec* out, uint64_t cap, uint64_t* n_out,
                      sgn_trace_span* spans, uint64_t span_cap, uint64_t* n_spans) {
  if (int rc = take_precheck(ctx, what)) return rc;
  if (discard && !ctx->dl) return set_error(ctx, SGN_ESTATE, std::string(what) + ": the report is not enabled (sgn_delay_enable)");
  const auto t_begin = std::chrono::steady_clock::now();
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = sync_ctrl(ctx)) return rc;  // (a trace overflow since the last take is reported here)
  const DevSim& S = ctx->S;
  const uint64_t tn = ctx->h_ctrl->trace_n;
  const uint64_t n = tn > ctx->trace_base ? tn - ctx->trace_base : 0;
  ctx->take_timing = sgn_trace_take_timing{};
  if (ctx->dl)
    if (int rc = delay_position_check(ctx, what)) return rc;
  if (n > ctx->trace_cap) return set_error(ctx, SGN_EOVERFLOW, std::string(what) + ": more records pending than the trace buffer holds");
  if (n == 0) {
    if (ctx->dl) delay_position_set(ctx, ctx->trace_base, true);
    ctx->take_timing.total_ms = ms_since(t_begin);
    return 0;
  }
  if (int rc = take_run(ctx, what, (const sgn_trace_rec*)ctx->trace_buf, n, 0, S.lo, S.nH, discard, out, cap, n_out, spans, span_cap,
                        n_spans, ctx->dl))
    return rc;
  // the buffer is empty: the next record goes to its start
  if (int rc = trace_view_set(ctx, tn)) return rc;
  if (ctx->dl) delay_position_set(ctx, tn, true);
  ctx->take_timing.total_ms = ms_since(t_begin);
  return 0;
}

}  // namespace sgn

extern "C" {

int sgn_trace_pending(sgn_ctx* ctx, uint64_t* n) {
  if (n) *n = 0;
  if (!ctx || !n) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_trace_pending: null argument") : SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  const int rc = sync_ctrl(ctx);
  if (!ctx->trace_buf) return rc;  // (an untraced simulation produces none)
  const uint64_t tn = ctx->h_ctrl->trace_n;
  *n = tn > ctx->trace_base ? tn - ctx->trace_base : 0;
  return rc;
}

int sgn_trace_take(sgn_ctx* ctx, sgn_trace_rec* out, uint64_t cap, uint64_t* n_out, sgn_trace_span* spans, uint64_t span_cap,
                   uint64_t* n_spans) {
  if (n_out) *n_out = 0;
  if (n_spans) *n_spans = 0;
  if (!ctx || !n_out || (!out && cap) || (!spans && span_cap))
    return ctx ? set_error(ctx, SGN_EINVAL, "sgn_trace_take: null argument") : SGN_EINVAL;
  return trace_take_common(ctx, "sgn_trace_take", false, out, cap, n_out, spans, span_cap, n_spans);
}

int sgn_trace_take_timing_get(sgn_ctx* ctx, sgn_trace_take_timing* out) {
  if (!ctx || !out) return SGN_EINVAL;
  *out = ctx->take_timing;
  return 0;
}

}  // extern "C"

uint64_t sgn::layout_sig_trace_take() { return kLayoutSig; }
