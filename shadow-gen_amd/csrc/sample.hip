// sample.hip — interval statistics: per-host counters sampled on the device (sgn_sample_*).
//
// The seven per-host counters behind sgn_host_digests and sgn_stats_get already live in device
// memory and are final at every launch boundary: n_sent / n_popped / n_delivered in the dense
// DevSim::n_cnt rows (PERIODIC) or in the host record (TGEN, EXTERNAL), n_codel / n_unknown /
// n_local_deliv / n_blocked in the host record for every kind. A sample compares them with a
// device-resident baseline and keeps one 64-byte row (current - baseline) per host that changed,
// ascending by HostId, in three launches — the count / scan / scatter shape of trace_take.hip:
//   1. k_sample_count    one lane per owned HostId (sid_of -> slot): load the counters, compare
//                        with the baseline, ballot; one count of changed hosts per wave;
//   2. k_sample_scan     one workgroup: an exclusive scan of the wave counts, and the sample's row
//                        total, which the host checks against the free rows before anything is
//                        written (all or nothing: SGN_EOVERFLOW changes nothing);
//   3. k_sample_scatter  the same flags again; a changed host's row goes to rows[first + wave
//                        offset + its rank among the wave's changed lanes] as four 16-byte stores,
//                        its baseline becomes the current values, and the seven deltas are summed
//                        over the wave and added to the sample's totals, one 64-bit atomic add per
//                        wave and counter.
// Nothing of the round path is touched: the kernels read the simulation's buffers and write only
// the sampler's own (baseline, rows, scratch). The baseline is counter-major and indexed by
// HostId - lo, so a wave's baseline accesses are contiguous; the counters are gathered from the
// hosts' (permuted) slots.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>

#include "report_common.h"

using namespace sgn;
using namespace sgn::report;  // the scan (kScanTile = 1024 waves a tile), the wave reductions, the host scaffolding

// ---- device side ----------------------------------------------------------------------------
namespace {

constexpr uint32_t kSmpThreads = 256;  // k_sample_count, _scatter, _rebase: one lane per host
constexpr uint32_t kCounters = 7;

static_assert(sizeof(sgn_sample_row) == 64 && offsetof(sgn_sample_row, sent) == 8 && offsetof(sgn_sample_row, blocked) == 56,
              "a row is four 16-byte stores: {host | sample, sent}, {popped, delivered}, {codel, unknown}, {local, blocked}");
static_assert(sizeof(sgn_sample_info) == 104, "");
// the record's counters lie in one 128-byte line (a sample reads one line per TGEN / EXTERNAL host,
// and 32 bytes of it per PERIODIC host)
static_assert(offsetof(HostRec, n_sent) / 128 == (offsetof(HostRec, n_blocked) + 7) / 128 &&
                  offsetof(HostRec, n_sent) < offsetof(HostRec, n_popped) && offsetof(HostRec, n_delivered) < offsetof(HostRec, n_codel) &&
                  offsetof(HostRec, n_codel) < offsetof(HostRec, n_blocked),
              "HostRec's per-host counters left their cache line");
static_assert(offsetof(HostRec, n_codel) % 16 == 0 && offsetof(HostRec, n_local_deliv) == offsetof(HostRec, n_codel) + 16,
              "n_codel .. n_blocked are two aligned 16-byte loads");

enum : uint32_t {
  SMP_ESLOT = 1u,  // a host's slot lies outside the shard (nothing of it was read)
  SMP_EROW = 2u,   // the scatter met a row outside the buffer (skipped)
};
struct __attribute__((aligned(16))) SmpHdr {
  uint64_t rows;              // k_sample_scan: hosts that changed
  uint32_t err, err_host;     // SMP_E*, and the first offender (HostId)
  uint64_t total[kCounters];  // k_sample_scatter: the rows' deltas summed
  uint64_t pad[7];
};
static_assert(sizeof(SmpHdr) == 128, "");

// what the kernels read of the simulation, and the baseline
struct SmpArgs {
  const HostRec* hrec;      // [nH] by slot
  const uint64_t* n_cnt;    // [N_CNT * nH] by slot (PERIODIC), else null: the counters are in hrec
  const uint32_t* sid_of;   // [n_all] HostId -> lo + slot
  uint64_t* base;           // [kCounters * nH] by HostId - lo
  uint32_t lo, nH;
};

// the seven counters of owned host i (HostId lo + i); false: its slot is not this shard's
__device__ __forceinline__ bool load_counters(const SmpArgs& a, uint32_t i, uint64_t c[kCounters]) {
  const uint32_t slot = a.sid_of[a.lo + i] - a.lo;
  if (slot >= a.nH) return false;
  const HostRec* r = a.hrec + slot;
  if (a.n_cnt) {
    c[0] = a.n_cnt[(size_t)N_SENT * a.nH + slot];
    c[1] = a.n_cnt[(size_t)N_POPPED * a.nH + slot];
    c[2] = a.n_cnt[(size_t)N_DELIVERED * a.nH + slot];
  } else {
    c[0] = r->n_sent;
    c[1] = r->n_popped;
    c[2] = r->n_delivered;
  }
  const u64x2 v = *(const u64x2*)&r->n_codel, w = *(const u64x2*)&r->n_local_deliv;
  c[3] = v.x;  // n_codel
  c[4] = v.y;  // n_unknown
  c[5] = w.x;  // n_local_deliv
  c[6] = w.y;  // n_blocked
  return true;
}

// 1. per wave (64 consecutive HostIds): the hosts whose counters differ from the baseline
__global__ __launch_bounds__(kSmpThreads) void k_sample_count(SmpArgs a, uint32_t* __restrict__ wave_cnt, SmpHdr* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * kSmpThreads + threadIdx.x;
  bool changed = false;
  if (i < a.nH) {
    uint64_t c[kCounters];
    if (load_counters(a, i, c)) {
#pragma unroll
      for (uint32_t k = 0; k < kCounters; k++) changed |= c[k] != a.base[(size_t)k * a.nH + i];
    } else {
      report_fail(&hdr->err, &hdr->err_host, SMP_ESLOT, a.lo + i);
    }
  }
  const uint64_t m = __ballot(changed);
  if ((threadIdx.x & 63u) == 0 && i < a.nH) wave_cnt[i >> 6] = (uint32_t)__popcll(m);
}

// 2. one workgroup scans the nW wave counts (tiled_scan; the total is at most nH < 2^32):
// wave_off[w] = changed hosts of the waves before w
__global__ __launch_bounds__(kScanThreads) void k_sample_scan(const uint32_t* __restrict__ wave_cnt, uint32_t nW,
                                                              uint32_t* __restrict__ wave_off, SmpHdr* __restrict__ hdr) {
  const uint32_t rows = tiled_scan<uint32_t>(
      nW, [&](uint32_t j) { return wave_cnt[j]; }, [&](uint32_t j, uint32_t before, uint32_t) { wave_off[j] = before; });
  if (threadIdx.x == 0) hdr->rows = rows;
}

// 3. rows, baseline, totals. The flags are those of k_sample_count (nothing ran in between), so
// every row lies in [first, first + hdr->rows), which the host found free; a row outside the
// buffer is skipped and reported, never stored.
__global__ __launch_bounds__(kSmpThreads) void k_sample_scatter(SmpArgs a, const uint32_t* __restrict__ wave_off,
                                                                sgn_sample_row* __restrict__ rows, uint64_t first, uint64_t cap,
                                                                uint32_t sample, SmpHdr* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * kSmpThreads + threadIdx.x, lane = threadIdx.x & 63u;
  uint64_t c[kCounters], d[kCounters];
#pragma unroll
  for (uint32_t k = 0; k < kCounters; k++) d[k] = 0;
  bool changed = false;
  if (i < a.nH && load_counters(a, i, c)) {
#pragma unroll
    for (uint32_t k = 0; k < kCounters; k++) {
      d[k] = c[k] - a.base[(size_t)k * a.nH + i];
      changed |= d[k] != 0;
    }
  }
  const uint64_t m = __ballot(changed);
  if (m == 0) return;  // (the whole wave: nothing to write, nothing to add)
  if (changed) {
    const uint64_t j = first + wave_off[i >> 6] + rank_below(m, lane);
    if (j < cap) {
      u64x2* p = (u64x2*)(rows + j);
      p[0] = u64x2{(uint64_t)(a.lo + i) | (uint64_t)sample << 32, d[0]};
      p[1] = u64x2{d[1], d[2]};
      p[2] = u64x2{d[3], d[4]};
      p[3] = u64x2{d[5], d[6]};
#pragma unroll
      for (uint32_t k = 0; k < kCounters; k++)
        if (d[k]) a.base[(size_t)k * a.nH + i] = c[k];
    } else {
      report_fail(&hdr->err, &hdr->err_host, SMP_EROW, a.lo + i);
#pragma unroll
      for (uint32_t k = 0; k < kCounters; k++) d[k] = 0;
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kCounters; k++) {
    const uint64_t s = wave_sum(d[k]);
    if (lane == 0 && s) atomicAdd((unsigned long long*)&hdr->total[k], (unsigned long long)s);
  }
}

// the baseline := the counters as they are (sgn_sample_enable, sgn_sample_rebase)
__global__ __launch_bounds__(kSmpThreads) void k_sample_rebase(SmpArgs a, SmpHdr* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * kSmpThreads + threadIdx.x;
  if (i >= a.nH) return;
  uint64_t c[kCounters];
  if (!load_counters(a, i, c)) {
    report_fail(&hdr->err, &hdr->err_host, SMP_ESLOT, a.lo + i);
    return;
  }
#pragma unroll
  for (uint32_t k = 0; k < kCounters; k++) a.base[(size_t)k * a.nH + i] = c[k];
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
namespace {

// the scratch of one sample: header, per-wave counts, per-wave offsets
struct SmpLay {
  size_t hdr, cnt, off, bytes;
};
SmpLay smp_lay(size_t nW) {
  ScratchLay s;
  SmpLay l;
  l.hdr = s.take(sizeof(SmpHdr), 16);
  l.cnt = s.take(nW * 4, 16);
  l.off = s.take(nW * 4, 16);
  l.bytes = s.take(0, 16);
  return l;
}

SmpArgs smp_args(const sgn_ctx* ctx) {
  const DevSim& S = ctx->S;
  SmpArgs a;
  a.hrec = (const HostRec*)S.hrec;
  a.n_cnt = S.tkind == SGN_TRAFFIC_PERIODIC ? (const uint64_t*)S.n_cnt : nullptr;
  a.sid_of = (const uint32_t*)S.sid_of;
  a.base = (uint64_t*)ctx->smp_base;
  a.lo = S.lo;
  a.nH = S.nH;
  return a;
}

int smp_precheck(sgn_ctx* ctx, const char* what) {
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (!ctx->smp_rows) return set_error(ctx, SGN_ESTATE, std::string(what) + ": the sampler is not enabled (sgn_sample_enable)");
  return 0;
}

int smp_bad(sgn_ctx* ctx, const char* what, const SmpHdr& h) {
  const char* why = h.err & SMP_ESLOT ? "a host's slot lies outside the shard: host " : "a row outside the row buffer: host ";
  return set_error(ctx, SGN_EDEVICE, std::string(what) + ": " + why + std::to_string(h.err_host));
}

// the baseline from the counters as they are now; the stream is idle on return
int smp_rebase(sgn_ctx* ctx, const char* what) {
  if (int rc = sync_ctrl(ctx)) return rc;
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t nH = ctx->S.nH;
  SmpHdr* d_hdr = (SmpHdr*)ctx->smp_scratch;
  hipStream_t st = ctx->stream;
  SGN_HIP(ctx, hipMemsetAsync(d_hdr, 0, sizeof(SmpHdr), st));
  if (nH) hipLaunchKernelGGL(k_sample_rebase, dim3((nH + kSmpThreads - 1) / kSmpThreads), dim3(kSmpThreads), 0, st, smp_args(ctx), d_hdr);
  SmpHdr h{};
  if (int rc = read_header(ctx, d_hdr, &h)) return rc;
  if (h.err) return smp_bad(ctx, what, h);
  ctx->smp_base_rounds = ctx->h_ctrl->rounds;
  ctx->smp_stale = false;
  return 0;
}

}  // namespace

namespace sgn {

void sample_release(sgn_ctx* ctx) {
  if (ctx->smp_rows) (void)hipFree(ctx->smp_rows);
  if (ctx->smp_base) (void)hipFree(ctx->smp_base);
  if (ctx->smp_scratch) (void)hipFree(ctx->smp_scratch);
  ctx->smp_rows = ctx->smp_base = ctx->smp_scratch = nullptr;
  ctx->smp_ev.release();
  ctx->smp_cap = ctx->smp_pending = 0;
  ctx->smp_index = ctx->smp_base_rounds = 0;
  ctx->smp_stale = false;
  ctx->smp_infos.clear();
  ctx->smp_timing = sgn_sample_timing{};
}

}  // namespace sgn

extern "C" {

int sgn_sample_enable(sgn_ctx* ctx, uint64_t row_capacity) {
  if (!ctx) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (row_capacity == 0) return set_error(ctx, SGN_EINVAL, "sgn_sample_enable: row_capacity must be >= 1");
  if (row_capacity > (~0ull >> 8)) return set_error(ctx, SGN_EINVAL, "sgn_sample_enable: row_capacity too large");
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  sample_release(ctx);
  const uint32_t nH = ctx->S.nH;
  const SmpLay L = smp_lay(((size_t)nH + 63) / 64);
  bool ok = hipMalloc(&ctx->smp_rows, row_capacity * sizeof(sgn_sample_row)) == hipSuccess;
  ok = ok && hipMalloc(&ctx->smp_base, std::max<size_t>(16, (size_t)kCounters * nH * 8)) == hipSuccess;
  ok = ok && hipMalloc(&ctx->smp_scratch, L.bytes) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    sample_release(ctx);
    return set_error(ctx, SGN_ENOMEM, "device allocation failed (sgn_sample_enable)");
  }
  if (!ctx->smp_ev.make()) {
    sample_release(ctx);
    return set_error(ctx, SGN_EDEVICE, "hipEventCreate failed (sgn_sample_enable)");
  }
  ctx->smp_cap = row_capacity;
  if (int rc = smp_rebase(ctx, "sgn_sample_enable")) {
    sample_release(ctx);
    return rc;
  }
  return 0;
}

int sgn_sample_rebase(sgn_ctx* ctx) {
  if (!ctx) return SGN_EINVAL;
  if (int rc = smp_precheck(ctx, "sgn_sample_rebase")) return rc;
  return smp_rebase(ctx, "sgn_sample_rebase");
}

int sgn_sample(sgn_ctx* ctx, sgn_sample_info* out) {
  if (!ctx) return SGN_EINVAL;
  if (int rc = smp_precheck(ctx, "sgn_sample")) return rc;
  const auto t_begin = std::chrono::steady_clock::now();
  if (int rc = sync_ctrl(ctx)) return rc;  // (the stream is idle; the round count and the window)
  const Ctrl& c = *ctx->h_ctrl;
  if (c.rounds < ctx->smp_base_rounds) ctx->smp_stale = true;
  if (ctx->smp_stale)
    return set_error(ctx, SGN_ESTATE, "sgn_sample: the simulation went back behind the baseline (round " + std::to_string(c.rounds) +
                                          ", baseline of round " + std::to_string(ctx->smp_base_rounds) + "): sgn_sample_rebase first");
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t nH = ctx->S.nH, nW = (nH + 63) / 64;
  const SmpLay L = smp_lay(nW);
  char* m = (char*)ctx->smp_scratch;
  SmpHdr* d_hdr = (SmpHdr*)(m + L.hdr);
  uint32_t* d_cnt = (uint32_t*)(m + L.cnt);
  uint32_t* d_off = (uint32_t*)(m + L.off);
  const SmpArgs a = smp_args(ctx);
  hipStream_t st = ctx->stream;
  const ReportEvents<8>& ev = ctx->smp_ev;
  const uint32_t blocks = (nH + kSmpThreads - 1) / kSmpThreads;
  SmpHdr h{};
  if (nH) {
    SGN_HIP(ctx, hipMemsetAsync(d_hdr, 0, sizeof(SmpHdr), st));
    (void)hipEventRecord(ev[0], st);
    hipLaunchKernelGGL(k_sample_count, dim3(blocks), dim3(kSmpThreads), 0, st, a, d_cnt, d_hdr);
    (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t*)d_cnt, nW, d_off, d_hdr);
    (void)hipEventRecord(ev[2], st);
    if (int rc = read_header(ctx, d_hdr, &h)) return rc;
    if (h.err) return smp_bad(ctx, "sgn_sample", h);
    if (h.rows > nH) return set_error(ctx, SGN_EDEVICE, "sgn_sample: the wave counts add up to more rows than hosts");
  }
  const uint64_t rows = h.rows, free_rows = ctx->smp_cap - ctx->smp_pending;
  if (rows > free_rows)
    return set_error(ctx, SGN_EOVERFLOW, "sgn_sample: the sample needs " + std::to_string(rows) + " rows, " + std::to_string(free_rows) +
                                             " of " + std::to_string(ctx->smp_cap) + " are free (sgn_sample_take, or a larger row_capacity); nothing was appended");
  if (rows) {
    (void)hipEventRecord(ev[3], st);
    hipLaunchKernelGGL(k_sample_scatter, dim3(blocks), dim3(kSmpThreads), 0, st, a, (const uint32_t*)d_off,
                       (sgn_sample_row*)ctx->smp_rows, ctx->smp_pending, ctx->smp_cap, (uint32_t)ctx->smp_index, d_hdr);
    (void)hipEventRecord(ev[4], st);
    if (int rc = read_header(ctx, d_hdr, &h)) return rc;
    if (h.err) return smp_bad(ctx, "sgn_sample", h);
  }
  sgn_sample_info info{};
  info.sample = ctx->smp_index;
  info.rounds = c.rounds;
  info.window_start = c.ws;
  info.window_end = c.we;
  info.first_row = ctx->smp_pending;
  info.rows = rows;
  for (uint32_t k = 0; k < kCounters; k++) info.total[k] = h.total[k];
  ctx->smp_infos.push_back(info);
  ctx->smp_pending += rows;
  ctx->smp_index++;
  ctx->smp_base_rounds = c.rounds;
  if (out) *out = info;
  sgn_sample_timing& T = ctx->smp_timing;
  const double copy_ms = T.copy_ms;  // (of the last take)
  T = sgn_sample_timing{};
  T.copy_ms = copy_ms;
  if (nH) T.kernel_ms[0] = elapsed_ms(ev[0], ev[1]);
  if (nH) T.kernel_ms[1] = elapsed_ms(ev[1], ev[2]);
  if (rows) T.kernel_ms[2] = elapsed_ms(ev[3], ev[4]);
  T.hosts = nH;
  T.rows = rows;
  T.total_ms = ms_since(t_begin);
  return 0;
}

int sgn_sample_pending(sgn_ctx* ctx, uint64_t* rows, uint64_t* samples) {
  if (rows) *rows = 0;
  if (samples) *samples = 0;
  if (!ctx) return SGN_EINVAL;
  if (int rc = smp_precheck(ctx, "sgn_sample_pending")) return rc;
  if (rows) *rows = ctx->smp_pending;
  if (samples) *samples = ctx->smp_infos.size();
  return 0;
}

int sgn_sample_take(sgn_ctx* ctx, sgn_sample_row* out, uint64_t cap, uint64_t* n_out, sgn_sample_info* infos, uint64_t info_cap,
                    uint64_t* n_infos) {
  if (n_out) *n_out = 0;
  if (n_infos) *n_infos = 0;
  if (!ctx || !n_out || (!out && cap) || (!infos && info_cap))
    return ctx ? set_error(ctx, SGN_EINVAL, "sgn_sample_take: null argument") : SGN_EINVAL;
  if (int rc = smp_precheck(ctx, "sgn_sample_take")) return rc;
  const uint64_t n = ctx->smp_pending, ni = ctx->smp_infos.size();
  if (cap < n || info_cap < ni) {
    *n_out = n;
    if (n_infos) *n_infos = ni;
    return set_error(ctx, SGN_ERANGE, "sgn_sample_take: " + std::to_string(n) + " rows of " + std::to_string(ni) +
                                          " samples are pending, the caller's arrays are smaller (nothing was taken)");
  }
  if (n) {
    SGN_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    (void)hipEventRecord(ctx->smp_ev[5], st);
    SGN_HIP(ctx, hipMemcpyAsync(out, ctx->smp_rows, n * sizeof(sgn_sample_row), hipMemcpyDeviceToHost, st));
    (void)hipEventRecord(ctx->smp_ev[6], st);
    SGN_HIP(ctx, hipStreamSynchronize(st));
    ctx->smp_timing.copy_ms = elapsed_ms(ctx->smp_ev[5], ctx->smp_ev[6]);
  } else {
    ctx->smp_timing.copy_ms = 0;
  }
  if (ni) std::memcpy(infos, ctx->smp_infos.data(), ni * sizeof(sgn_sample_info));
  ctx->smp_infos.clear();
  ctx->smp_pending = 0;
  *n_out = n;
  if (n_infos) *n_infos = ni;
  return 0;
}

int sgn_sample_timing_get(sgn_ctx* ctx, sgn_sample_timing* out) {
  if (!ctx || !out) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_sample_timing_get: null argument") : SGN_EINVAL;
  if (int rc = smp_precheck(ctx, "sgn_sample_timing_get")) return rc;
  *out = ctx->smp_timing;
  return 0;
}

// Test hook: k_sample_scan on the caller's counts (no simulation needed).
int sgn_selftest_report_scan(sgn_ctx* ctx, const uint32_t* counts, uint32_t n, uint32_t* off_out, uint64_t* total_out) {
  if (!ctx || !total_out || (n && (!counts || !off_out)))
    return ctx ? set_error(ctx, SGN_EINVAL, "sgn_selftest_report_scan: null argument") : SGN_EINVAL;
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  const SmpLay L = smp_lay(std::max<uint32_t>(n, 1u));
  char* m = nullptr;
  SGN_HIP(ctx, hipMalloc(&m, L.bytes));
  SmpHdr* d_hdr = (SmpHdr*)(m + L.hdr);
  uint32_t* d_cnt = (uint32_t*)(m + L.cnt);
  uint32_t* d_off = (uint32_t*)(m + L.off);
  hipStream_t st = ctx->stream;
  SmpHdr h{};
  hipError_t e = hipMemsetAsync(d_hdr, 0, sizeof(SmpHdr), st);
  if (e == hipSuccess && n) e = hipMemcpyAsync(d_cnt, counts, (size_t)n * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t*)d_cnt, n, d_off, d_hdr);
    e = hipGetLastError();
  }
  if (e == hipSuccess && n) e = hipMemcpyAsync(off_out, d_off, (size_t)n * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d_hdr, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(m);
  if (e != hipSuccess) return hip_fail(ctx, e, "report scan selftest");
  *total_out = h.rows;
  return 0;
}

}  // extern "C"

uint64_t sgn::layout_sig_sample() { return kLayoutSig; }
