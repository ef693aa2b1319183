// interop.cpp — what the C ABI reads back from a simulation and feeds into it between rounds:
// stats, digests, next-event times, the trace, engine info and kernel times, the sgn_debug_*
// buffers; sgn_submit / sgn_stage_* / sgn_drain (EXTERNAL traffic); the host-RNG calls. Host
// code only: its kernels are launched through engine.hip's launch functions (sgn_internal.h).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "sgn_internal.h"
#include "sgn_workload.h"

using namespace sgn;

extern "C" {

namespace {
// the records of owned hosts [off, off + n) (device -> host)
int read_recs(sgn_ctx* ctx, uint32_t off, uint32_t n, std::vector<HostRec>* out) {
  out->resize(n);
  if (n) SGN_HIP(ctx, hipMemcpy(out->data(), (const void*)(ctx->S.hrec + off), (size_t)n * sizeof(HostRec),
                                hipMemcpyDeviceToHost));
  if (n && ctx->S.htile) {  // the hot lines from their tiles
    const uint32_t t0 = off >> 6, t1 = (off + n + 63) >> 6;
    std::vector<uint64_t> tile((size_t)(t1 - t0) * 8 * 64 * 2);
    SGN_HIP(ctx, hipMemcpy(tile.data(), (const void*)(ctx->S.htile + (size_t)t0 * 8 * 64 * 2), tile.size() * 8,
                           hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++)
      for (uint32_t c = 0; c < 8; c++)
        std::memcpy((char*)&(*out)[i] + 16 * c, &tile[2 * (hot_idx(off + i, c) - (size_t)t0 * 8 * 64)], 16);
  }
  return 0;
}
// the per-host totals of owned slots [off, off + n): N_CNT rows, then the CoDel maxima
int read_counts(sgn_ctx* ctx, uint32_t off, uint32_t n, std::vector<uint64_t>* cnt, std::vector<uint32_t>* mq) {
  const size_t nH = ctx->S.nH;
  cnt->assign((size_t)N_CNT * n, 0);
  if (mq) mq->assign(n, 0);
  if (!n) return 0;
  if (ctx->S.tkind != SGN_TRAFFIC_PERIODIC) {  // (these kinds keep them in the cold lines)
    std::vector<HostRec> recs;
    if (int e = read_recs(ctx, off, n, &recs)) return e;
    for (uint32_t i = 0; i < n; i++) {
      (*cnt)[(size_t)N_SENT * n + i] = recs[i].n_sent;
      (*cnt)[(size_t)N_POPPED * n + i] = recs[i].n_popped;
      (*cnt)[(size_t)N_DELIVERED * n + i] = recs[i].n_delivered;
      if (mq) (*mq)[i] = recs[i].max_codel;
    }
    return 0;
  }
  for (int k = 0; k < N_CNT; k++)
    SGN_HIP(ctx, hipMemcpy(cnt->data() + (size_t)k * n, (const void*)(ctx->S.n_cnt + k * nH + off), (size_t)n * 8,
                           hipMemcpyDeviceToHost));
  if (mq) SGN_HIP(ctx, hipMemcpy(mq->data(), (const void*)(ctx->S.maxq + off), (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}
// the cold lines hold the host's queue state (else it is an idle host's: empty queues)
inline bool cold_valid(const sgn_ctx* ctx, const HostRec& r) {
  return ctx->S.tkind != SGN_TRAFFIC_PERIODIC || (r.flags & F_COLD);
}
}  // namespace

int sgn_stats_get(sgn_ctx* ctx, sgn_stats* out) {
  if (!ctx || !out) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  int rc = sync_ctrl(ctx);
  const uint32_t nH = ctx->S.nH;
  std::vector<HostRec> recs;
  std::vector<uint64_t> cnt;
  std::vector<uint32_t> mq;
  if (int e = read_recs(ctx, 0, nH, &recs)) return e;
  if (int e = read_counts(ctx, 0, nH, &cnt, &mq)) return e;
  sgn_stats s{};
  uint64_t mc = 0;
  for (uint32_t h = 0; h < nH; h++) {
    const HostRec& r = recs[h];
    s.packets_sent += cnt[(size_t)N_SENT * nH + h];
    s.packets_unknown_dst += r.n_unknown;
    s.packet_events_popped += cnt[(size_t)N_POPPED * nH + h];
    s.codel_dropped += r.n_codel;
    s.delivered += cnt[(size_t)N_DELIVERED * nH + h];
    s.local_delivered += r.n_local_deliv;
    s.app_blocked += r.n_blocked;
    mc = std::max<uint64_t>(mc, mq[h]);
  }
  s.rounds = ctx->h_ctrl->rounds;
  s.min_used_latency_ns = ctx->h_ctrl->min_used;
  s.max_codel_len = mc;

  {
    const size_t G = ctx->S.G;
    std::vector<uint64_t> wc(W_N * G);
    SGN_HIP(ctx, hipMemcpy(wc.data(), (const void*)ctx->S.w_cnt, wc.size() * 8, hipMemcpyDeviceToHost));
    uint64_t acc[W_N] = {};
    for (int k = 0; k < W_N; k++)
      for (size_t g = 0; g < G; g++)
        acc[k] = k == W_MAXFILL ? std::max(acc[k], wc[k * G + g]) : acc[k] + wc[k * G + g];
    s.max_pending_events = acc[W_MAXFILL];
    s.host_executions = acc[W_EXEC];
    s.event_runs = acc[W_RUNS];
    s.sched_sorted_segments = acc[W_SORTED];
    s.packets_loss_dropped = acc[W_LOSS];
    s.local_events = acc[W_LOCAL_EV];
    s.bytes_delivered = acc[W_BYTES];
  }
  s.sched_heavy_hosts = 0;
  *out = s;
  return rc;
}

int sgn_host_digests(sgn_ctx* ctx, uint32_t lo, uint32_t hi, sgn_host_digest* out) {
  if (!ctx || !out) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (lo < ctx->lo || hi > ctx->hi || lo > hi) return set_error(ctx, SGN_EINVAL, "range outside the owned shard");
  if (int e = rng_release(ctx)) return e;
  int rc = sync_ctrl(ctx);
  const uint32_t n = hi - lo;
  // the range's hosts sit in permuted slots: read the slots they span
  uint32_t smin = ctx->hi, smax = ctx->lo;
  for (uint32_t i = lo; i < hi; i++) {
    smin = std::min(smin, ctx->sid_of[i]);
    smax = std::max(smax, ctx->sid_of[i]);
  }
  std::vector<HostRec> recs;
  std::vector<uint64_t> cnt;
  const uint32_t ns = n ? smax - smin + 1 : 0;
  if (n) {
    if (int e = read_recs(ctx, smin - ctx->lo, ns, &recs)) return e;
    if (int e = read_counts(ctx, smin - ctx->lo, ns, &cnt, nullptr)) return e;
  }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t j = ctx->sid_of[lo + i] - smin;
    const HostRec& r = recs[j];
    sgn_host_digest& o = out[i];
    o.tx = r.dig[0];
    o.rx = r.dig[1];
    o.app = r.dig[2];
    for (int k = 0; k < 4; k++) o.rng[k] = r.rng[k];
    o.next_event_id = r.eid;
    o.n_sent = cnt[(size_t)N_SENT * ns + j];
    o.n_popped = cnt[(size_t)N_POPPED * ns + j];
    o.n_delivered = cnt[(size_t)N_DELIVERED * ns + j];
    o.n_codel_dropped = r.n_codel;
  }
  return rc;
}

namespace {
// Host::next_event_time for owned HostIds [lo, hi): two small kernels, one copy.
int next_event_times(sgn_ctx* ctx, uint32_t lo, uint32_t hi, uint64_t* out) {
  if (!ctx || (!out && hi > lo)) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (lo < ctx->lo || hi > ctx->hi || lo > hi) return set_error(ctx, SGN_EINVAL, "host range not owned by this shard");
  int rc = sync_ctrl(ctx);
  if (rc) return rc;
  const uint32_t n = hi - lo;
  if (n == 0) return 0;
  const DevSim& S = ctx->S;
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  uint64_t* d = nullptr;
  SGN_HIP(ctx, hipMalloc(&d, (size_t)n * 8));
  // the groups holding the range's slots: one host's group, or all of them
  uint32_t g0 = 0, ng = S.G;
  if (n == 1) {
    g0 = (ctx->sid_of[lo] - ctx->lo) >> S.gsh;
    ng = 1;
  }
  launch_k_next_local(ctx->stream, (const DevSim*)ctx->d_S, lo, n, d);
  launch_k_next_packet(ctx->stream, S.NB, (const DevSim*)ctx->d_S, lo, n, g0, ng, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  hipFree(d);
  if (e != hipSuccess) return hip_fail(ctx, e, "next event times");
  return 0;
}
}  // namespace

int sgn_host_next_event_time(sgn_ctx* ctx, uint32_t host, uint64_t* t) {
  if (!ctx || !t) return SGN_EINVAL;
  return next_event_times(ctx, host, host + 1, t);
}

int sgn_hosts_next_event_time(sgn_ctx* ctx, uint32_t host_lo, uint32_t host_hi, uint64_t* out) {
  return next_event_times(ctx, host_lo, host_hi, out);
}

int sgn_trace_read(sgn_ctx* ctx, sgn_trace_rec* out, uint64_t cap, uint64_t* n_total) {
  if (!ctx) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  int rc = sync_ctrl(ctx);
  // (the records still in the buffer: all of them until the first sgn_trace_take)
  const uint64_t n = trace_held(ctx, ctx->h_ctrl->trace_n);
  if (n_total) *n_total = ctx->h_ctrl->trace_n;
  const uint64_t k = std::min(n, cap);
  if (k && out) SGN_HIP(ctx, hipMemcpy(out, ctx->trace_buf, k * sizeof(sgn_trace_rec), hipMemcpyDeviceToHost));
  return rc;
}

int sgn_engine_info_get(sgn_ctx* ctx, sgn_engine_info* out) {
  if (!ctx || !out) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  const DevSim& S = ctx->S;
  out->calendar_buckets = S.NB;
  out->bucket_width_ns = S.BW;
  out->host_groups = S.G;
  out->slab_capacity = S.CAP;
  out->hosts_per_wave = 1u << S.gsh;
  out->persistent_grid = ctx->persist_grid;
  out->persistent_fallbacks = ctx->persist_fallbacks;
  out->device_bytes = ctx->sim_bytes;
  out->exchange_slot_runs = ctx->nranks > 1 ? ctx->xslot : 0;
  out->exchange_send_runs = ctx->xsz_cur;
  out->exchange_hwm_runs = ctx->h_ctrl ? ctx->h_ctrl->xhwm : 0;
  out->exchange_spills = ctx->x_spills;
  out->exchange_bytes = ctx->x_bytes;
  out->codel_pages = ctx->S.cq_pages;
  // the control block as is (an overflow is reported by the calls that run rounds, not here)
  SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SGN_HIP(ctx, hipMemcpy(ctx->h_ctrl, (const void*)ctx->S.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost));
  const Ctrl& c = *ctx->h_ctrl;
  out->codel_page_allocs = ctx->counters.codel_allocs_before + c.pg_alloc;
  out->codel_pages_free = c.pg_tail >= c.pg_alloc ? c.pg_tail - c.pg_alloc : 0;
  std::vector<HostRec> recs;
  if (int e = read_recs(ctx, 0, ctx->S.nH, &recs)) return e;
  uint64_t chained = 0;
  for (const HostRec& r : recs) {
    const uint32_t nr = cold_valid(ctx, r) ? r.cq_nr : 0;
    chained += nr == 0 ? 1 : ((r.cq_head & (CQ_PAGE - 1)) + nr + CQ_PAGE - 1) / CQ_PAGE;
  }
  out->codel_pages_chained = chained;
  int ncu = 0;
  SGN_HIP(ctx, hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  out->compute_units = (uint64_t)ncu;
  out->bucket_min_lds = ctx->S.agg_bmin;
  out->lds_per_cu = ctx->lds_per_cu;
  out->codel_pool_grows = ctx->counters.codel_grows;
  out->calendar_grows = ctx->counters.cal_grows;
  out->calendar_spill_runs = ctx->counters.cal_spill_runs;
  out->exchange_slot_grows = ctx->xslot_grows;
  out->rounds_held = ctx->counters.rounds_held;
  out->slab_extensions = ctx->counters.ext_slabs;
  out->slab_extension_runs = ctx->S.ext_total;
  {
    const size_t G = ctx->S.G;
    std::vector<uint64_t> wb(G);
    SGN_HIP(ctx, hipMemcpy(wb.data(), (const void*)(ctx->S.w_cnt + W_BIG * G), G * 8, hipMemcpyDeviceToHost));
    uint64_t t = 0;
    for (uint64_t v : wb) t += v;
    out->big_slab_pieces = t;
  }
  out->spill_area_runs = ctx->S.spill_cap;
  out->spill_area_grows = ctx->counters.spill_grows;
  out->exchange_mode = ctx->nranks > 1 ? ctx->x_mode : 0;
  out->inbox_slot_runs = ctx->nranks > 1 ? ctx->S.xislot : 0;
  out->inbox_grows = ctx->x_grows;
  out->inbox_overflow_rounds = ctx->x_over_rounds;
  out->inbox_moved_runs = ctx->x_moved;
  out->persistent_x_launches = ctx->x_launches;
  out->persistent_x_grid = ctx->x_grid;
  return 0;
}

int sgn_kernel_times_get(sgn_ctx* ctx, sgn_kernel_times* out) {
  if (!ctx || !out) return SGN_EINVAL;
  if (ctx->sim_ready) {
    int rc = sync_ctrl(ctx);
    if (rc) return rc;
  }
  std::memset(out, 0, sizeof(*out));
  out->n_kernels = K_NUM;
  for (int i = 0; i < K_NUM; i++) {
    out->launches[i] = ctx->kt[i].launches;
    out->launches_total[i] = ctx->kt[i].total;
    out->ms[i] = ctx->kt[i].ms;
    out->name[i] = kKernelNames[i];
  }
  // the round kernel's slot: persistent launches (many rounds each) when enabled
  if (ctx->persist_grid) out->name[K_EXECUTE] = "k_rounds";
  if (ctx->x_mode == 2) out->name[K_EXECUTE] = "k_rounds_x";
  return 0;
}

// Diagnostics: per-wave {cycles, events, max lane events, busy lanes} of the last k_execute
// (allocated when SGN_STAMPS=1 is set in the environment at sgn_sim_init).
// Diagnostics of the last persistent launch (SGN_STAMPS=2): per round {earliest start, latest
// arrival, round edge done} (100 MHz clock), 128 rounds; resets the buffer for the next launch.
int sgn_debug_rounds(sgn_ctx* ctx, uint64_t* out) {
  if (!ctx || !ctx->sim_ready || !ctx->S.rdbg) return SGN_EINVAL;
  SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SGN_HIP(ctx, hipMemcpy(out, (const void*)ctx->S.rdbg, 3 * 128 * 8, hipMemcpyDeviceToHost));
  std::vector<uint64_t> init(3 * 128, 0);
  for (int r = 0; r < 128; r++) init[3 * r] = ~0ULL;
  SGN_HIP(ctx, hipMemcpy((void*)ctx->S.rdbg, init.data(), init.size() * 8, hipMemcpyHostToDevice));
  return 0;
}

// The same for k_rounds_x: per round 8 words (see the kernel's stamps), 128 rounds; resets.
int sgn_debug_rounds_x(sgn_ctx* ctx, uint64_t* out) {
  if (!ctx || !ctx->sim_ready || !ctx->S.rdbg) return SGN_EINVAL;
  SGN_HIP(ctx, hipDeviceSynchronize());
  SGN_HIP(ctx, hipMemcpy(out, (const void*)ctx->S.rdbg, 8 * 128 * 8, hipMemcpyDeviceToHost));
  std::vector<uint64_t> init(8 * 128, 0);
  for (int r = 0; r < 128; r++) init[8 * r] = ~0ULL;
  SGN_HIP(ctx, hipMemcpy((void*)ctx->S.rdbg, init.data(), init.size() * 8, hipMemcpyHostToDevice));
  return 0;
}

// k_rounds_x with SGN_STAMPS=3: every workgroup's stamps, [128 rounds][2048 workgroups][8]
// (this shard's workgroup index; unwritten: 0); resets.
int sgn_debug_rounds_xw(sgn_ctx* ctx, uint64_t* out) {
  if (!ctx || !ctx->sim_ready || !ctx->S.rdbg || !ctx->S.rdbg_wg) return SGN_EINVAL;
  const size_t n = (size_t)8 * 128 * 2048;
  SGN_HIP(ctx, hipDeviceSynchronize());
  SGN_HIP(ctx, hipMemcpy(out, (const void*)ctx->S.rdbg, n * 8, hipMemcpyDeviceToHost));
  SGN_HIP(ctx, hipMemset((void*)ctx->S.rdbg, 0, n * 8));
  return 0;
}

int sgn_debug_stamps(sgn_ctx* ctx, uint64_t* out, uint64_t cap, uint64_t* n) {
  if (!ctx || !ctx->sim_ready) return SGN_EINVAL;
  const uint64_t waves = ctx->S.G;
  if (n) *n = ctx->S.stamps ? waves : 0;
  if (!ctx->S.stamps || !out) return 0;
  SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SGN_HIP(ctx, hipMemcpy(out, ctx->S.stamps, std::min(cap, waves) * SGN_STAMP_WORDS * 8, hipMemcpyDeviceToHost));
  return 0;
}

// ---- CPU-resident applications (SGN_TRAFFIC_EXTERNAL) ----
int sgn_submit(sgn_ctx* ctx, const sgn_pkt_soa* b) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  if (!ctx || !b) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  const DevSim& S = ctx->S;
  if (S.tkind != SGN_TRAFFIC_EXTERNAL)
    return set_error(ctx, SGN_ESTATE, "sgn_submit needs SGN_TRAFFIC_EXTERNAL traffic");
  if (b->n == 0) return 0;
  if (!b->src_host || !b->dst_ip || !b->payload_len || !b->send_time)
    return set_error(ctx, SGN_EINVAL, "sgn_submit: missing array");
  int rc = sync_ctrl(ctx);
  if (rc) return rc;
  const uint64_t ws = ctx->h_ctrl->ws;
  // the calendar holds NB buckets of BW ns; the gather walks forward from the window
  const uint64_t horizon = ws + (uint64_t)(S.NB - 2) * S.BW;
  if (ctx->handles.size() + b->n > SGN_TAG_SLOT_MASK)
    return set_error(ctx, SGN_ERANGE, "more than 2^29 submissions on one shard");
  std::vector<EvRec> recs(b->n);
  std::vector<uint32_t> seq_add;
  std::vector<uint32_t> seq = ctx->submit_seq;  // committed only on success
  for (uint64_t i = 0; i < b->n; i++) {
    const uint32_t src = b->src_host[i];
    const uint64_t t = b->send_time[i];
    const uint32_t pay = b->payload_len[i];
    if (src < ctx->lo || src >= ctx->hi)
      return set_error(ctx, SGN_EINVAL, "sgn_submit: source host " + std::to_string(src) + " not owned by this shard");
    if (t < ws || t >= S.end_time)
      return set_error(ctx, SGN_EINVAL, "sgn_submit: send_time outside [window start, stop time)");
    if (t >= horizon)
      return set_error(ctx, SGN_EINVAL, "sgn_submit: send_time beyond the event calendar's horizon; submit it closer to its window");
    if (pay > 0xFFFFu) return set_error(ctx, SGN_EINVAL, "sgn_submit: payload_len > 65535");
    uint32_t hdr = 0;
    if (b->wire_len && b->wire_len[i] != 0) {
      const uint32_t w = b->wire_len[i];
      if (w == pay + SGN_UDP_HEADER_BYTES) hdr = 0;
      else if (w == pay + SGN_TCP_HEADER_BYTES) hdr = SGN_TAG_HDR_TCP;
      else if (w == pay + SGN_TCP_WS_HEADER_BYTES) hdr = SGN_TAG_HDR_TCPWS;
      else
        return set_error(ctx, SGN_EINVAL,
                         "sgn_submit: wire_len must be payload_len + 28 (UDP/IPv4), + 40 or + 44 (TCP/IPv4)");
    }
    uint32_t& q = seq[src - ctx->lo];
    if (q == 0xFFFFFFFFu) return set_error(ctx, SGN_ERANGE, "sgn_submit: 2^32 submissions from one host");
    EvRec& r = recs[i];
    r.time = t;
    r.eid = ((uint64_t)q++ << 32) | b->dst_ip[i];  // submission order, then the address
    r.src = src;
    r.dst = ctx->sid_of[src];  // filed in the source's own slot
    r.pc = pay | (1u << 16);
    r.tag = SGN_TAG_EXT | hdr | (uint32_t)(ctx->handles.size() + i);
  }
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->stage_cap < b->n) {
    if (ctx->d_stage) hipFree(ctx->d_stage);
    ctx->d_stage = nullptr;
    ctx->stage_cap = 0;
    SGN_HIP(ctx, hipMalloc(&ctx->d_stage, b->n * sizeof(EvRec)));
    ctx->stage_cap = b->n;
  }
  SGN_HIP(ctx, hipMemcpyAsync(ctx->d_stage, recs.data(), b->n * sizeof(EvRec), hipMemcpyHostToDevice, ctx->stream));
  launch_k_inject(ctx->stream, (const DevSim*)ctx->d_S, (const EvRec*)ctx->d_stage, (uint32_t)b->n);
  SGN_HIP(ctx, hipGetLastError());
  // the runs are in the device calendar from here: a failure past this point leaves them there
  // with no handle, so the context is marked unusable (a retry would file them twice)
  rc = sync_ctrl(ctx);
  if (!rc && ctx->h_ctrl->spill_n) rc = relayout_calendar(ctx);
  if (rc) {
    ctx->failed = std::string("sgn_submit failed after filing its runs: ") + sgn_last_error(ctx);
    return rc;
  }
  for (uint64_t i = 0; i < b->n; i++) ctx->handles.push_back(b->handle ? b->handle[i] : 0);
  ctx->submit_seq.swap(seq);
  return 0;
}

// ---- per-thread staging: stages are plain host buffers; one flush submits all
int sgn_stage_create(sgn_ctx* ctx, sgn_stage** out) {
  if (!ctx || !out) return SGN_EINVAL;
  sgn_stage* st = new sgn_stage();
  st->ctx = ctx;
  std::lock_guard<std::mutex> g(ctx->stage_mu);
  ctx->stages.push_back(st);
  *out = st;
  return 0;
}

void sgn_stage_destroy(sgn_stage* st) {
  if (!st) return;
  if (st->ctx) {
    std::lock_guard<std::mutex> g(st->ctx->stage_mu);
    auto& v = st->ctx->stages;
    v.erase(std::remove(v.begin(), v.end(), st), v.end());
  }
  delete st;
}

int sgn_stage_push(sgn_stage* st, const sgn_pkt_soa* b) {
  if (!st || !b) return SGN_EINVAL;
  if (b->n == 0) return 0;
  if (!b->src_host || !b->dst_ip || !b->payload_len || !b->send_time) return SGN_EINVAL;
  for (uint64_t i = 0; i < b->n; i++) {
    if (b->payload_len[i] > 0xFFFFu) return SGN_EINVAL;
    if (b->wire_len && b->wire_len[i] != 0) {
      const uint32_t w = b->wire_len[i], p = b->payload_len[i];
      if (w != p + SGN_UDP_HEADER_BYTES && w != p + SGN_TCP_HEADER_BYTES && w != p + SGN_TCP_WS_HEADER_BYTES)
        return SGN_EINVAL;
    }
  }
  std::lock_guard<std::mutex> g(st->mu);  // (uncontended except against a concurrent flush)
  st->src.insert(st->src.end(), b->src_host, b->src_host + b->n);
  st->dst.insert(st->dst.end(), b->dst_ip, b->dst_ip + b->n);
  st->pay.insert(st->pay.end(), b->payload_len, b->payload_len + b->n);
  st->time.insert(st->time.end(), b->send_time, b->send_time + b->n);
  for (uint64_t i = 0; i < b->n; i++) st->handle.push_back(b->handle ? b->handle[i] : 0);
  for (uint64_t i = 0; i < b->n; i++) st->wire.push_back(b->wire_len ? b->wire_len[i] : 0);
  return 0;
}

uint64_t sgn_stage_pending(const sgn_stage* st) {
  if (!st) return 0;
  std::lock_guard<std::mutex> g(st->mu);
  return st->src.size();
}

int sgn_stage_flush(sgn_ctx* ctx) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  if (!ctx) return SGN_EINVAL;
  std::vector<uint32_t> src, dst, pay, wire;
  std::vector<uint64_t> time, handle;
  // each stage's size at copy time: only that prefix is cleared after the submit, so a push
  // that lands while the flush runs stays staged for the next flush
  std::vector<std::pair<sgn_stage*, size_t>> taken;
  {
    std::lock_guard<std::mutex> g(ctx->stage_mu);
    for (sgn_stage* st : ctx->stages) {
      std::lock_guard<std::mutex> sg(st->mu);
      taken.push_back({st, st->src.size()});
      wire.insert(wire.end(), st->wire.begin(), st->wire.end());
      src.insert(src.end(), st->src.begin(), st->src.end());
      dst.insert(dst.end(), st->dst.begin(), st->dst.end());
      pay.insert(pay.end(), st->pay.begin(), st->pay.end());
      time.insert(time.end(), st->time.begin(), st->time.end());
      handle.insert(handle.end(), st->handle.begin(), st->handle.end());
    }
  }
  if (src.empty()) return 0;
  sgn_pkt_soa b{src.size(), src.data(), dst.data(), pay.data(), wire.data(), time.data(), handle.data()};
  if (int rc = sgn_submit(ctx, &b)) return rc;
  std::lock_guard<std::mutex> g(ctx->stage_mu);
  for (auto& t : taken) {
    sgn_stage* st = t.first;
    if (std::find(ctx->stages.begin(), ctx->stages.end(), st) == ctx->stages.end()) continue;  // destroyed meanwhile
    std::lock_guard<std::mutex> sg(st->mu);
    const size_t k = t.second;
    st->src.erase(st->src.begin(), st->src.begin() + k);
    st->dst.erase(st->dst.begin(), st->dst.begin() + k);
    st->pay.erase(st->pay.begin(), st->pay.begin() + k);
    st->time.erase(st->time.begin(), st->time.begin() + k);
    st->handle.erase(st->handle.begin(), st->handle.begin() + k);
    st->wire.erase(st->wire.begin(), st->wire.begin() + k);
  }
  return 0;
}

int sgn_drain(sgn_ctx* ctx, uint32_t lo, uint32_t hi, sgn_drain_rec* out, uint64_t cap, uint64_t* n_out) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  if (!ctx || (!out && cap)) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (ctx->S.tkind != SGN_TRAFFIC_EXTERNAL)
    return set_error(ctx, SGN_ESTATE, "sgn_drain needs SGN_TRAFFIC_EXTERNAL traffic");
  int rc = sync_ctrl(ctx);
  if (rc) return rc;
  const uint64_t n = ctx->h_ctrl->drain_n;
  if (n) {
    const size_t old = ctx->drain_held.size();
    ctx->drain_held.resize(old + n);
    SGN_HIP(ctx, hipMemcpy(ctx->drain_held.data() + old, (const void*)ctx->S.drain, n * sizeof(sgn_drain_rec),
                           hipMemcpyDeviceToHost));
    const uint64_t zero = 0;
    SGN_HIP(ctx, hipMemcpy((char*)ctx->S.ctrl + offsetof(Ctrl, drain_n), &zero, 8, hipMemcpyHostToDevice));
    ctx->h_ctrl->drain_n = 0;
    for (size_t i = old; i < ctx->drain_held.size(); i++) {
      sgn_drain_rec& r = ctx->drain_held[i];
      const uint32_t slot = r.tag & SGN_TAG_SLOT_MASK;
      // a slot is this shard's when the datagram's source is one of its hosts
      r.handle = ((r.tag & SGN_TAG_EXT) && r.src_host >= ctx->lo && r.src_host < ctx->hi &&
                  slot < ctx->handles.size()) ? ctx->handles[slot] : 0;
    }
  }
  std::vector<sgn_drain_rec> sel, keep;
  for (const sgn_drain_rec& r : ctx->drain_held) (r.host >= lo && r.host < hi ? sel : keep).push_back(r);
  auto key = [](const sgn_drain_rec& r) {
    return std::make_tuple(r.host, r.time, r.src_host, r.src_eid, r.tag, r.status);
  };
  std::sort(sel.begin(), sel.end(), [&](const sgn_drain_rec& a, const sgn_drain_rec& b) { return key(a) < key(b); });
  const uint64_t k = std::min<uint64_t>(cap, sel.size());
  if (k) std::memcpy(out, sel.data(), k * sizeof(sgn_drain_rec));
  keep.insert(keep.end(), sel.begin() + k, sel.end());
  ctx->drain_held.swap(keep);
  if (n_out) *n_out = k;
  return 0;
}

namespace {
// rand_xoshiro 0.7.0 Xoshiro256PlusPlus::next_u64 on the CPU (a CPU-held host state)
inline uint64_t host_xoshiro_next(uint64_t* s) {
  auto rotl = [](uint64_t x, int k) { return (x << k) | (x >> (64 - k)); };
  const uint64_t r = rotl(s[0] + s[3], 23) + s[0], t = s[1] << 17;
  s[2] ^= s[0];
  s[3] ^= s[1];
  s[1] ^= s[2];
  s[0] ^= s[3];
  s[2] ^= t;
  s[3] = rotl(s[3], 45);
  return r;
}
// n single draws of one owned host on the CPU: the first draw after a device operation reads
// the state (one 32-byte copy); later ones are a few nanoseconds each
int rng_cpu_draws(sgn_ctx* ctx, uint32_t host, uint64_t n, uint64_t* out) {
  if (!ctx) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (host < ctx->lo || host >= ctx->hi) return set_error(ctx, SGN_EINVAL, "host not owned by this shard");
  const uint32_t slot = ctx->sid_of[host] - ctx->lo;
  auto it = ctx->rng_held.find(slot);
  if (it == ctx->rng_held.end()) {
    sgn_ctx::RngHeld h{};
    SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->S.htile) {
      SGN_HIP(ctx, hipMemcpy(h.s, (const void*)(ctx->S.htile + 2 * hot_idx(slot, 0)), 16, hipMemcpyDeviceToHost));
      SGN_HIP(ctx, hipMemcpy(h.s + 2, (const void*)(ctx->S.htile + 2 * hot_idx(slot, 1)), 16, hipMemcpyDeviceToHost));
    } else {
      SGN_HIP(ctx, hipMemcpy(h.s, (const void*)(ctx->S.hrec + slot), 32, hipMemcpyDeviceToHost));
    }
    it = ctx->rng_held.emplace(slot, h).first;
  }
  for (uint64_t i = 0; i < n; i++) out[i] = host_xoshiro_next(it->second.s);
  it->second.draws += n;
  return 0;
}
// counts[i] draws from each of n distinct owned hosts, concatenated in order into out
int rng_draws(sgn_ctx* ctx, const uint32_t* hosts, const uint32_t* counts, uint32_t n, uint64_t* out) {
  if (!ctx || (n && (!hosts || !counts))) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  std::vector<uint32_t> loc(n);
  std::vector<uint64_t> off(n);
  uint64_t total = 0;
  std::vector<uint32_t> seen;
  for (uint32_t i = 0; i < n; i++) {
    if (hosts[i] < ctx->lo || hosts[i] >= ctx->hi) return set_error(ctx, SGN_EINVAL, "host not owned by this shard");
    loc[i] = ctx->sid_of[hosts[i]] - ctx->lo;  // the host's slot
    off[i] = total;
    total += counts[i];
    seen.push_back(hosts[i]);
  }
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
    return set_error(ctx, SGN_EINVAL, "sgn_rng_next_u64_batch: hosts must be distinct");
  if (total && !out) return SGN_EINVAL;
  if (n == 0) return 0;
  if (int rc = rng_release(ctx)) return rc;
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  char* d = nullptr;
  const size_t bytes = (size_t)n * (4 + 4 + 8) + total * 8 + 16;
  SGN_HIP(ctx, hipMalloc(&d, bytes));
  uint32_t* dh = (uint32_t*)d;
  uint32_t* dc = dh + n;
  uint64_t* doff = (uint64_t*)(d + ((size_t)n * 8 + 7) / 8 * 8);
  uint64_t* dout = doff + n;
  hipError_t e = hipMemcpyAsync(dh, loc.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dc, counts, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(doff, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_k_rng(ctx->stream, (const DevSim*)ctx->d_S, dh, dc, doff, n, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess && total) e = hipMemcpyAsync(out, dout, total * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  hipFree(d);
  if (e != hipSuccess) return hip_fail(ctx, e, "host rng draws");
  return 0;
}
int rng_draw(sgn_ctx* ctx, uint32_t host, uint32_t n, uint64_t* out) {
  return rng_cpu_draws(ctx, host, n, out);
}
}  // namespace

int sgn_rng_next_u64_batch(sgn_ctx* ctx, const uint32_t* hosts, const uint32_t* counts, uint32_t n,
                           uint64_t* out) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  return rng_draws(ctx, hosts, counts, n, out);
}

int sgn_rng_next_u64(sgn_ctx* ctx, uint32_t host, uint64_t* out) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  return rng_draw(ctx, host, 1, out);
}

int sgn_rng_double(sgn_ctx* ctx, uint32_t host, double* out) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  if (!out) return SGN_EINVAL;
  uint64_t x = 0;
  int rc = rng_draw(ctx, host, 1, &x);
  if (rc == 0) *out = (double)(x >> 11) * 0x1.0p-53;
  return rc;
}

int sgn_rng_fill_bytes(sgn_ctx* ctx, uint32_t host, uint8_t* buf, size_t len) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  if (!buf && len) return SGN_EINVAL;
  if (len / 8 + 1 > 0xFFFFFFFFull) return set_error(ctx, SGN_ERANGE, "sgn_rng_fill_bytes: len too large");
  const size_t full = len / 8, rem = len % 8;
  std::vector<uint64_t> v(full + (rem ? 1 : 0));
  int rc = rng_draw(ctx, host, (uint32_t)v.size(), v.data());
  if (rc) return rc;
  for (size_t i = 0; i < full; i++)
    for (int k = 0; k < 8; k++) buf[8 * i + k] = (uint8_t)(v[i] >> (8 * k));
  if (rem) {
    // fill_bytes_via_next: 5..7 bytes from next_u64, 1..4 from next_u32 = next_u64 >> 32
    const uint64_t w = rem > 4 ? v[full] : (v[full] >> 32);
    for (size_t k = 0; k < rem; k++) buf[8 * full + k] = (uint8_t)(w >> (8 * k));
  }
  return 0;
}

// Test hook: device CoDel control-law increments for count in [0, n).
int sgn_selftest_codel_law(sgn_ctx* ctx, uint64_t n, uint64_t* out) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  if (!ctx || !out) return SGN_EINVAL;
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  uint64_t* d = nullptr;
  SGN_HIP(ctx, hipMalloc(&d, n * 8));
  launch_k_codel_law_test(ctx->stream, n, d);
  hipError_t e = hipMemcpyAsync(out, d, n * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  hipFree(d);
  if (e != hipSuccess) return hip_fail(ctx, e, "codel law selftest");
  return 0;
}

}  // extern "C"

namespace sgn {
// The CPU-held states go back before anything on the device uses a host RNG (rounds, batch
// draws, digests): one small upload and one kernel, stream-ordered (no host wait).
int rng_release(sgn_ctx* ctx) {
  if (ctx->rng_held.empty() || !ctx->sim_ready) {
    ctx->rng_held.clear();
    return 0;
  }
  std::vector<uint64_t> st;
  st.reserve(ctx->rng_held.size() * 6);
  for (auto& kv : ctx->rng_held) {
    if (!kv.second.draws) continue;
    st.push_back(kv.first);
    for (int k = 0; k < 4; k++) st.push_back(kv.second.s[k]);
    st.push_back(kv.second.draws);
  }
  ctx->rng_held.clear();
  const uint32_t n = (uint32_t)(st.size() / 6);
  if (!n) return 0;
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->rng_stage_cap < st.size()) {
    if (ctx->d_rng_stage) hipFree(ctx->d_rng_stage);
    ctx->d_rng_stage = nullptr;
    ctx->rng_stage_cap = 0;
    SGN_HIP(ctx, hipMalloc(&ctx->d_rng_stage, st.size() * 8));
    ctx->rng_stage_cap = st.size();
  }
  SGN_HIP(ctx, hipMemcpyAsync(ctx->d_rng_stage, st.data(), st.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  launch_k_rng_set(ctx->stream, (const DevSim*)ctx->d_S, (const uint64_t*)ctx->d_rng_stage, n);
  SGN_HIP(ctx, hipGetLastError());
  SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the staging vector goes out of scope)
  return 0;
}

}  // namespace sgn

uint64_t sgn::layout_sig_interop() { return kLayoutSig; }
