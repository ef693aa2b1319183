// run.cpp — running rounds: which round kernel a simulation launches and how large (the table of
// engine.hip's launch surface, occupancy, the persistent grid), the control block on the host,
// launch timing and captured batches, the run loops of the C ABI (sgn_round, sgn_run,
// sgn_run_until, sgn_set_window) and the persistent multi-shard launches (k_rounds_x) with
// their held round edges. Host code only.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sgn_internal.h"

using namespace sgn;

namespace {

constexpr uint32_t kPersistRounds = 128;  // rounds per persistent launch (then a host sync)
constexpr uint64_t kTimeEvery = 8;        // per-round launches: one timed in kTimeEvery

// The round kernels of a simulation, from the one table (round_kernels): k_execute traced or
// lean; k_rounds' twin with the diagnostics when the simulation started with SGN_STAMPS set
// (DevSim::stamps, sgn_sim_init) — the same rule for the kernel that sizes the persistent grid
// and the kernel that is launched.
const void* execute_fn(const DevSim& S) { return round_kernels(S.tkind).execute[S.trace_on ? 1 : 0]; }
const void* rounds_fn(const DevSim& S, bool big) { return round_kernels(S.tkind).rounds[S.stamps ? 1 : 0][big ? 1 : 0]; }
// the persistent kernel with the big-slab path only while a slab can hold more than CAP runs
bool rounds_big(const sgn_ctx* ctx) { return ctx->counters.ext_slabs > 0; }
// the census verdict of the last persistent launch: 1 resident, 2 not (0: none recorded)
uint32_t census_verdict(const sgn_ctx* ctx, uint32_t epoch) {
  const uint32_t v = ctx->h_ctrl->res_verdict;
  return (v >> 2) == (epoch & 0x3FFFFFFFu) ? (v & 3u) : 0u;
}

int check_overflow(sgn_ctx* ctx) {
  const Ctrl& c = *ctx->h_ctrl;
  if (c.overflow == 0) return 0;
  std::string what;
  if (c.overflow & OVF_BUCKET) what += " calendar bucket (raise sgn_sim_config.event_capacity)";
  if (c.overflow & OVF_CODEL) what += " CoDel page pool (raise sgn_sim_config.codel_cap)";
  if (c.overflow & OVF_SEG) what += " due-event segment buffer";
  if (c.overflow & OVF_EXCHANGE) what += " exchange slot (raise exchange_slot_events)";
  if (c.overflow & OVF_TRACE) what += " trace buffer";
  if (c.overflow & OVF_TIMEOUT) what += " persistent grid barrier timed out (grid not resident)";
  if (c.overflow & OVF_HORIZON) what += " event calendar horizon (a delivery beyond the calendar's buckets)";
  if (c.overflow & OVF_DRAIN) what += " drain buffer (raise sgn_drain_enable's capacity or drain more often)";
  return set_error(ctx, SGN_EOVERFLOW,
                   "device capacity exceeded:" + what + " (info " +
                       std::to_string(c.overflow_info) + "); results are invalid");
}

// Resident workgroups of a round kernel on this GPU (0: unknown): the occupancy query,
// capped by LDS per CU (the device attribute: 160 KiB on gfx950) — LDS is allocated per
// workgroup in 512-byte granules (a 23184-byte workgroup fits 6 per CU, not 7: a grid sized
// for 7 was not resident and its barrier timed out)
uint64_t resident_wg(sgn_ctx* ctx, const void* fn, size_t dyn) {
  int occ = 0, ncu = 0, lds_cu = 0;
  hipFuncAttributes fa{};
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64, dyn) != hipSuccess ||
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess ||
      hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, ctx->device) != hipSuccess ||
      hipFuncGetAttributes(&fa, fn) != hipSuccess || occ <= 0 || ncu <= 0 || lds_cu <= 0)
    return 0;
  const size_t lds_wg = (fa.sharedSizeBytes + dyn + 511) / 512 * 512;
  ctx->lds_per_cu = (uint32_t)lds_cu;
  return (uint64_t)std::min<int>(occ, (int)((size_t)lds_cu / lds_wg)) * (uint64_t)ncu;
}

}  // namespace

namespace sgn {

// one round's k_execute: one wave per host group (a launch error is the caller's hipGetLastError)
void launch_execute(sgn_ctx* ctx) {
  const size_t lds = exec_lds_bytes(ctx->S.CAP, ctx->S.agg_bmin ? ctx->S.NB : 0);
  const DevSim* d = (const DevSim*)ctx->d_S;
  void* args[] = {&d};
  (void)hipLaunchKernel(execute_fn(ctx->S), dim3(ctx->S.G), dim3(64), args, lds, ctx->stream);
}
// k_import files the received runs and its last block advances the window
void launch_import(sgn_ctx* ctx) {
  launch_k_import(ctx->stream, ctx->S);
  if (!ctx->capturing) ctx->kt[K_IMPORT].total++;
}

// The largest slab capacity whose round-kernel LDS fits one workgroup (calendar re-layout).
uint32_t max_slab_capacity(sgn_ctx* ctx, const DevSim& S) {
  int per_block = 0;
  if (hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess ||
      per_block <= 0)
    per_block = 64 * 1024;
  size_t st = 0;
  for (const void* fn : {rounds_fn(S, false), rounds_fn(S, true), execute_fn(S)}) {
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, fn) == hipSuccess) st = std::max<size_t>(st, fa.sharedSizeBytes);
  }
  uint32_t cap = CAP_MIN;
  while (cap < (1u << 15) && st + exec_lds_bytes(cap * 2, S.NB) <= (size_t)per_block) cap *= 2;
  // test hook: a lower limit, so that hot slabs take extensions and the big-slab path at small sizes
  if (const char* e = getenv("SGN_SLAB_LIM")) cap = std::max<uint32_t>(16, std::min<uint32_t>(cap, (uint32_t)atoi(e)));
  return cap;
}

// The round kernels' shapes for the calendar as it is now (sim_init, and after a re-layout):
// the LDS table of bucket minima ((NB + 1) x 4 bytes per workgroup, flush_bmin) is used when
// it costs no resident workgroups where they count — the round kernels' grids stay as large
// (config C has no LDS to spare: its 1563 groups need 7 workgroups per CU), or the grid
// exceeds the chip either way (config D); SGN_AGG_BMIN=0/1 overrides — and the persistent
// grid (single shard): entirely resident, with workgroups looping over groups when G exceeds
// it. Persistent rounds keep the bucket -> slab table in LDS (each workgroup applies the
// round's swap itself), so they need NB <= LDS_BSLAB; longer calendars run one launch per
// round, and so does a traced run (k_rounds is built without the per-packet trace).
void size_round_kernels(sgn_ctx* ctx, DevSim& S) {
  const uint64_t G = S.G, NB = S.NB;
  bool agg = S.tkind == SGN_TRAFFIC_PERIODIC;  // the kernels fold in LDS for PERIODIC traffic (kAggBmin)
  for (const void* fn : {rounds_fn(S, false), rounds_fn(S, true), execute_fn(S)}) {
    const uint64_t r0 = resident_wg(ctx, fn, exec_lds_bytes(S.CAP)), r1 = resident_wg(ctx, fn, exec_lds_bytes(S.CAP, S.NB));
    if (!r0 || std::min<uint64_t>(G, r1) < std::min<uint64_t>(G, r0)) agg = false;
  }
  if (const char* e = getenv("SGN_AGG_BMIN")) agg = atoi(e) != 0;
  if ((NB + 1) * S.BW >= (1ULL << 32)) agg = false;  // offsets from the window start must fit u32
  S.agg_bmin = agg ? 1u : 0u;
  ctx->persist_grid = 0;
  if (ctx->nranks == 1 && NB <= LDS_BSLAB && !S.trace_on && !ctx->persist_off &&
      !(getenv("SGN_PERSISTENT") && atoi(getenv("SGN_PERSISTENT")) == 0)) {
    // (resident for either variant: a re-layout that adds slab extensions switches to kBig)
    const size_t lds = exec_lds_bytes(S.CAP, S.agg_bmin ? S.NB : 0);
    const uint64_t res = std::min(resident_wg(ctx, rounds_fn(S, false), lds), resident_wg(ctx, rounds_fn(S, true), lds));
    if (res) {
      ctx->persist_grid = (uint32_t)std::min<uint64_t>(G, res);
      // test hook: a smaller grid makes every workgroup serve several groups per round
      if (const char* e = getenv("SGN_PERSIST_GRID"))
        ctx->persist_grid = std::max<uint32_t>(1, std::min<uint32_t>(ctx->persist_grid, (uint32_t)atoi(e)));
      // test hook: an oversized grid (not resident) exercises the residency census fallback
      if (const char* e = getenv("SGN_PERSIST_GRID_FORCE")) ctx->persist_grid = (uint32_t)atoi(e);
    }
  }
  if (ctx->persist_grid > 64 * RB_CH) ctx->persist_grid = 64 * RB_CH;
}

int sync_ctrl(sgn_ctx* ctx) {
  if (!ctx->failed.empty()) return set_error(ctx, SGN_ESTATE, "simulation unusable: " + ctx->failed);
  SGN_HIP(ctx, hipMemcpyAsync(ctx->h_ctrl, ctx->S.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost,
                              ctx->stream));
  SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  time_collect(ctx);
  return check_overflow(ctx);
}

}  // namespace sgn

namespace {

// After a persistent launch of census epoch ep: its own copy of the control block when it wrote
// one (no device-to-host copy on the launch edge), else sync_ctrl.
int sync_ctrl_persist(sgn_ctx* ctx, uint32_t ep) {
  if (!ctx->failed.empty()) return set_error(ctx, SGN_ESTATE, "simulation unusable: " + ctx->failed);
  if (!ctx->h_mirror) return sync_ctrl(ctx);
  SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  constexpr size_t NW = sizeof(Ctrl) / 8;
  if (__atomic_load_n(&ctx->h_mirror[NW], __ATOMIC_ACQUIRE) != ep || ctx->h_mirror[kMirrorWords - 1])
    return sync_ctrl(ctx);
  std::memcpy(ctx->h_ctrl, ctx->h_mirror, sizeof(Ctrl));
  time_collect(ctx);
  return check_overflow(ctx);
}

// one persistent launch of up to n rounds (k_rounds, or its twin: rounds_fn)
void launch_k_rounds(sgn_ctx* ctx, uint32_t n) {
  const size_t lds = exec_lds_bytes(ctx->S.CAP, ctx->S.agg_bmin ? ctx->S.NB : 0);
  const DevSim* d = (const DevSim*)ctx->d_S;
  // (the census: this launch's epoch, and the arrivals of the launches before it)
  uint32_t ep = ++ctx->res_epoch, base = ctx->res_base;
  ctx->res_base += ctx->persist_grid;
  void* args[] = {&d, &n, &ep, &base};
  (void)hipLaunchKernel(rounds_fn(ctx->S, rounds_big(ctx)), dim3(ctx->persist_grid), dim3(64), args, lds, ctx->stream);
}

int launch_round(sgn_ctx* ctx) {
  // a multi-shard round needs its exchange transport before anything is launched
  if (ctx->nranks > 1 && !ctx->comm)
    return set_error(ctx, SGN_ESTATE, "multi-shard round without an RCCL communicator");
  // per-round launches time one round in kTimeEvery: an event record is a barrier packet
  // with a cache write-back, and around every launch it cost 20 % of the rounds (eager) or
  // 45 % (graph batches) on config C; a sample gives the kernel's average duration
  const bool timed = ctx->capturing || (ctx->t_seq++ % kTimeEvery) == 0;
  if (timed) time_begin(ctx, K_EXECUTE);
  launch_execute(ctx);
  if (timed) time_end(ctx);
  if (!ctx->capturing) ctx->kt[K_EXECUTE].total++;
  if (ctx->nranks > 1) {
    // exchange + import + local finalize + all-reduce(min) + advance (comm.cpp)
    int rc = comm_round_exchange(ctx);
    if (rc) return rc;
  } else {
    // single shard: k_execute's last wave runs the round edge (finalize_fused)
  }
  SGN_HIP(ctx, hipGetLastError());
  ctx->counters.rounds_enqueued++;
  return 0;
}

// Event-record nodes around the timed kernel nodes of a captured batch (a captured
// hipEventRecord yields no timing on ROCm 7.2; explicit record nodes do).
int add_timing_nodes(sgn_ctx* ctx, hipGraph_t g) {
  const bool all = ctx->flags & SGN_CREATE_TIME_KERNELS;
  const bool exec = ctx->flags & SGN_CREATE_TIME_EXECUTE;
  ctx->graph_timed.clear();
  if (!all && !exec) return 0;
  const void* fn[K_NUM] = {execute_fn(ctx->S), import_kernel()};
  size_t n = 0;
  SGN_HIP(ctx, hipGraphGetNodes(g, nullptr, &n));
  std::vector<hipGraphNode_t> nodes(n);
  SGN_HIP(ctx, hipGraphGetNodes(g, nodes.data(), &n));
  size_t ev = 0;
  uint32_t tseen[K_NUM] = {};
  for (hipGraphNode_t node : nodes) {
    hipGraphNodeType t;
    SGN_HIP(ctx, hipGraphNodeGetType(node, &t));
    if (t != hipGraphNodeTypeKernel) continue;
    hipKernelNodeParams p;
    SGN_HIP(ctx, hipGraphKernelNodeGetParams(node, &p));
    int kid = -1;
    for (int k = 0; k < K_NUM; k++)
      if (p.func == fn[k]) kid = k;
    if (kid < 0 || (!all && kid != K_EXECUTE)) continue;
    if ((tseen[kid]++ % kTimeEvery) != 0) continue;  // a sample (launch_round's note)
    if (ev >= ctx->ev_pool.size()) {
      hipEvent_t a, b;
      SGN_HIP(ctx, hipEventCreate(&a));
      SGN_HIP(ctx, hipEventCreate(&b));
      ctx->ev_pool.push_back({a, b});
    }
    size_t nd = 0, nn = 0;
    SGN_HIP(ctx, hipGraphNodeGetDependencies(node, nullptr, &nd));
    std::vector<hipGraphNode_t> deps(nd);
    if (nd) SGN_HIP(ctx, hipGraphNodeGetDependencies(node, deps.data(), &nd));
    SGN_HIP(ctx, hipGraphNodeGetDependentNodes(node, nullptr, &nn));
    std::vector<hipGraphNode_t> outs(nn);
    if (nn) SGN_HIP(ctx, hipGraphNodeGetDependentNodes(node, outs.data(), &nn));
    hipGraphNode_t a, b;
    SGN_HIP(ctx, hipGraphAddEventRecordNode(&a, g, nd ? deps.data() : nullptr, nd, ctx->ev_pool[ev].first));
    SGN_HIP(ctx, hipGraphAddDependencies(g, &a, &node, 1));
    SGN_HIP(ctx, hipGraphAddEventRecordNode(&b, g, &node, 1, ctx->ev_pool[ev].second));
    for (hipGraphNode_t o : outs) SGN_HIP(ctx, hipGraphAddDependencies(g, &b, &o, 1));
    ctx->graph_timed.push_back({kid, ev});
    ev++;
  }
  return 0;
}

}  // namespace

namespace sgn {

void time_begin(sgn_ctx* ctx, int kernel) {
  if (ctx->capturing) return;  // graph mode: event-record nodes are added after capture
  const bool all = ctx->flags & SGN_CREATE_TIME_KERNELS;
  const bool exec = (ctx->flags & SGN_CREATE_TIME_EXECUTE) && kernel == K_EXECUTE;
  if (!all && !exec) return;
  if (ctx->ev_next >= ctx->ev_pool.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    ctx->ev_pool.push_back({a, b});
  }
  hipEventRecord(ctx->ev_pool[ctx->ev_next].first, ctx->stream);
  ctx->ev_pending.push_back({kernel, ctx->ev_next});
}

void time_end(sgn_ctx* ctx) {
  if (ctx->capturing) return;
  if (!(ctx->flags & (SGN_CREATE_TIME_KERNELS | SGN_CREATE_TIME_EXECUTE))) return;
  if (ctx->ev_pending.empty() || ctx->ev_pending.back().second != ctx->ev_next) return;
  hipEventRecord(ctx->ev_pool[ctx->ev_next].second, ctx->stream);
  ctx->ev_next++;
}

void time_collect(sgn_ctx* ctx) {
  if (!(ctx->flags & (SGN_CREATE_TIME_KERNELS | SGN_CREATE_TIME_EXECUTE))) return;
  if (ctx->graph_pending) {
    // events recorded by the replayed graph's event-record nodes
    for (auto& p : ctx->graph_timed) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->ev_pool[p.second].first,
                              ctx->ev_pool[p.second].second) == hipSuccess) {
        ctx->kt[p.first].ms += ms;
        ctx->kt[p.first].launches++;
      }
    }
    ctx->graph_pending = false;
  }
  for (auto& p : ctx->ev_pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev_pool[p.second].first, ctx->ev_pool[p.second].second) ==
        hipSuccess) {
      ctx->kt[p.first].ms += ms;
      ctx->kt[p.first].launches++;
    }
  }
  ctx->ev_pending.clear();
  ctx->ev_next = 0;
}

void drop_graph(sgn_ctx* ctx) {
  if (ctx->gexec) hipGraphExecDestroy(ctx->gexec);
  if (ctx->graph) hipGraphDestroy(ctx->graph);
  ctx->gexec = nullptr;
  ctx->graph = nullptr;
  ctx->gbatch = 0;
  ctx->gsz = 0;
  ctx->graph_timed.clear();
  ctx->graph_pending = false;
}

// The persistent multi-shard path runs where the persistent kernel would (the bucket -> slab
// table in LDS, no per-packet trace) unless refused before or switched off (SGN_XPERSIST=0 or
// SGN_PERSISTENT=0: per-round launches and the RCCL / local-copy exchange).
bool xpersist_possible(sgn_ctx* ctx) {
  // (read per call, like the single-shard path's SGN_PERSISTENT: a test that changes either
  // variable within one process must see it — ADVICE r5)
  const bool off = (getenv("SGN_XPERSIST") && atoi(getenv("SGN_XPERSIST")) == 0) ||
                   (getenv("SGN_PERSISTENT") && atoi(getenv("SGN_PERSISTENT")) == 0);
  return ctx->nranks > 1 && ctx->nranks <= XR_MAX && ctx->sim_ready && ctx->xin_mem && ctx->S.NB <= LDS_BSLAB &&
         !ctx->S.trace_on &&
         !ctx->x_off && !ctx->persist_off && !off;
}

}  // namespace sgn

namespace {

// One k_rounds_x launch of up to n rounds over the shards sh (all on sh[0]'s GPU and stream).
// Returns 1 when no resident grid can be sized (the caller falls back to per-round launches).
int x_launch(const std::vector<sgn_ctx*>& sh, bool peers, uint32_t n) {
  sgn_ctx* c0 = sh[0];
  const void* fn = round_kernels(c0->S.tkind).rounds_x;
  size_t lds = 0;
  uint64_t sumG = 0;
  for (sgn_ctx* c : sh) {
    lds = std::max(lds, exec_lds_bytes(c->S.CAP, c->S.agg_bmin ? c->S.NB : 0));
    sumG += c->S.G;
  }
  const uint64_t res = resident_wg(c0, fn, lds) / std::max<uint32_t>(1, peers ? c0->x_share : 1);
  // A refusal is decided here, from this GPU's LDS and residency alone (CAP may differ between
  // shards after their re-layouts). A local group falls back at once; one shard per GPU must not,
  // or its peers would launch and wait for it: it launches ONE workgroup that publishes "not
  // resident" to every peer's census word, and every shard falls back together.
  bool refuse = !res || res < sh.size();
  // (test hook: this rank refuses as if its GPU could not hold the grid)
  if (peers && getenv("SGN_XREFUSE_RANK") && atoi(getenv("SGN_XREFUSE_RANK")) == (int)c0->rank) refuse = true;
  if (refuse && !peers) return 1;
  if (!c0->x_hxl) SGN_HIP(c0, hipHostMalloc(&c0->x_hxl, sizeof(XLaunch), 0));
  XLaunch& xl = *(XLaunch*)c0->x_hxl;
  std::memset(&xl, 0, sizeof(xl));
  xl.n_local = (uint32_t)sh.size();
  xl.peers_census = peers ? 1u : 0u;
  xl.refuse = refuse ? 1u : 0u;
  xl.epoch = ++c0->x_epoch;
  uint32_t b = 0;
  const char* cap_env = getenv("SGN_PERSIST_GRID");
  for (size_t i = 0; i < sh.size(); i++) {
    sgn_ctx* c = sh[i];
    uint64_t P = std::max<uint64_t>(1, std::min<uint64_t>(c->S.G, res * c->S.G / sumG));
    if (cap_env) P = std::max<uint64_t>(1, std::min<uint64_t>(P, (uint64_t)atoi(cap_env)));
    P = std::min<uint64_t>(P, 64 * RB_CH);
    if (refuse) P = 1;
    xl.base[i] = b;
    xl.S[i] = (std::remove_reference_t<decltype(xl.S[i])>)c->d_S;
    b += (uint32_t)P;
    c->x_grid = (uint32_t)P;
    const DevSim& S = c->S;
    (void)S;  // (no per-launch memsets: each shard's launch resets its round buffers itself)
  }
  xl.base[sh.size()] = b;
  xl.res_base = c0->res_base;  // (the census counts in the first shard's control block)
  if (!refuse) c0->res_base += b;  // (a refused launch runs no census)
  if (refuse) lds = 0;             // (its one workgroup leaves before touching the dynamic LDS)
  SGN_HIP(c0, hipMemcpyAsync(c0->d_xl, &xl, sizeof(XLaunch), hipMemcpyHostToDevice, c0->stream));
  time_begin(c0, K_EXECUTE);
  const XLaunch* d = (const XLaunch*)c0->d_xl;
  void* args[] = {&d, &n};
  (void)hipLaunchKernel(fn, dim3(b), dim3(64), args, lds, c0->stream);
  time_end(c0);
  c0->kt[K_EXECUTE].total++;
  SGN_HIP(c0, hipGetLastError());
  for (sgn_ctx* c : sh) {
    c->x_launches++;
    c->x_mode = 2;
  }
  return 0;
}

// A round edge held by k_rounds_x (every shard the same flags): runs past an inbox slot go from
// the senders' spill areas into their shards' calendars, and the inboxes grow; then each shard's
// own pools (resolve_hold). sh: every shard of the group (local) or this GPU's one (peers).
int x_resolve(const std::vector<sgn_ctx*>& sh, bool peers) {
  uint32_t hold = 0;
  uint64_t hwm = 0;
  for (sgn_ctx* c : sh) {
    hold |= c->h_ctrl->hold;
    hwm = std::max<uint64_t>(hwm, c->h_ctrl->xhwm);
  }
  const uint32_t xf = HOLD_XSLOT | HOLD_XGROW;
  if (!(hold & xf)) {
    for (sgn_ctx* c : sh)
      if (int rc = resolve_hold(c)) return rc;
    return 0;
  }
  for (sgn_ctx* c : sh) {  // the inbox flags are this function's: cleared before any growth
    c->h_ctrl->hold &= ~xf;
    SGN_HIP(c, hipMemcpy((char*)c->S.ctrl + offsetof(Ctrl, hold), &c->h_ctrl->hold, 4, hipMemcpyHostToDevice));
  }
  if (hold & HOLD_XSLOT) {
    // each sender's runs past a peer's slot (spill-area entries tagged SPILL_PEER | peer)
    std::vector<std::vector<std::vector<EvRec>>> out(sh.size());
    for (size_t i = 0; i < sh.size(); i++) {
      sgn_ctx* c = sh[i];
      const DevSim& S = c->S;
      out[i].assign(c->nranks, {});
      const uint64_t n = std::min<uint64_t>(c->h_ctrl->spill_n, S.spill_cap);
      if (!n) continue;
      std::vector<uint32_t> idx(n);
      std::vector<EvRec> rec(n);
      SGN_HIP(c, hipMemcpy(idx.data(), (const void*)S.spill_idx, n * 4, hipMemcpyDeviceToHost));
      SGN_HIP(c, hipMemcpy(rec.data(), (const void*)S.spill, n * sizeof(EvRec), hipMemcpyDeviceToHost));
      bool any = false;
      for (uint64_t k = 0; k < n; k++)
        if ((idx[k] & SPILL_PEER) && idx[k] != SPILL_DEAD) {
          out[i][idx[k] & ~SPILL_PEER].push_back(rec[k]);
          idx[k] = SPILL_DEAD;
          any = true;
        }
      if (any) SGN_HIP(c, hipMemcpy((void*)S.spill_idx, idx.data(), n * 4, hipMemcpyHostToDevice));
    }
    if (!peers) {
      for (size_t i = 0; i < sh.size(); i++)
        for (uint32_t q = 0; q < sh[i]->nranks; q++) {
          sh[q]->x_moved += out[i][q].size();
          if (int rc = inject_runs(sh[q], out[i][q])) return rc;
        }
    } else {
      std::vector<EvRec> in;
      if (int rc = comm_xmove_spills(sh[0], out[0], &in)) return rc;
      sh[0]->x_moved += in.size();
      if (int rc = inject_runs(sh[0], in)) return rc;
    }
    for (sgn_ctx* c : sh) c->x_over_rounds++;
  }
  // larger inboxes: 4x the largest per-peer count any round produced (every shard sees the same
  // maximum: the same size everywhere), at least twice the slot
  uint64_t ns = sh[0]->S.xislot;
  do ns *= 2;
  while (ns < 4 * hwm);
  if (ns > (1ULL << 26)) return set_error(sh[0], SGN_EOVERFLOW, "inbox slot above 2^26 runs per sender");
  for (sgn_ctx* c : sh)
    if (int rc = xinbox_alloc(c, ns)) return rc;
  if (!peers) {
    std::vector<char*> base(sh.size());
    for (size_t i = 0; i < sh.size(); i++) base[sh[i]->rank] = (char*)sh[i]->xin_mem;
    for (sgn_ctx* c : sh) {
      c->x_base = base;
      if (int rc = xpeer_upload(c)) return rc;
      c->x_mapped = true;
    }
  } else {
    if (int rc = comm_xpeer_map(sh[0])) return rc;
    if (!sh[0]->x_mapped) return set_error(sh[0], SGN_EDEVICE, "inbox growth: the peers' new inboxes could not be mapped");
  }
  for (sgn_ctx* c : sh) {
    c->x_grows++;
    if (int rc = upload_sim(c)) return rc;
    if (int rc = sync_ctrl(c)) return rc;  // (the injected runs' occupancy and spills)
    if (int rc = resolve_hold(c)) return rc;
  }
  return 0;
}

}  // namespace

namespace sgn {

// Rounds through k_rounds_x until max_rounds, the end, or a refused census (every shard's x_off
// set: the caller goes on with per-round launches). sh: the shards of one launch — a local
// group's (rank order) or this GPU's one (peers: the census and messages cross GPUs).
int run_xpersist(const std::vector<sgn_ctx*>& sh, bool peers, uint64_t max_rounds, uint64_t* rounds_done) {
  sgn_ctx* c0 = sh[0];
  for (sgn_ctx* c : sh)
    if (int rc = sync_ctrl(c)) return rc;
  const uint64_t r_start = c0->h_ctrl->rounds;
  uint64_t enq = 0;
  int rc = 0;
  // (a round still held from an earlier call: its pools first)
  if (!rc) rc = x_resolve(sh, peers);
  while (!rc && c0->h_ctrl->active && enq < max_rounds && !c0->paused) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(kPersistRounds, max_rounds - enq);
    const int lr = x_launch(sh, peers, n);
    if (lr < 0) return lr;
    if (lr == 0) SGN_HIP(c0, hipStreamSynchronize(c0->stream));
    for (sgn_ctx* c : sh)
      if ((rc = sync_ctrl(c))) break;
    if (rc) break;
    if (lr == 1 || census_verdict(c0, (uint32_t)c0->x_epoch) != 1) {
      // not resident (here or on a peer): nothing ran; per-round launches from now on
      for (sgn_ctx* c : sh) {
        c->x_off = true;
        c->x_mode = 1;
        c->persist_fallbacks++;
      }
      break;
    }
    rc = x_resolve(sh, peers);
    enq = c0->h_ctrl->rounds - r_start;
  }
  for (sgn_ctx* c : sh)  // (the per-round path counts its sends in row 0 from zero)
    if (c->S.xout_n) (void)hipMemsetAsync((void*)c->S.xout_n, 0, (6 * (size_t)c->nranks + 8) * 4, c->stream);
  if (rounds_done) *rounds_done = c0->h_ctrl->rounds - r_start;
  return rc;
}

// A resolved round edge on every shard of sh (sgn_shards_*): what the run loops do between their
// launches. A round k_import held for a full-slot exchange is completed first (RCCL transport; a
// local group completes it inside sgn_run_local_group and never returns with one), then the held
// flags: inbox overflow and growth across the shards, each shard's own pools and re-layout.
int shards_resolve(const std::vector<sgn_ctx*>& sh, bool peers) {
  for (sgn_ctx* c : sh) {
    c->ctrl_fresh = false;
    if (int rc = sync_ctrl(c)) return rc;
    if (!c->h_ctrl->xspill) continue;
    if (!peers)
      return set_error(c, SGN_ESTATE, "a round's full-slot exchange is incomplete: run the group first");
    if (int rc = comm_complete_spill(c)) return rc;
  }
  bool held = false;
  for (sgn_ctx* c : sh) held = held || c->h_ctrl->hold || c->h_ctrl->spill_n;
  if (!held) return 0;
  if (int rc = x_resolve(sh, peers)) return rc;
  for (sgn_ctx* c : sh)
    if (int rc = sync_ctrl(c)) return rc;
  return 0;
}

}  // namespace sgn

extern "C" {

int sgn_window(sgn_ctx* ctx, uint64_t* start, uint64_t* end, int32_t* active) {
  if (!ctx || !ctx->sim_ready) return ctx ? set_error(ctx, SGN_ESTATE, "no simulation") : SGN_EINVAL;
  int rc = sync_ctrl(ctx);
  if (start) *start = ctx->h_ctrl->ws;
  if (end) *end = ctx->h_ctrl->we;
  if (active) *active = (int32_t)ctx->h_ctrl->active;
  return rc;
}

int sgn_round(sgn_ctx* ctx, uint64_t* min_next) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  if (!ctx || !ctx->sim_ready) return ctx ? set_error(ctx, SGN_ESTATE, "no simulation") : SGN_EINVAL;
  if (int e = rng_release(ctx)) return e;
  if (ctx->comm_local)
    return set_error(ctx, SGN_ESTATE, "a local shard group runs with sgn_run_local_group, not sgn_round");
  int rc = sync_ctrl(ctx);
  if (rc) return rc;
  if (!ctx->h_ctrl->active) return set_error(ctx, SGN_ESTATE, "simulation already finished");
  if (ctx->h_ctrl->hold && (rc = resolve_hold(ctx))) return rc;  // (an earlier growth failed)
  if ((rc = launch_round(ctx))) return rc;
  rc = sync_ctrl(ctx);
  if (!rc && ctx->h_ctrl->xspill) rc = comm_complete_spill(ctx);
  if (!rc) rc = resolve_hold(ctx);
  if (min_next) *min_next = ctx->h_ctrl->last_min_next;
  return rc;
}

int sgn_run(sgn_ctx* ctx, uint64_t max_rounds, uint64_t* rounds_done) {
  if (!ctx || !ctx->sim_ready) return ctx ? set_error(ctx, SGN_ESTATE, "no simulation") : SGN_EINVAL;
  if (int e = rng_release(ctx)) return e;
  if (ctx->comm_local)
    return set_error(ctx, SGN_ESTATE, "a local shard group runs with sgn_run_local_group, not sgn_run");
  // (the control block as the last sgn_run left it, unless a call since may have changed it)
  int rc = ctx->ctrl_fresh ? 0 : sync_ctrl(ctx);
  ctx->ctrl_fresh = false;
  if (rc) return rc;
  // a round still held (an earlier pool growth failed and the caller runs again): grow first
  if ((ctx->h_ctrl->hold || ctx->h_ctrl->spill_n) && (rc = resolve_hold(ctx))) return rc;
  // (sgn_run_until: a round edge at or past Ctrl::pause_at holds with HOLD_PAUSE and the loops
  // below stop on it; sgn_run itself runs with pause_at = EMU_MAX and never sees one)
  ctx->paused = false;
  const uint64_t r_start = ctx->h_ctrl->rounds;
  uint64_t enq = 0;
  // Rounds are enqueued in batches with one host synchronisation per batch (the window
  // lives on the device; kernels of rounds past the end return at once). On a single
  // shard a full batch is one hipGraph replay: the round's launches are captured once.
  const uint64_t batch = 32;
  // SGN_GRAPH=1: a full batch is captured once as a hipGraph and replayed (multi-shard over
  // RCCL too: each round's k_execute, the grouped send/recv — RCCL records its kernels in the
  // graph — and k_import). Off by default: measured on config C with per-round launches,
  // replays are no faster than eager launches (38.9 vs 38.9 us per round untimed), and the
  // event-record nodes that time a sample of the rounds slow the replay (1.35 vs 1.47 G
  // packet events/s); the host enqueues eager rounds faster than the GPU runs them.
  const bool graph = ctx->use_graph && (ctx->nranks == 1 || ctx->comm) &&
                     getenv("SGN_GRAPH") && atoi(getenv("SGN_GRAPH")) == 1;
  if (ctx->nranks == 1 && ctx->persist_grid) {
    bool fresh = true;
    // persistent rounds: one launch runs up to kPersistRounds rounds (grid barriers inside);
    // a launch ends early at a held round edge (a pool grows here, then the rounds go on)
    while (ctx->h_ctrl->active && enq < max_rounds && ctx->persist_grid && !ctx->paused) {
      const uint32_t n = (uint32_t)std::min<uint64_t>(kPersistRounds, max_rounds - enq);
      // (no per-launch memsets: the launch resets its round buffers before its census)
      time_begin(ctx, K_EXECUTE);
      launch_k_rounds(ctx, n);
      time_end(ctx);
      ctx->kt[K_EXECUTE].total++;
      SGN_HIP(ctx, hipGetLastError());
      if ((rc = sync_ctrl_persist(ctx, ctx->res_epoch))) return rc;
      if (census_verdict(ctx, ctx->res_epoch) != 1) {
        // the grid was not resident (the occupancy model was wrong, or another context holds
        // part of the GPU): nothing ran; continue with one launch per round
        ctx->persist_grid = 0;
        ctx->persist_fallbacks++;
        ctx->persist_off = true;
        break;
      }
      if (ctx->h_ctrl->hold || ctx->h_ctrl->spill_n) fresh = false;  // (the host grows a pool)
      if ((rc = resolve_hold(ctx))) return rc;
      enq = ctx->h_ctrl->rounds - r_start;
    }
    if (!ctx->persist_grid) {
      uint64_t more = 0;
      rc = sgn_run(ctx, max_rounds - enq, &more);
      if (rounds_done) *rounds_done = ctx->h_ctrl->rounds - r_start;
      return rc;
    }
    if (rounds_done) *rounds_done = ctx->h_ctrl->rounds - r_start;
    ctx->ctrl_fresh = fresh;
    return 0;
  }
  // multi-shard, one shard per GPU: persistent rounds with the peers' inboxes mapped into this
  // process (k_rounds_x; mapped at the first run, a collective over RCCL), unless refused — then
  // per-round launches with the RCCL send/recv for the rest
  if (ctx->nranks > 1 && ctx->comm && xpersist_possible(ctx)) {
    if (!ctx->x_mapped && (rc = comm_xpeer_map(ctx))) return rc;
    if (ctx->x_mapped) {
      uint64_t k = 0;
      if ((rc = run_xpersist({ctx}, true, max_rounds, &k))) return rc;
      if (!ctx->x_off || k >= max_rounds || !ctx->h_ctrl->active) {
        if (rounds_done) *rounds_done = ctx->h_ctrl->rounds - r_start;
        return 0;
      }
    }
  }
  // rounds are counted as they complete: a multi-shard round held for a full-slot exchange
  // (comm_complete_spill) turns the rest of its batch into no-ops, which are not rounds
  uint64_t done = ctx->h_ctrl->rounds - r_start;
  static const bool dbg = getenv("SGN_DEBUG_RUN") != nullptr;
  while (ctx->h_ctrl->active && done < max_rounds && !ctx->paused) {
    const uint64_t n = std::min<uint64_t>(batch, max_rounds - done);
    if (dbg)
      fprintf(stderr, "[sgn r%u] batch n=%llu done=%llu graph=%d gexec=%d gsz=%u xsz=%u spills=%llu\n", ctx->rank,
              (unsigned long long)n, (unsigned long long)done, (int)graph, ctx->gexec != nullptr, ctx->gsz,
              ctx->xsz_cur, (unsigned long long)ctx->x_spills);
    if (graph && n == batch) {
      if (ctx->gexec && ctx->gsz != ctx->xsz_cur) drop_graph(ctx);  // the send size changed
      if (!ctx->gexec) {
        ctx->ev_pending.clear();
        ctx->ev_next = 0;
        ctx->capturing = true;
        hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
        for (uint64_t i = 0; i < n && rc == 0 && e == hipSuccess; i++) rc = launch_round(ctx);
        hipGraph_t g = nullptr;
        hipError_t e2 = hipStreamEndCapture(ctx->stream, &g);
        ctx->capturing = false;
        if (rc) return rc;
        if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamBeginCapture");
        if (e2 != hipSuccess) return hip_fail(ctx, e2, "hipStreamEndCapture");
        ctx->graph = g;
        if ((rc = add_timing_nodes(ctx, g))) return rc;
        SGN_HIP(ctx, hipGraphInstantiate(&ctx->gexec, g, nullptr, nullptr, 0));
        ctx->gbatch = batch;
        ctx->gsz = ctx->xsz_cur;
      }
      SGN_HIP(ctx, hipGraphLaunch(ctx->gexec, ctx->stream));
      ctx->kt[K_EXECUTE].total += n;
      if (ctx->nranks > 1) ctx->kt[K_IMPORT].total += n;
      ctx->graph_pending = !ctx->graph_timed.empty();
      ctx->x_bytes += n * comm_round_bytes(ctx);
    } else {
      for (uint64_t i = 0; i < n; i++)
        if ((rc = launch_round(ctx))) return rc;
    }
    if ((rc = sync_ctrl(ctx))) return rc;
    if (dbg)
      fprintf(stderr, "[sgn r%u] synced rounds=%llu spill=%u hwm=%llu\n", ctx->rank,
              (unsigned long long)(ctx->h_ctrl->rounds - r_start), ctx->h_ctrl->xspill,
              (unsigned long long)ctx->h_ctrl->xhwm);
    if (ctx->h_ctrl->xspill && (rc = comm_complete_spill(ctx))) return rc;
    if ((rc = resolve_hold(ctx))) return rc;
    if (dbg && ctx->h_ctrl->xspill == 0) fprintf(stderr, "[sgn r%u] after: rounds=%llu\n", ctx->rank,
                                                 (unsigned long long)(ctx->h_ctrl->rounds - r_start));
    done = ctx->h_ctrl->rounds - r_start;
  }
  if (rounds_done) *rounds_done = ctx->h_ctrl->rounds - r_start;
  return 0;
}

int sgn_run_until(sgn_ctx* ctx, uint64_t t_emulated, uint64_t* rounds_done) {
  if (rounds_done) *rounds_done = 0;
  if (!ctx) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (ctx->nranks > 1 || ctx->comm_local)
    return set_error(ctx, SGN_ESTATE, "sgn_run_until runs a single shard: a sharded context has no device-side pause "
                                      "(its round edges are decided across shards)");
  ctx->ctrl_fresh = false;
  int rc = sync_ctrl(ctx);
  if (rc) return rc;
  // (the fork's rule, manager.rs:1372-1382: pause once min_next_event_time >= target — the window
  // start IS that minimum, so a target at or below it pauses before anything runs)
  if (!ctx->h_ctrl->active || t_emulated <= ctx->h_ctrl->ws) return 0;
  // the round edges compare on the device (finalize_fused, k_rounds): no single-stepping, one
  // persistent launch still runs many rounds and ends at the first edge at or past the target
  SGN_HIP(ctx, hipMemcpy((char*)ctx->S.ctrl + offsetof(Ctrl, pause_at), &t_emulated, 8, hipMemcpyHostToDevice));
  rc = sgn_run(ctx, ~0ull, rounds_done);
  const uint64_t never = EMU_MAX;
  const hipError_t e = hipMemcpy((char*)ctx->S.ctrl + offsetof(Ctrl, pause_at), &never, 8, hipMemcpyHostToDevice);
  ctx->h_ctrl->pause_at = never;
  ctx->paused = false;
  if (!rc && e != hipSuccess) rc = hip_fail(ctx, e, "hipMemcpy(pause_at)");
  return rc;
}

int sgn_set_window(sgn_ctx* ctx, uint64_t start, uint64_t end) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  if (!ctx) return SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  int rc = sync_ctrl(ctx);
  if (rc) return rc;
  Ctrl& c = *ctx->h_ctrl;
  if (start < c.prev_we) return set_error(ctx, SGN_EINVAL, "sgn_set_window: start before the previous window's end");
  if (start > c.ws) return set_error(ctx, SGN_EINVAL, "sgn_set_window: start after the device's next event time");
  if (end <= start) return set_error(ctx, SGN_EINVAL, "sgn_set_window: empty window");
  if (end - start > ctx->S.BW)
    return set_error(ctx, SGN_EINVAL, "sgn_set_window: window longer than the runahead the calendar was sized for");
  end = std::min(end, ctx->S.end_time);
  if (end <= start) return set_error(ctx, SGN_EINVAL, "sgn_set_window: window at or past the stop time");
  c.ws = start;
  c.we = end;
  c.active = 1;
  SGN_HIP(ctx, hipMemcpy((void*)ctx->S.ctrl, &c, offsetof(Ctrl, overflow), hipMemcpyHostToDevice));
  // the CoDel guard for the window as set (the last round edge evaluated the one it computed)
  const uint64_t need = codel_need_host(ctx), have = c.pg_avail > c.pg_alloc ? c.pg_avail - c.pg_alloc : 0;
  if (have < need) return grow_codel(ctx, need - have);
  return 0;
}

}  // extern "C"

uint64_t sgn::layout_sig_run() { return kLayoutSig; }
