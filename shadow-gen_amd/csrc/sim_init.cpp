// sim_init.cpp — sgn_sim_init: a simulation's device state built from the routes, the hosts and
// the traffic (host slots, records, CoDel pool, calendar, exchange buffers, control block), and
// its release; the persistent multi-shard rounds' inboxes (layout, allocation, XPeer table).
// Host code only (sgn_internal.h declares what it shares with the other objects).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "sgn_internal.h"
#include "sgn_workload.h"

using namespace sgn;

namespace {

inline uint64_t host_splitmix(uint64_t& s) {
  s += 0x9e3779b97f4a7c15ULL;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

template <typename T>
T* dalloc(sgn_ctx* ctx, size_t n) {
  return (T*)dev_alloc(ctx, n * sizeof(T));
}

}  // namespace

namespace sgn {

// ---- persistent multi-shard rounds (k_rounds_x): host side ----
// Inbox layout (one uncached allocation per shard): headers [2][R][XH_WORDS], census words [R]
// (padded to a line), runs [2][R][xislot].
// (then the bins: [2][R][G][xbk] runs, G = the receiving shard's host groups)
XLay xlay(uint32_t R, uint64_t xislot, uint32_t G, uint32_t xbk) {
  XLay l;
  l.hdr = 0;
  l.cen = (size_t)2 * R * XH_WORDS * 8;
  l.runs = l.cen + ((size_t)R * 8 + 127) / 128 * 128;
  l.bins = l.runs + (size_t)2 * R * xislot * sizeof(EvRec);
  l.bytes = l.bins + (size_t)2 * R * G * xbk * sizeof(EvRec);
  return l;
}

void xinbox_release(sgn_ctx* ctx) {
  for (void* p : ctx->x_opened)
    if (p) (void)hipIpcCloseMemHandle(p);
  ctx->x_opened.clear();
  if (ctx->xin_mem) {
    (void)hipFree(ctx->xin_mem);
    ctx->sim_bytes -= std::min<uint64_t>(ctx->sim_bytes, ctx->xin_bytes);
  }
  ctx->xin_mem = nullptr;
  ctx->xin_bytes = 0;
  ctx->x_base.clear();
  ctx->x_mapped = false;
}

// A (new) inbox of xislot runs per sender and round parity, zeroed (no tag matches a round).
// Uncached device memory: peers' stores reach it over xGMI and no L2 — the writer's or this
// GPU's — keeps a copy, so the tags polled and the runs read here are the memory's. The old
// inbox and the peer mappings go (the caller maps the new ones).
int xinbox_alloc(sgn_ctx* ctx, uint64_t xislot) {
  DevSim& S = ctx->S;
  const XLay l = xlay(ctx->nranks, xislot, S.G, S.xbk);
  void* p = nullptr;
  // (a local group's shards share this GPU: ordinary device memory, device-scope accesses;
  // one shard per GPU: uncached, the peers write it over xGMI)
  S.xsys = ctx->comm_local ? 0u : 1u;
  hipError_t e = S.xsys ? hipExtMallocWithFlags(&p, l.bytes, hipDeviceMallocUncached) : hipMalloc(&p, l.bytes);
  if (e != hipSuccess) return set_error(ctx, SGN_ENOMEM, std::string("inbox allocation: ") + hipGetErrorString(e));
  if ((e = hipMemset(p, 0, l.bytes)) != hipSuccess) {
    (void)hipFree(p);
    return hip_fail(ctx, e, "hipMemset (inbox)");
  }
  xinbox_release(ctx);
  ctx->xin_mem = p;
  ctx->xin_bytes = l.bytes;
  ctx->sim_bytes += l.bytes;
  S.xin_hdr = (decltype(S.xin_hdr))((char*)p + l.hdr);
  S.xin_cen = (decltype(S.xin_cen))((char*)p + l.cen);
  S.xin_runs = (decltype(S.xin_runs))((char*)p + l.runs);
  S.xislot = (uint32_t)xislot;
  S.xin_bins = S.xbk ? (decltype(S.xin_bins))((char*)p + l.bins) : nullptr;
  return 0;
}

// This shard's XPeer table: its slot, header and census word in every shard's inbox
// (ctx->x_base, by rank; none before the mapping) and the RCCL transport's send blocks.
int xpeer_upload(sgn_ctx* ctx) {
  DevSim& S = ctx->S;
  const uint32_t R = ctx->nranks, s = ctx->rank;
  std::vector<XPeer> xp(R);
  std::memset(xp.data(), 0, R * sizeof(XPeer));
  for (uint32_t q = 0; q < R; q++) {
    XPeer& x = xp[q];
    char* b = q < ctx->x_base.size() ? ctx->x_base[q] : nullptr;
    const uint32_t Gq = q < ctx->x_G.size() ? ctx->x_G[q] : 0;
    const XLay l = xlay(R, S.xislot, Gq, S.xbk);  // (receiver q's inbox)
    if (b) {
      for (uint32_t k = 0; k < 2; k++) {
        x.runs[k] = (std::remove_reference_t<decltype(x.runs[k])>)((EvRec*)(b + l.runs) + ((size_t)k * R + s) * S.xislot);
        x.hdr[k] = (std::remove_reference_t<decltype(x.hdr[k])>)((uint64_t*)(b + l.hdr) + ((size_t)k * R + s) * XH_WORDS);
        if (S.xbk)
          x.bins[k] = (std::remove_reference_t<decltype(x.bins[k])>)((EvRec*)(b + l.bins) + ((size_t)k * R + s) * Gq * S.xbk);
      }
      x.cen = (decltype(x.cen))((uint64_t*)(b + l.cen) + s);
    }
    if (S.xout) x.runs[2] = (std::remove_reference_t<decltype(x.runs[2])>)((EvRec*)S.xout + (size_t)q * (S.xslot + XHDR) + XHDR);
  }
  SGN_HIP(ctx, hipMemcpy(ctx->d_xp, xp.data(), R * sizeof(XPeer), hipMemcpyHostToDevice));
  return 0;
}

// The exchange layer after a shard's state went back to a snapshot (sgn_shards_snapshot_restore).
// The inbox keeps its size and its mappings, but its message granules carry the global round
// number as their tag and the rewound rounds repeat those numbers: a receiver would take the
// first pass's message for the round's. The headers are zeroed (no tag matches a round, as in a
// new inbox). Slots and bins hold no run at a launch's end; the census words carry launch epochs.
int xlayer_rewind(sgn_ctx* ctx) {
  const DevSim& S = ctx->S;
  if (ctx->xin_mem) {
    const XLay l = xlay(ctx->nranks, S.xislot, S.G, S.xbk);
    SGN_HIP(ctx, hipMemsetAsync((char*)ctx->xin_mem + l.hdr, 0, l.cen - l.hdr, ctx->stream));
  }
  // (the per-round path counts its sends in row 0 from zero: run_xpersist's end)
  if (S.xout_n) SGN_HIP(ctx, hipMemsetAsync((void*)S.xout_n, 0, (6 * (size_t)ctx->nranks + 8) * 4, ctx->stream));
  if (ctx->gexec && ctx->gsz != ctx->xsz_cur) drop_graph(ctx);
  return 0;
}

void free_sim(sgn_ctx* ctx) {
  drop_graph(ctx);
  xinbox_release(ctx);
  if (ctx->x_hxl) (void)hipHostFree(ctx->x_hxl);
  ctx->x_hxl = nullptr;
  ctx->d_xp = ctx->d_xl = nullptr;  // (in allocs)
  ctx->x_mapped = false;
  ctx->rng_held.clear();
  if (ctx->d_rng_stage) hipFree(ctx->d_rng_stage);
  ctx->d_rng_stage = nullptr;
  ctx->rng_stage_cap = 0;
  if (ctx->take_mem) hipFree(ctx->take_mem);
  ctx->take_mem = nullptr;
  ctx->take_bytes = 0;
  sample_release(ctx);
  backlog_release(ctx);
  drain_take_release(ctx);
  delay_release(ctx);
  ctx->trace_buf = nullptr;  // (in allocs)
  ctx->trace_base = 0;
  ctx->trace_held = 0;
  for (void* p : ctx->allocs) hipFree(p);
  ctx->allocs.clear();
  ctx->sim_bytes = 0;
  if (ctx->d_stage) hipFree(ctx->d_stage);
  ctx->d_stage = nullptr;
  ctx->stage_cap = 0;
  if (ctx->h_ctrl) {
    hipHostFree(ctx->h_ctrl);
    ctx->h_ctrl = nullptr;
  }
  if (ctx->h_mirror) {
    hipHostFree(ctx->h_mirror);
    ctx->h_mirror = nullptr;
  }
  ctx->ctrl_fresh = false;
  ctx->sim_ready = false;
}

}  // namespace sgn

extern "C" {

int sgn_trace_enable(sgn_ctx* ctx, uint64_t capacity) {
  if (!ctx) return SGN_EINVAL;
  if (ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "sgn_trace_enable must precede sgn_sim_init");
  ctx->trace_cap = capacity;
  if (!capacity) ctx->trace_hosts.clear();  // (no trace: no set of traced hosts either)
  return 0;
}

int sgn_trace_hosts(sgn_ctx* ctx, const uint32_t* hosts, uint32_t n) {
  if (!ctx || (!hosts && n)) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_trace_hosts: null argument") : SGN_EINVAL;
  if (ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "sgn_trace_hosts must precede sgn_sim_init");
  if (!ctx->trace_cap) return set_error(ctx, SGN_ESTATE, "sgn_trace_hosts needs a trace (sgn_trace_enable first)");
  std::vector<uint32_t> v(hosts, hosts + n);
  std::sort(v.begin(), v.end());
  for (uint32_t i = 1; i < n; i++)
    if (v[i] == v[i - 1])
      return set_error(ctx, SGN_EINVAL, "sgn_trace_hosts: host " + std::to_string(v[i]) + " is listed twice");
  ctx->trace_hosts = std::move(v);  // (ascending: the identity digest does not depend on the caller's order)
  return 0;
}

int sgn_drain_enable(sgn_ctx* ctx, uint64_t capacity) {
  if (!ctx) return SGN_EINVAL;
  if (ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "sgn_drain_enable must precede sgn_sim_init");
  if (capacity == 0) return set_error(ctx, SGN_EINVAL, "drain capacity must be >= 1");
  ctx->drain_cap = capacity;
  return 0;
}

int sgn_sim_init(sgn_ctx* ctx, const sgn_sim_config* cfg, const sgn_traffic* tr) {
  if (ctx) ctx->ctrl_fresh = false;  // (it may change the device control block)
  if (!ctx || !cfg || !tr) return SGN_EINVAL;
  if (!ctx->routes_ready) return set_error(ctx, SGN_ESTATE, "sgn_routes_build must precede sgn_sim_init");
  if (!ctx->hosts_ready) return set_error(ctx, SGN_ESTATE, "sgn_hosts_set must precede sgn_sim_init");
  if (tr->kind != SGN_TRAFFIC_PERIODIC && tr->kind != SGN_TRAFFIC_TGEN &&
      tr->kind != SGN_TRAFFIC_EXTERNAL)
    return set_error(ctx, SGN_EINVAL, "unknown traffic kind");
  if (cfg->out_fifo_cap == 0 || cfg->codel_cap == 0)
    return set_error(ctx, SGN_EINVAL, "out_fifo_cap and codel_cap must be >= 1");
  if (tr->kind == SGN_TRAFFIC_PERIODIC && tr->payload_len > 0xFFFFu)
    return set_error(ctx, SGN_EINVAL, "payload_len must fit a UDP datagram");
  if (tr->kind == SGN_TRAFFIC_TGEN && (tr->n_servers == 0 || !tr->server_hosts))
    return set_error(ctx, SGN_EINVAL, "TGEN traffic needs servers");
  if (tr->kind == SGN_TRAFFIC_TGEN && tr->req_payload > 0xFFFFu)
    return set_error(ctx, SGN_EINVAL, "req_payload must fit a UDP datagram");
  if (ctx->trace_cap && !ctx->trace_hosts.empty() && ctx->trace_hosts.back() >= ctx->n_all)
    return set_error(ctx, SGN_EINVAL, "sgn_trace_hosts: host " + std::to_string(ctx->trace_hosts.back()) +
                                          " is not in the simulation (" + std::to_string(ctx->n_all) + " hosts)");
  if (ctx->sim_ready) free_sim(ctx);
  SGN_HIP(ctx, hipSetDevice(ctx->device));

  DevSim S{};
  const uint32_t nH = ctx->hi - ctx->lo;
  const uint32_t N = ctx->n_all;
  ctx->persist_off = false;
  ctx->res_epoch = ctx->res_base = 0;  // (the new control block's census words are zero)
  ctx->counters = {};
  ctx->xslot_grows = 0;
  ctx->h_ext.clear();
  ctx->failed.clear();
  S.n_all = N;
  S.lo = ctx->lo;
  S.nH = nH;
  S.U = ctx->U;
  S.end_time = SIM_START + cfg->stop_time_ns;
  S.boot_end = SIM_START + cfg->bootstrap_end_ns;
  S.runahead_cfg = cfg->runahead_ns;
  S.dynamic = cfg->use_dynamic_runahead ? 1 : 0;
  S.fifo_cap = cfg->out_fifo_cap;
  if (cfg->interface_qdisc > SGN_QDISC_ROUND_ROBIN) return set_error(ctx, SGN_EINVAL, "unknown interface_qdisc");
  S.qdisc_rr = cfg->interface_qdisc == SGN_QDISC_ROUND_ROBIN ? 1u : 0u;
  // CoDel page pool: codel_cap run slots per host on average, at least one page per host
  // (its first) plus 64 to share
  {
    const uint64_t pages = std::max<uint64_t>((uint64_t)nH + 64, ((uint64_t)nH * cfg->codel_cap + CQ_PAGE - 1) / CQ_PAGE);
    if (pages >= (1ULL << 28)) return set_error(ctx, SGN_EINVAL, "codel_cap: CoDel page pool above 2^28 pages");
    S.cq_pages = (uint32_t)pages;
    S.div_cq.init(pages);
  }
  // 1: every host is traced; 2: the hosts of sgn_trace_hosts (host code reads it: which k_execute
  // to launch, a snapshot file's identity; the kernel tests F_TRACED in the host's flags)
  const bool trace_some = ctx->trace_cap && !ctx->trace_hosts.empty();
  S.trace_on = ctx->trace_cap ? (trace_some ? 2u : 1u) : 0u;
  S.tkind = tr->kind;
  S.payload_len = tr->payload_len;
  S.unknown_permille = tr->unknown_dst_permille;
  S.req_payload = tr->req_payload;
  S.n_servers = tr->kind == SGN_TRAFFIC_TGEN ? tr->n_servers : 0;
  S.flow_seed = tr->flow_seed;
  S.period = tr->period_ns;
  S.period_jitter = tr->period_jitter_ns;
  for (int i = 0; i < 3; i++) S.file_bytes[i] = tr->file_bytes[i];

  const uint64_t min_possible = ctx->lat_min, max_lat = ctx->lat_max;
  S.min_possible = min_possible;
  S.max_lat = max_lat;
  if (min_possible == 0) return set_error(ctx, SGN_EINVAL, "route latency 0 (Runahead::new asserts)");

  // routing (device copies made by sgn_routes_build)
  S.rlat = (decltype(S.rlat))ctx->d_lat;
  S.rloss = (decltype(S.rloss))ctx->d_loss;
  uint32_t* d_unode = dalloc<uint32_t>(ctx, N);
  uint32_t* d_ip = dalloc<uint32_t>(ctx, N);
  uint32_t* d_dk = dalloc<uint32_t>(ctx, ctx->dns_key.size());
  uint32_t* d_dv = dalloc<uint32_t>(ctx, ctx->dns_val.size());
  if (!d_unode || !d_ip || !d_dk || !d_dv) return set_error(ctx, SGN_ENOMEM, "device allocation failed");
  SGN_HIP(ctx, hipMemcpy(d_unode, ctx->unode.data(), N * 4, hipMemcpyHostToDevice));
  SGN_HIP(ctx, hipMemcpy(d_ip, ctx->ip.data(), N * 4, hipMemcpyHostToDevice));
  SGN_HIP(ctx, hipMemcpy(d_dk, ctx->dns_key.data(), ctx->dns_key.size() * 4, hipMemcpyHostToDevice));
  SGN_HIP(ctx, hipMemcpy(d_dv, ctx->dns_val.data(), ctx->dns_val.size() * 4, hipMemcpyHostToDevice));
  S.unode = (decltype(S.unode))d_unode;
  S.ip = (decltype(S.ip))d_ip;
  S.dns_key = (decltype(S.dns_key))d_dk;
  S.dns_val = (decltype(S.dns_val))d_dv;
  S.dns_mask = ctx->dns_mask;
  std::vector<uint8_t> is_server(N, 0);
  if (tr->kind == SGN_TRAFFIC_TGEN) {
    uint32_t* d_sv = dalloc<uint32_t>(ctx, tr->n_servers);
    if (!d_sv) return set_error(ctx, SGN_ENOMEM, "device allocation failed");
    for (uint32_t i = 0; i < tr->n_servers; i++) {
      if (tr->server_hosts[i] >= N) return set_error(ctx, SGN_EINVAL, "server host out of range");
      is_server[tr->server_hosts[i]] = 1;
    }
    SGN_HIP(ctx, hipMemcpy(d_sv, tr->server_hosts, tr->n_servers * 4, hipMemcpyHostToDevice));
    S.servers = (decltype(S.servers))d_sv;
  }

  // ---- host slots: every shard's HostId range, permuted so that hosts of one kind share
  // waves (TGEN: servers by uplink, then clients by downlink; otherwise by bandwidth, then by
  // graph node: a wave's sends then read one row of the route table, and an XCD's workgroups
  // a few hundred rows instead of all of them — config D's ~1 k hosts per node fill whole
  // waves, so its random-peer route lookups become L2 hits). The
  // permutation only places hosts on lanes; semantics follow HostIds. SGN_HOST_ORDER=id keeps
  // HostId order (test hook). Every shard computes every shard's permutation (same inputs).
  {
    const bool by_id = getenv("SGN_HOST_ORDER") && std::string(getenv("SGN_HOST_ORDER")) == "id";
    ctx->sid_of.assign(N, 0);
    std::vector<uint32_t> order;
    for (uint32_t rk = 0; rk < ctx->nranks; rk++) {
      uint32_t lo = 0, hi = 0;
      sgn_shard_range(N, rk, ctx->nranks, &lo, &hi);
      order.resize(hi - lo);
      for (uint32_t i = lo; i < hi; i++) order[i - lo] = i;
      if (!by_id) {
        auto key = [&](uint32_t i) {
          if (tr->kind == SGN_TRAFFIC_TGEN)
            return std::make_tuple(is_server[i] ? 0u : 1u, is_server[i] ? ctx->bw_up[i] : ctx->bw_down[i], (uint64_t)i);
          return std::make_tuple(0u, ctx->bw_up[i] ^ (ctx->bw_down[i] << 1), (uint64_t)ctx->unode[i] << 32 | i);
        };
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
      }
      for (uint32_t k = 0; k < hi - lo; k++) ctx->sid_of[order[k]] = lo + k;
      if (rk == ctx->rank) ctx->host_of = order;
    }
  }
  // ---- per-host state records (one per slot), initialised on the host ----
  std::vector<HostRec> recs(nH);
  std::vector<HostConst> hk(nH);
  std::vector<uint64_t> nextloc(nH, INVALID);
  std::memset(recs.data(), 0, recs.size() * sizeof(HostRec));
  std::memset(hk.data(), 0, hk.size() * sizeof(HostConst));
  for (uint32_t h = 0; h < nH; h++) {
    const uint32_t g = ctx->host_of[h];
    HostRec& r = recs[h];
    HostConst& k = hk[h];
    k.gid = r.k_gid = g;
    k.ip = r.k_ip = ctx->ip[g];
    k.unode = r.k_unode = ctx->unode[g];
    // Xoshiro256PlusPlus::seed_from_u64 (SplitMix64 fill), host.rs:234
    uint64_t sm = ctx->seed[g];
    for (int i = 0; i < 4; i++) r.rng[i] = host_splitmix(sm);
    r.st0 = r.st1 = r.st2 = INVALID;
    // create_token_bucket (relay/mod.rs:278-288) for inet_out (up) and inet_in (down)
    for (int w = 0; w < 2; w++) {
      const uint64_t bps = (w == 0 ? ctx->bw_up[g] : ctx->bw_down[g]) / 8;
      const uint64_t inc = std::max<uint64_t>(1, bps / 1000);
      k.tb_inc[w] = r.k_tbinc[w] = inc;  // (capacity = inc + MTU, the bucket starts full)
      r.tb_bal[w] = inc + SGN_CONFIG_MTU;
      r.tb_last[w] = SIM_START;
    }
    for (int i = 0; i < 3; i++) r.dig[i] = SGN_DIGEST_SEED;
    r.rc_dst = NO_HOST;  // empty route cache
    r.cq_head = h * CQ_PAGE;  // CoDel chain: page h
    r.cq_tp = h;
    if (is_server[g]) r.flags |= F_SERVER;
    if (ctx->trace_cap && (!trace_some || std::binary_search(ctx->trace_hosts.begin(), ctx->trace_hosts.end(), g)))
      r.flags |= F_TRACED;  // (what the traced k_execute tests: every host, or the listed ones)
    const bool has_app = tr->kind == SGN_TRAFFIC_PERIODIC || (tr->kind == SGN_TRAFFIC_TGEN && !is_server[g]);
    if (has_app) {
      r.flags |= F_HAS_APP;
      const uint64_t t = SIM_START + sgn_app_start_rel(tr->flow_seed, g, tr->start_ns, tr->start_jitter_ns);
      const uint64_t e = r.eid++;
      if (t < S.end_time) {
        r.st2 = t;
        r.se2 = e;
        nextloc[h] = t;
      }
    }
  }
  auto up64 = [&](const std::vector<uint64_t>& v, auto* out) -> int {
    *out = (std::remove_reference_t<decltype(*out)>)dalloc<uint64_t>(ctx, v.size());
    if (!*out) return set_error(ctx, SGN_ENOMEM, "device allocation failed");
    SGN_HIP(ctx, hipMemcpy((void*)*out, v.data(), v.size() * 8, hipMemcpyHostToDevice));
    return 0;
  };
  auto up32 = [&](const std::vector<uint32_t>& v, auto* out) -> int {
    *out = (std::remove_reference_t<decltype(*out)>)dalloc<uint32_t>(ctx, v.size());
    if (!*out) return set_error(ctx, SGN_ENOMEM, "device allocation failed");
    SGN_HIP(ctx, hipMemcpy((void*)*out, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    return 0;
  };
  int rc = 0;
  if ((rc = up32(ctx->sid_of, &S.sid_of)) || (rc = up32(ctx->host_of, &S.host_of))) return rc;
  {  // the packet path's peer and route forms (send_batch: two loads per route-cache miss)
    std::vector<uint64_t> pe(N);
    for (uint32_t i = 0; i < N; i++) pe[i] = (uint64_t)ctx->sid_of[i] | ((uint64_t)ctx->unode[i] << 32);
    if ((rc = up64(pe, &S.peer))) return rc;
    // the 4-byte form when slot ids and node indices fit together (sid < N, node < U)
    uint32_t sb = 1, ub = 1;
    while (sb < 32 && (1ull << sb) < N) sb++;
    while (ub < 32 && (1ull << ub) < ctx->U) ub++;
    S.peer32 = nullptr;
    S.peer_sb = sb;
    if (sb + ub <= 32 && !getenv("SGN_PEER64")) {
      std::vector<uint32_t> p32(N);
      for (uint32_t i = 0; i < N; i++) p32[i] = ctx->sid_of[i] | (ctx->unode[i] << sb);
      if ((rc = up32(p32, &S.peer32))) return rc;
    }
    if ((rc = ensure_host_routes(ctx))) return rc;
    const size_t UU = (size_t)ctx->U * ctx->U;
    std::vector<RouteEnt> re(UU);
    for (size_t i = 0; i < UU; i++) {
      // reliability = (f64)(1.0f - loss) (worker.rs:363-371), exactly as the device would
      volatile float rel32 = 1.0f - ctx->h_loss[i];
      re[i].lat = ctx->h_lat[i];
      re[i].T = (uint64_t)((double)rel32 * 9007199254740992.0);
    }
    RouteEnt* d = (RouteEnt*)dev_alloc(ctx, UU * sizeof(RouteEnt), false);
    if (!d) return set_error(ctx, SGN_ENOMEM, "device allocation failed (route table)");
    SGN_HIP(ctx, hipMemcpy(d, re.data(), UU * sizeof(RouteEnt), hipMemcpyHostToDevice));
    S.route = (decltype(S.route))d;
  }
  S.hrec = (decltype(S.hrec))dalloc<HostRec>(ctx, nH);
  S.codel = (decltype(S.codel))dalloc<CodelEnt>(ctx, (size_t)S.cq_pages * CQ_PAGE);
  S.cq_next = (decltype(S.cq_next))dalloc<uint32_t>(ctx, S.cq_pages);
  {  // host slot h starts with page h; pages nH.. are the free ring's first entries
    std::vector<uint32_t> fr(S.cq_pages, 0);
    for (uint32_t i = 0; i + nH < S.cq_pages; i++) fr[i] = nH + i;
    if ((rc = up32(fr, &S.cq_free))) return rc;
  }
  S.rb_free = (decltype(S.rb_free))dalloc<uint64_t>(ctx, 3);
  S.fifo = (decltype(S.fifo))dalloc<FifoEnt>(ctx, (size_t)nH * cfg->out_fifo_cap);
  S.fifo_addr = nullptr;
  if (ctx->trace_cap) {
    S.fifo_addr = (decltype(S.fifo_addr))dalloc<uint32_t>(ctx, (size_t)nH * cfg->out_fifo_cap);
    if (!S.fifo_addr) return set_error(ctx, SGN_ENOMEM, "device allocation failed (trace)");
  }
  if (!S.hrec || !S.codel || !S.fifo || !S.cq_next || !S.rb_free)
    return set_error(ctx, SGN_ENOMEM, "device allocation failed (host state)");
  SGN_HIP(ctx, hipMemcpy((void*)S.hrec, recs.data(), recs.size() * sizeof(HostRec), hipMemcpyHostToDevice));
  S.htile = nullptr;
  if (tr->kind == SGN_TRAFFIC_PERIODIC) {  // the hot lines, tiled (kSoa)
    const size_t nt = ((size_t)nH + 63) / 64;
    std::vector<uint64_t> tile(nt * 8 * 64 * 2, 0);
    for (uint32_t h = 0; h < nH; h++)
      for (uint32_t c = 0; c < 8; c++) std::memcpy(&tile[2 * hot_idx(h, c)], (const char*)&recs[h] + 16 * c, 16);
    S.htile = (decltype(S.htile))dalloc<uint64_t>(ctx, tile.size());
    if (!S.htile) return set_error(ctx, SGN_ENOMEM, "device allocation failed (host tiles)");
    SGN_HIP(ctx, hipMemcpy((void*)S.htile, tile.data(), tile.size() * 8, hipMemcpyHostToDevice));
  }
  {
    HostConst* dk = dalloc<HostConst>(ctx, nH);
    S.n_cnt = (decltype(S.n_cnt))dalloc<uint64_t>(ctx, (size_t)N_CNT * nH);
    S.maxq = (decltype(S.maxq))dalloc<uint32_t>(ctx, nH);
    if (!dk || !S.n_cnt || !S.maxq) return set_error(ctx, SGN_ENOMEM, "device allocation failed (host state)");
    SGN_HIP(ctx, hipMemcpy(dk, hk.data(), hk.size() * sizeof(HostConst), hipMemcpyHostToDevice));
    S.hconst = (decltype(S.hconst))dk;
  }
  if ((rc = up64(nextloc, &S.nextloc))) return rc;
  S.npeer = nullptr;
  if (tr->kind == SGN_TRAFFIC_PERIODIC) {  // every app counter starts at 0
    std::vector<uint32_t> np(nH);
    for (uint32_t h = 0; h < nH; h++) {
      uint32_t peer = NO_HOST, uip = 0;
      np[h] = sgn_periodic_dst(tr->flow_seed, ctx->host_of[h], 0, N, tr->unknown_dst_permille, &peer, &uip) ? peer : NO_HOST;
    }
    if ((rc = up32(np, &S.npeer))) return rc;
  }

  // ---- calendar: bucket width >= any window length, horizon > max latency ----
  // The shortest possible window (Runahead::get, runahead.rs:44-57): a window spans at least
  // one bucket, and in dynamic mode possibly many (executed bucket by bucket).
  uint64_t BW = std::max<uint64_t>(1, std::max(min_possible, cfg->runahead_ns));
  // Every pending event lies in [ws, we + max_lat): sends happen before the window end and
  // arrive at most max_lat later (worker.rs:386-390). A static window is BW long; a dynamic
  // one is max(min used latency, configured runahead) (runahead.rs:44-57), i.e. up to
  // max(max_lat, runahead). The calendar spans that plus one partial bucket at each end;
  // send_batch checks the horizon on the device (OVF_HORIZON), so a violation is reported.
  // The persistent kernel resets a round's consumed buckets during the next round, so one more
  // window of slack keeps the next round's sends off them (see k_rounds).
  const uint64_t wmax = cfg->use_dynamic_runahead ? std::max<uint64_t>(BW, std::max(max_lat, cfg->runahead_ns)) : BW;
  uint64_t NB = (3 * wmax + max_lat) / BW + 8;
  if (NB > (1u << 20)) return set_error(ctx, SGN_EINVAL, "calendar would need > 2^20 buckets");
  while (NB & (NB - 1)) NB += NB & (~NB + 1);  // round up to a power of two
  // hosts per k_execute wave: fewer than 64 spreads the (divergent, per-lane serial) host
  // work of a round over more waves; sgn_sim_config.hosts_per_wave (0 = default 64)
  uint32_t gsz = cfg->hosts_per_wave ? cfg->hosts_per_wave : 64;
  if (const char* e = getenv("SGN_HOSTS_PER_WAVE")) gsz = (uint32_t)atoi(e);
  if (gsz == 0 || gsz > GROUP_MAX || (gsz & (gsz - 1)))
    return set_error(ctx, SGN_EINVAL, "hosts_per_wave must be a power of two in [1, 64]");
  S.gsh = (uint32_t)__builtin_ctz(gsz);
  const uint64_t G = (nH + gsz - 1) / gsz;
  uint64_t cap = cfg->event_capacity ? cfg->event_capacity : (1ULL << 22);
  uint64_t CAP = cap / ((NB + 1) * G);
  CAP = std::max<uint64_t>(CAP_MIN, std::min<uint64_t>(CAP_MAX, CAP));
  // test hook: small slabs, so that rounds spill runs and the calendar is re-laid out
  if (const char* e = getenv("SGN_SLAB_CAP")) CAP = std::max<uint64_t>(16, std::min<uint64_t>(CAP_MAX, atoll(e)));
  S.NB = (uint32_t)NB;
  S.G = (uint32_t)G;
  S.CAP = (uint32_t)CAP;
  S.BW = BW;
  S.bw_div.init(BW);
  S.div_n.init(std::max<uint64_t>(1, N));
  S.div_1000.init(1000);
  S.div_ns.init(std::max<uint64_t>(1, S.n_servers));
  S.pool = (decltype(S.pool))dalloc<EvRec>(ctx, (NB + 1) * G * CAP);
  S.w_cnt = (decltype(S.w_cnt))dalloc<uint64_t>(ctx, W_N * G);
  if (!S.w_cnt) return set_error(ctx, SGN_ENOMEM, "device allocation failed (wave slots)");
  S.slab_n = (decltype(S.slab_n))dalloc<uint32_t>(ctx, (NB + 1) * G);
  if (!S.pool || !S.slab_n) return set_error(ctx, SGN_ENOMEM, "device allocation failed (event calendar)");
  std::vector<uint32_t> bslab(NB);
  for (uint64_t b = 0; b < NB; b++) bslab[b] = (uint32_t)b;
  if ((rc = up32(bslab, &S.bucket_slab))) return rc;
  std::vector<uint64_t> bmin(NB, INVALID);
  if ((rc = up64(bmin, &S.bucket_min))) return rc;
  // SGN_STAMPS=1: per-group stamps; =2: also the persistent kernel's per-round timeline (one
  // atomic min and max per workgroup and round on shared words: it slows the rounds it times)
  if (const char* e = getenv("SGN_STAMPS")) {
    S.stamps = (decltype(S.stamps))dalloc<uint64_t>(ctx, SGN_STAMP_WORDS * G);
    if (atoi(e) >= 2) {
      S.rdbg_wg = atoi(e) >= 3 ? 1u : 0u;
      S.rdbg = (decltype(S.rdbg))dalloc<uint64_t>(ctx, S.rdbg_wg ? (size_t)8 * 128 * 2048 : 8 * 128);
    }
  }
  if (ctx->trace_cap) {
    ctx->trace_buf = dalloc<sgn_trace_rec>(ctx, ctx->trace_cap);
    if (!ctx->trace_buf) return set_error(ctx, SGN_ENOMEM, "device allocation failed (trace)");
    ctx->trace_base = 0;  // (nothing taken: the kernels' view is the buffer itself)
    ctx->trace_held = 0;
    S.trace = (decltype(S.trace))ctx->trace_buf;
    S.trace_cap = ctx->trace_cap;
  }
  ctx->handles.clear();
  ctx->drain_held.clear();
  ctx->submit_seq.assign(nH, 0u);
  if (tr->kind == SGN_TRAFFIC_EXTERNAL) {
    const uint64_t dc = ctx->drain_cap ? ctx->drain_cap : (1ULL << 20);
    S.drain = (decltype(S.drain))dalloc<sgn_drain_rec>(ctx, dc);
    if (!S.drain) return set_error(ctx, SGN_ENOMEM, "device allocation failed (drain buffer)");
    S.drain_cap = dc;
  }
  // multi-GPU exchange slots
  S.n_ranks = ctx->nranks;
  S.rank = ctx->rank;
  {
    std::vector<uint32_t> rl(ctx->nranks + 1);
    for (uint32_t r = 0; r <= ctx->nranks; r++) {
      uint32_t lo = 0, hi = 0;
      sgn_shard_range(N, r < ctx->nranks ? r : ctx->nranks - 1, ctx->nranks, &lo, &hi);
      rl[r] = r < ctx->nranks ? lo : N;
    }
    if ((rc = up32(rl, &S.rank_lo))) return rc;
  }
  if (ctx->nranks > 1) {
    if (!ctx->comm && !ctx->comm_local)
      return set_error(ctx, SGN_ESTATE, "multi-shard context needs sgn_comm_init (or sgn_comm_init_local) before sgn_sim_init");
    S.xslot = (uint32_t)ctx->xslot;
    // per peer a block of 1 + xslot records: the 32-byte round-edge message, then the runs
    S.xout = (decltype(S.xout))dalloc<EvRec>(ctx, (size_t)ctx->nranks * (ctx->xslot + XHDR));
    S.xin = (decltype(S.xin))dalloc<EvRec>(ctx, (size_t)ctx->nranks * (ctx->xslot + XHDR));
    // (per-round launches count in row 0; k_rounds_x in row round % 3)
    // (k_rounds_x: rows [3][n_ranks] of slot counts, then [3][n_ranks] of totals, bins included)
    S.xout_n = (decltype(S.xout_n))dalloc<uint32_t>(ctx, ctx->nranks * 6 + 8);
    S.xin_n = (decltype(S.xin_n))dalloc<uint32_t>(ctx, ctx->nranks * 2 + 8);
    if (!S.xout || !S.xin || !S.xout_n || !S.xin_n) return set_error(ctx, SGN_ENOMEM, "device allocation failed (exchange)");
    // persistent rounds: the second barrier's counters, the XPeer table, the launch descriptor
    // and this shard's inbox (SGN_XISLOT: a smaller first slot, a test hook for the growth path)
    S.rb2_cnt = (decltype(S.rb2_cnt))dalloc<uint32_t>(ctx, 3 * RB_CB_MAX);
    ctx->d_xp = dalloc<XPeer>(ctx, ctx->nranks);
    ctx->d_xl = dalloc<XLaunch>(ctx, 1);
    if (!S.rb2_cnt || !ctx->d_xp || !ctx->d_xl) return set_error(ctx, SGN_ENOMEM, "device allocation failed (exchange)");
    S.xp = (decltype(S.xp))ctx->d_xp;
    S.xown = kOwnFile;
    if (const char* e = getenv("SGN_XOWN")) S.xown = (uint32_t)atoi(e);
    // inbox bins: xbk runs per (parity, sender, receiving group), a power of two;
    // SGN_XBIN: another size, 0 = none (every import through the slots)
    ctx->x_G.assign(ctx->nranks, 0u);
    S.xgx = 0;
    for (uint32_t q = 0; q < ctx->nranks; q++) {
      uint32_t lo = 0, hi = 0;
      sgn_shard_range(N, q, ctx->nranks, &lo, &hi);
      ctx->x_G[q] = (hi - lo + gsz - 1) / gsz;
      S.xgx = std::max(S.xgx, ctx->x_G[q]);
    }
    S.xbk = kXBin;
    if (const char* e = getenv("SGN_XBIN")) {  // (a test hook: small bins send runs to the slots)
      const uint32_t v = (uint32_t)atoi(e);
      S.xbk = 0;
      if (v) {
        S.xbk = 1;
        while (S.xbk < v && S.xbk < (1u << 12)) S.xbk *= 2;
      }
    }
    S.xbin_n = nullptr;
    if (S.xbk) {
      S.xbin_n = (decltype(S.xbin_n))dalloc<uint32_t>(ctx, (size_t)2 * ctx->nranks * S.xgx);
      if (!S.xbin_n) return set_error(ctx, SGN_ENOMEM, "device allocation failed (inbox bin counters)");
    }
    uint64_t xis = ctx->xslot;
    if (const char* e = getenv("SGN_XISLOT")) xis = std::max<uint64_t>(1, std::min<uint64_t>(xis, (uint64_t)atoll(e)));
    ctx->S = S;  // (xinbox_alloc / xpeer_upload work on ctx->S)
    if ((rc = xinbox_alloc(ctx, xis)) || (rc = xpeer_upload(ctx))) return rc;
    S = ctx->S;
    ctx->x_off = false;
    ctx->x_mode = 1;
    ctx->x_epoch = ctx->x_grows = ctx->x_over_rounds = ctx->x_moved = ctx->x_launches = 0;
    for (sgn_ctx* g : ctx->group)  // (a local group maps every member's inbox at its next run)
      if (g) g->x_mapped = false;
  }
  Ctrl c{};
  c.ws = SIM_START;  // initial window (manager.rs:506-509)
  c.we = SIM_START + 1;
  c.active = 1;
  c.round_min = INVALID;
  c.min_used = INVALID;
  c.keep_slab = (uint32_t)NB;
  c.keep_min = INVALID;
  c.last_min_next = INVALID;
  c.prev_we = SIM_START;
  c.pause_at = EMU_MAX;
  c.pg_tail = c.pg_avail = S.cq_pages - nH;  // the free ring holds the pages beyond the hosts' first
  // multi-shard exchange size: RCCL rounds start at min(slot, kXszInit) runs per peer and
  // grow with the high-water mark; a local shard group copies counts, so it uses the slot
  ctx->xsz_cur = ctx->nranks > 1 ? (ctx->comm_local ? (uint32_t)ctx->xslot
                                                    : (uint32_t)std::min<uint64_t>(ctx->xslot, kXszInit))
                                 : 0;
  // test hook: a small first size makes the first rounds hold and complete (spill path)
  if (const char* e = getenv("SGN_XSZ_INIT"))
    if (ctx->nranks > 1 && !ctx->comm_local)
      ctx->xsz_cur = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ctx->xslot, (uint64_t)atoll(e)));
  ctx->x_spills = ctx->x_bytes = 0;
  c.xsz = ctx->xsz_cur;
  S.ctrl = (decltype(S.ctrl))dalloc<Ctrl>(ctx, 1);
  if (!S.ctrl) return set_error(ctx, SGN_ENOMEM, "device allocation failed");
  SGN_HIP(ctx, hipMemcpy(S.ctrl, &c, sizeof(c), hipMemcpyHostToDevice));
  if (!ctx->h_ctrl) SGN_HIP(ctx, hipHostMalloc((void**)&ctx->h_ctrl, sizeof(Ctrl), 0));
  static_assert(sizeof(Ctrl) % 8 == 0, "the control block's copy is written in u64 words");
  if (!ctx->h_mirror) SGN_HIP(ctx, hipHostMalloc((void**)&ctx->h_mirror, kMirrorWords * 8, 0));
  std::memset(ctx->h_mirror, 0, kMirrorWords * 8);
  {
    void* dm = nullptr;
    SGN_HIP(ctx, hipHostGetDevicePointer(&dm, ctx->h_mirror, 0));
    S.ctrl_mirror = (decltype(S.ctrl_mirror))dm;
  }
  *ctx->h_ctrl = c;
  S.fuse_finalize = ctx->nranks == 1 ? 1u : 0u;
  // PERIODIC traffic: each host receives ~BW / period runs per bucket, so a group's slab holds
  // ~gsz * BW / period; when that is a full wave (config D: 64 hosts, one send per window) all
  // 64 lanes load speculatively and the second round trip goes (same-box A/B: D +1.3 %, while
  // B's ~2-run slabs measured 1 % slower at 64 and unchanged at 4 and 8)
  // (round 4: from 4 up, twice the expected fill: config B's ~2-run slabs of 16 hosts read 4
  // records instead of 16 — its PMC traffic was 3.4x the algorithmic bytes, mostly these
  // speculative heads, while B's time measured the same at 4, 8 and 16 in round 3)
  S.gspec = GATHER_SPEC;
  if (S.tkind == SGN_TRAFFIC_PERIODIC && S.period) {
    const uint64_t fill = ((uint64_t)gsz * BW + S.period - 1) / S.period;
    S.gspec = 4;
    while (S.gspec < 64 && S.gspec < 2 * fill) S.gspec *= 2;
  }
  if (const char* e = getenv("SGN_GATHER_SPEC")) S.gspec = std::min<uint32_t>(64, (uint32_t)atoi(e));
  S.gspec = (uint32_t)std::min<uint64_t>(S.gspec, S.CAP);  // speculative loads stay inside the slab
  size_round_kernels(ctx, S);
  // persistent-round buffers (three, by round % 3): chunk minima + keep minima, counters
  S.rb_min = (decltype(S.rb_min))dalloc<uint64_t>(ctx, 3 * RB_CH * RB_MS_MAX + 4);
  S.rb_keep = S.rb_min + 3 * RB_CH * RB_MS_MAX;
  S.rb_cnt = (decltype(S.rb_cnt))dalloc<uint32_t>(ctx, 3 * RB_CB_MAX + 1);
  S.rb_occ = (decltype(S.rb_occ))dalloc<uint64_t>(ctx, 3 * RB_CH * RB_OS_MAX + 6);
  if (!S.rb_min || !S.rb_cnt || !S.rb_occ) return set_error(ctx, SGN_ENOMEM, "device allocation failed");
  S.fin_cnt = (decltype(S.fin_cnt))dalloc<uint32_t>(ctx, (G + 63) / 64 + 1);
  S.fin_occ = (decltype(S.fin_occ))dalloc<uint64_t>(ctx, (G + 63) / 64);
  if (!S.fin_occ) return set_error(ctx, SGN_ENOMEM, "device allocation failed");
  // the calendar's spill area: runs whose slab is full until the next re-layout (a round edge
  // holds right after a spill); sized for an eighth of the slabs, at least 2^16 runs
  S.spill_cap = std::max<uint64_t>(1u << 16, std::min<uint64_t>(1u << 24, (NB + 1) * G * CAP / 8));
  S.spill = (decltype(S.spill))dev_alloc(ctx, S.spill_cap * sizeof(EvRec), false);
  S.spill_idx = (decltype(S.spill_idx))dev_alloc(ctx, S.spill_cap * 4, false);
  if (!S.spill || !S.spill_idx) return set_error(ctx, SGN_ENOMEM, "device allocation failed (spill area)");
  {
    std::vector<uint64_t> inv((G + 63) / 64, INVALID);
    if ((rc = up64(inv, &S.fin_keep)) || (rc = up64(inv, &S.fin_next))) return rc;
  }
  if (!S.fin_cnt) return set_error(ctx, SGN_ENOMEM, "device allocation failed");
  ctx->d_S = dalloc<DevSim>(ctx, 1);
  if (!ctx->d_S) return set_error(ctx, SGN_ENOMEM, "device allocation failed");
  SGN_HIP(ctx, hipMemcpy(ctx->d_S, &S, sizeof(S), hipMemcpyHostToDevice));
  SGN_HIP(ctx, hipDeviceSynchronize());
  ctx->S = S;
  ctx->sim_ready = true;
  ctx->sim_gen++;  // (snapshots of the simulation before this one are refused from here)
  ctx->sim_cfg = *cfg;  // (a snapshot file's identity digest is made from these, when first asked for)
  ctx->sim_tr = *tr;
  ctx->sim_tr.server_hosts = nullptr;
  ctx->paused = false;
  for (int i = 0; i < K_NUM; i++) ctx->kt[i] = {kKernelNames[i], 0, 0.0, 0};
  return 0;
}

}  // extern "C"

uint64_t sgn::layout_sig_sim_init() { return kLayoutSig; }
