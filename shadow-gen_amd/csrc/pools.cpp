// pools.cpp — the pools that grow at a held round edge: the calendar's slabs, extensions and
// spill area, the CoDel page pool and the exchange slots. Host code only: the
// kernels it needs are launched through engine.hip's launch functions (sgn_internal.h).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "sgn_internal.h"

namespace sgn {

// ---- pools that grow (the reference's queues are unbounded): run at a held round edge ----
int upload_sim(sgn_ctx* ctx) {
  SGN_HIP(ctx, hipMemcpy(ctx->d_S, &ctx->S, sizeof(DevSim), hipMemcpyHostToDevice));
  drop_graph(ctx);  // captured batches hold k_import's by-value DevSim
  return 0;
}

// The calendar re-laid out after runs went past their slabs (a held round edge, or sgn_submit).
// The slab capacity CAP doubles while more than 1/256 of the slabs (and more than 16) would
// still overflow, up to what one workgroup's LDS orders at once; the few hot slabs past it get
// extensions of 1.5x their fill (a slab keeps the capacity it had). Every run moves into the
// new layout, the spilled runs after them; the spill area empties, and grows when it was more
// than a quarter full. Device memory grows with the hot slabs only (sizing every
// slab for the fullest cost config D ~8 -> ~16 GB for one hot slab).
int relayout_calendar(sgn_ctx* ctx) {
  DevSim& S = ctx->S;
  Ctrl& c = *ctx->h_ctrl;
  const uint64_t n_slabs = (uint64_t)(S.NB + 1) * S.G;
  if (c.spill_n > S.spill_cap)
    return set_error(ctx, SGN_EOVERFLOW, "calendar spill area exhausted within one round (" +
                                             std::to_string(c.spill_n) + " runs, capacity " +
                                             std::to_string(S.spill_cap) + ")");
  const uint64_t nsp = c.spill_n;
  std::vector<uint32_t> fill(n_slabs);
  SGN_HIP(ctx, hipMemcpy(fill.data(), (const void*)S.slab_n, n_slabs * 4, hipMemcpyDeviceToHost));
  const std::vector<uint64_t>& oext = ctx->h_ext;  // (empty: no extensions yet)
  auto oecap = [&](uint64_t i) -> uint64_t { return oext.empty() ? 0 : oext[i] >> 40; };
  // the new slab capacity
  const uint32_t lim = std::max(S.CAP, max_slab_capacity(ctx, S));
  const uint64_t few = std::max<uint64_t>(16, n_slabs / 256);
  uint32_t cap = S.CAP;
  size_t mfree = 0, mtot = 0;
  if (hipMemGetInfo(&mfree, &mtot) != hipSuccess) mfree = 0;
  while (cap * 2 <= lim && n_slabs * cap * 2 * sizeof(EvRec) < mfree / 2) {
    uint64_t over = 0;
    for (uint64_t i = 0; i < n_slabs; i++) over += fill[i] > cap;
    if (over <= few) break;
    cap *= 2;
  }
  // extensions: hot slabs keep room for 1.5x their fill, and never less than they had
  std::vector<uint64_t> next(n_slabs, 0), hot_old;
  uint64_t etot = 0, nhot = 0, max_oecap = 0;
  for (uint64_t i = 0; i < n_slabs; i++) {
    const uint64_t had = oecap(i) ? S.CAP + oecap(i) : 0;
    if (oecap(i)) {
      hot_old.push_back(i);
      max_oecap = std::max(max_oecap, oecap(i));
    }
    // (a slab that fits the slab capacity or what it had keeps that; one that outgrew both gets
    // 1.5x its fill — growth follows the fill, not the number of re-layouts)
    const uint64_t need = fill[i] <= std::max<uint64_t>(had, cap) ? had : fill[i] + fill[i] / 2;
    if (need <= cap) continue;
    const uint64_t e = ((need - cap) + 63) / 64 * 64;
    if (e >= (1ULL << 24))
      return set_error(ctx, SGN_EOVERFLOW, "a calendar slab above 2^24 runs (slab " + std::to_string(i) + ", fill " +
                                               std::to_string(fill[i]) + ", had " + std::to_string(had) + ", cap " +
                                               std::to_string(S.CAP) + " -> " + std::to_string(cap) + ")");
    next[i] = etot | (e << 40);
    etot += e;
    nhot++;
  }
  if (etot >= (1ULL << 40)) return set_error(ctx, SGN_EOVERFLOW, "calendar extensions above 2^40 runs");
  const bool changed = cap != S.CAP || next != (oext.empty() ? std::vector<uint64_t>(n_slabs, 0) : oext);
  if (changed) {
    EvRec* np = cap != S.CAP ? (EvRec*)dev_alloc(ctx, n_slabs * cap * sizeof(EvRec), false) : (EvRec*)S.pool;
    EvRec* nep = etot ? (EvRec*)dev_alloc(ctx, etot * sizeof(EvRec), false) : nullptr;
    uint64_t* nxt = etot ? (uint64_t*)dev_alloc(ctx, n_slabs * 8, false) : nullptr;
    uint32_t* cur = (uint32_t*)dev_alloc(ctx, (n_slabs + 1) * 4, false);  // + k_respill's lost-run count
    uint64_t* dhot = hot_old.empty() ? nullptr : (uint64_t*)dev_alloc(ctx, hot_old.size() * 8, false);
    auto undo = [&]() {
      if (np && np != (EvRec*)S.pool) dev_free(ctx, np, n_slabs * cap * sizeof(EvRec));
      if (nep) dev_free(ctx, nep, etot * sizeof(EvRec));
      if (nxt) dev_free(ctx, nxt, n_slabs * 8);
      if (cur) dev_free(ctx, cur, (n_slabs + 1) * 4);
      if (dhot) dev_free(ctx, dhot, hot_old.size() * 8);
    };
    if (!np || (etot && (!nep || !nxt)) || !cur || (!hot_old.empty() && !dhot)) {
      undo();
      return set_error(ctx, SGN_ENOMEM, "device allocation failed (calendar re-layout)");
    }
    if (nxt) SGN_HIP(ctx, hipMemcpy(nxt, next.data(), n_slabs * 8, hipMemcpyHostToDevice));
    if (dhot) SGN_HIP(ctx, hipMemcpy(dhot, hot_old.data(), hot_old.size() * 8, hipMemcpyHostToDevice));
    SGN_HIP(ctx, hipMemsetAsync(cur + n_slabs, 0, 4, ctx->stream));
    // the pool part moves only when the slabs grow (in place it stays where it is)
    if (np != (EvRec*)S.pool) {
      launch_k_relayout(ctx->stream, (const EvRec*)S.pool, S.CAP, (const uint64_t*)S.ext, np, cap, (const uint64_t*)nxt, nep,
                        (const uint32_t*)S.slab_n, cur, n_slabs);
    } else {
      std::vector<uint32_t> hc(n_slabs);
      for (uint64_t i = 0; i < n_slabs; i++) hc[i] = (uint32_t)std::min<uint64_t>(fill[i], S.CAP + oecap(i));
      SGN_HIP(ctx, hipMemcpy(cur, hc.data(), n_slabs * 4, hipMemcpyHostToDevice));
    }
    if (!hot_old.empty()) {
      launch_k_relayout_ext(ctx->stream, (const uint64_t*)dhot, (uint64_t)hot_old.size(), (uint32_t)max_oecap,
                            (const EvRec*)S.ext_pool, (const uint64_t*)S.ext, S.CAP, np, cap, (const uint64_t*)nxt, nep,
                            (const uint32_t*)S.slab_n);
    }
    if (nsp)
      launch_k_respill(ctx->stream, (const EvRec*)S.spill, (const uint32_t*)S.spill_idx, nsp, np, cap, (const uint64_t*)nxt,
                       nep, cur, cur + n_slabs);
    SGN_HIP(ctx, hipGetLastError());
    SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t lost = 0;
    SGN_HIP(ctx, hipMemcpy(&lost, cur + n_slabs, 4, hipMemcpyDeviceToHost));
    if (lost) {
      ctx->failed = "calendar re-layout lost " + std::to_string(lost) + " spilled runs (slab sizing)";
      return set_error(ctx, SGN_EOVERFLOW, ctx->failed);
    }
    if (np != (EvRec*)S.pool) dev_free(ctx, (void*)S.pool, n_slabs * S.CAP * sizeof(EvRec));
    if (S.ext_pool) dev_free(ctx, (void*)S.ext_pool, S.ext_total * sizeof(EvRec));
    if (S.ext) dev_free(ctx, (void*)S.ext, n_slabs * 8);
    dev_free(ctx, cur, (n_slabs + 1) * 4);
    if (dhot) dev_free(ctx, dhot, hot_old.size() * 8);
    if (cap != S.CAP) ctx->counters.cal_grows++;
    S.pool = (decltype(S.pool))np;
    S.CAP = cap;
    S.ext = (decltype(S.ext))nxt;
    S.ext_pool = (decltype(S.ext_pool))nep;
    S.ext_total = etot;
    ctx->h_ext = etot ? next : std::vector<uint64_t>();
    ctx->counters.ext_slabs = nhot;
    S.gspec = std::min<uint32_t>(S.gspec, S.CAP);
    size_round_kernels(ctx, S);
  }
  ctx->counters.cal_spill_runs += nsp;
  // the spill area: emptied; grown when this round used more than a quarter of it
  if (nsp > S.spill_cap / 4) {
    const uint64_t ncap = std::min<uint64_t>(1ULL << 30, std::max<uint64_t>(2 * S.spill_cap, 4 * nsp));
    EvRec* sp = (EvRec*)dev_alloc(ctx, ncap * sizeof(EvRec), false);
    uint32_t* si = (uint32_t*)dev_alloc(ctx, ncap * 4, false);
    if (sp && si) {
      dev_free(ctx, (void*)S.spill, S.spill_cap * sizeof(EvRec));
      dev_free(ctx, (void*)S.spill_idx, S.spill_cap * 4);
      S.spill = (decltype(S.spill))sp;
      S.spill_idx = (decltype(S.spill_idx))si;
      S.spill_cap = ncap;
      ctx->counters.spill_grows++;
    } else {  // (the area as it was still works)
      if (sp) dev_free(ctx, sp, ncap * sizeof(EvRec));
      if (si) dev_free(ctx, si, ncap * 4);
    }
  }
  const uint64_t zero[2] = {0, 0};
  SGN_HIP(ctx, hipMemcpy((char*)S.ctrl + offsetof(Ctrl, spill_n), zero, 8, hipMemcpyHostToDevice));
  SGN_HIP(ctx, hipMemcpy((char*)S.ctrl + offsetof(Ctrl, spill_imp), zero, 8, hipMemcpyHostToDevice));
  c.spill_n = 0;
  c.spill_imp = 0;
  return upload_sim(ctx);
}

// the CoDel pages the round of the current window may take (codel_round_bound, host form)
uint64_t codel_need_host(const sgn_ctx* ctx) {
  const DevSim& S = ctx->S;
  const Ctrl& c = *ctx->h_ctrl;
  if (!c.active || c.we <= c.ws) return 0;
  auto bk = [&](uint64_t t) { return (uint32_t)((t - SIM_START) / S.BW) & (S.NB - 1); };
  const uint64_t nbk = ((bk(c.we - 1) - bk(c.ws)) & (S.NB - 1)) + 1;
  return codel_pages_bound(std::min<uint64_t>(c.cal_occ, nbk * S.G * S.CAP + S.ext_total), S.nH);
}

// A CoDel page pool with at least `extra` more free pages (and at least double the size): the
// pages keep their indices (host records and chains stay valid), the free ring is rebuilt as
// its current entries followed by the new pages.
int grow_codel(sgn_ctx* ctx, uint64_t extra) {
  DevSim& S = ctx->S;
  Ctrl& c = *ctx->h_ctrl;
  if (c.pg_avail != c.pg_tail)
    return set_error(ctx, SGN_ESTATE, "CoDel pool growth outside a round edge");
  const uint64_t P = S.cq_pages;
  const uint64_t P2 = std::max<uint64_t>(2 * P, P + extra + extra / 2 + 64);
  if (P2 >= (1ULL << 28)) return set_error(ctx, SGN_EOVERFLOW, "CoDel page pool above 2^28 pages");
  CodelEnt* ne = (CodelEnt*)dev_alloc(ctx, P2 * CQ_PAGE * sizeof(CodelEnt), false);
  uint32_t* nn = (uint32_t*)dev_alloc(ctx, P2 * 4, true);
  uint32_t* nf = (uint32_t*)dev_alloc(ctx, P2 * 4, false);
  if (!ne || !nn || !nf) return set_error(ctx, SGN_ENOMEM, "device allocation failed (CoDel pool growth)");
  SGN_HIP(ctx, hipMemcpy(ne, (const void*)S.codel, P * CQ_PAGE * sizeof(CodelEnt), hipMemcpyDeviceToDevice));
  SGN_HIP(ctx, hipMemcpy(nn, (const void*)S.cq_next, P * 4, hipMemcpyDeviceToDevice));
  std::vector<uint32_t> ring(P), fr;
  SGN_HIP(ctx, hipMemcpy(ring.data(), (const void*)S.cq_free, P * 4, hipMemcpyDeviceToHost));
  fr.reserve(P2);
  for (uint64_t i = c.pg_alloc; i < c.pg_tail; i++) fr.push_back(ring[i % P]);
  for (uint64_t pg = P; pg < P2; pg++) fr.push_back((uint32_t)pg);
  const uint64_t nfree = fr.size();
  fr.resize(P2, 0);
  SGN_HIP(ctx, hipMemcpy(nf, fr.data(), P2 * 4, hipMemcpyHostToDevice));
  dev_free(ctx, (void*)S.codel, P * CQ_PAGE * sizeof(CodelEnt));
  dev_free(ctx, (void*)S.cq_next, P * 4);
  dev_free(ctx, (void*)S.cq_free, P * 4);
  S.codel = (decltype(S.codel))ne;
  S.cq_next = (decltype(S.cq_next))nn;
  S.cq_free = (decltype(S.cq_free))nf;
  S.cq_pages = (uint32_t)P2;
  S.div_cq.init(P2);
  ctx->counters.codel_allocs_before += c.pg_alloc;
  c.pg_alloc = 0;
  c.pg_tail = c.pg_avail = nfree;
  SGN_HIP(ctx, hipMemcpy((char*)S.ctrl + offsetof(Ctrl, pg_alloc), &c.pg_alloc, 3 * 8, hipMemcpyHostToDevice));
  ctx->counters.codel_grows++;
  return upload_sim(ctx);
}

// Multi-shard: a round in which some shard had more runs for a peer than a slot holds (the
// messages carry every shard's largest count, so every shard grows alike to twice that):
// the slots grow, keeping each outgoing block's message and runs, and the runs that went to
// the spill area (tagged SPILL_PEER | peer) follow them; comm_complete_spill then moves the
// whole slots and completes the round.
int grow_exchange_slot(sgn_ctx* ctx) {
  DevSim& S = ctx->S;
  const uint64_t hwm = ctx->h_ctrl->xhwm;
  uint64_t ns = S.xslot;
  while (ns < 2 * hwm) ns *= 2;
  if (ns > (1ULL << 26)) return set_error(ctx, SGN_EOVERFLOW, "exchange slot above 2^26 runs per peer");
  const size_t ob = XHDR + (size_t)S.xslot, nb = XHDR + (size_t)ns, R = S.n_ranks;
  EvRec* nxo = (EvRec*)dev_alloc(ctx, R * nb * sizeof(EvRec), true);
  EvRec* nxi = (EvRec*)dev_alloc(ctx, R * nb * sizeof(EvRec), true);
  if (!nxo || !nxi) return set_error(ctx, SGN_ENOMEM, "device allocation failed (exchange slot growth)");
  // (xin too: this shard's own message sits in its incoming block)
  for (size_t p = 0; p < R; p++) {
    SGN_HIP(ctx, hipMemcpy(nxo + p * nb, (const void*)(S.xout + p * ob), ob * sizeof(EvRec), hipMemcpyDeviceToDevice));
    SGN_HIP(ctx, hipMemcpy(nxi + p * nb, (const void*)(S.xin + p * ob), ob * sizeof(EvRec), hipMemcpyDeviceToDevice));
  }
  const uint64_t n = std::min<uint64_t>(ctx->h_ctrl->spill_n, S.spill_cap);
  if (n) {
    std::vector<uint32_t> idx(n);
    std::vector<EvRec> rec(n);
    SGN_HIP(ctx, hipMemcpy(idx.data(), (const void*)S.spill_idx, n * 4, hipMemcpyDeviceToHost));
    SGN_HIP(ctx, hipMemcpy(rec.data(), (const void*)S.spill, n * sizeof(EvRec), hipMemcpyDeviceToHost));
    std::vector<std::vector<EvRec>> per(R);
    for (uint64_t i = 0; i < n; i++)
      if ((idx[i] & SPILL_PEER) && idx[i] != SPILL_DEAD) per[idx[i] & ~SPILL_PEER].push_back(rec[i]);
    for (size_t p = 0; p < R; p++)
      if (!per[p].empty())
        SGN_HIP(ctx, hipMemcpy(nxo + p * nb + ob, per[p].data(), per[p].size() * sizeof(EvRec), hipMemcpyHostToDevice));
  }
  dev_free(ctx, (void*)S.xout, R * ob * sizeof(EvRec));
  dev_free(ctx, (void*)S.xin, R * ob * sizeof(EvRec));
  S.xout = (decltype(S.xout))nxo;
  S.xin = (decltype(S.xin))nxi;
  S.xslot = (uint32_t)ns;
  ctx->xslot = ns;
  ctx->xslot_grows++;
  if (int rc = xpeer_upload(ctx)) return rc;  // (the send blocks moved)
  return upload_sim(ctx);
}

// A round edge held the rounds (Ctrl::hold; nothing of the next round has run): the calendar
// is re-laid out after a spill, the CoDel pool grows until its free pages cover the next
// round's bound, and the rounds are released. (Multi-shard: every shard holds the same round;
// each grows what it needs.)
int resolve_hold(sgn_ctx* ctx) {
  Ctrl& c = *ctx->h_ctrl;
  if (!c.hold) {
    // (multi-shard: runs k_import spilled hold nothing; re-laid out at the batch's sync)
    return c.spill_n ? relayout_calendar(ctx) : 0;
  }
  int rc = 0;
  if (c.spill_n && (rc = relayout_calendar(ctx))) return rc;
  // (the bound again for the layout as it is now: spilled runs may be due in the held round)
  const uint64_t need = std::max(c.hold_need, codel_need_host(ctx));
  const uint64_t free = c.pg_avail > c.pg_alloc ? c.pg_avail - c.pg_alloc : 0;
  // (a pause is sgn_run_until's stop, not a pool's: it is released like one, but not counted,
  // and alone it grows nothing — the run goes on exactly as one without the pause would)
  if ((c.hold & ~HOLD_PAUSE) && free < need && (rc = grow_codel(ctx, need - free))) return rc;
  if (c.hold & HOLD_PAUSE) ctx->paused = true;
  if (c.hold & ~HOLD_PAUSE) ctx->counters.rounds_held++;
  c.hold = 0;
  c.hold_need = 0;
  SGN_HIP(ctx, hipMemcpy((char*)ctx->S.ctrl + offsetof(Ctrl, hold), &c.hold, 4, hipMemcpyHostToDevice));
  return 0;
}

// runs into this shard's calendar at a held round edge (k_inject: the bucket's current slab)
int inject_runs(sgn_ctx* ctx, const std::vector<EvRec>& runs) {
  if (runs.empty()) return 0;
  void* d = nullptr;
  SGN_HIP(ctx, hipMalloc(&d, runs.size() * sizeof(EvRec)));
  hipError_t e = hipMemcpy(d, runs.data(), runs.size() * sizeof(EvRec), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_k_inject(ctx->stream, (const DevSim*)ctx->d_S, (const EvRec*)d, (uint32_t)runs.size());
    e = hipStreamSynchronize(ctx->stream);
  }
  (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(ctx, e, "inject_runs");
  return 0;
}

}  // namespace sgn

uint64_t sgn::layout_sig_pools() { return kLayoutSig; }
