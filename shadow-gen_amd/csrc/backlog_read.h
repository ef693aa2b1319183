// backlog_read.h — a host's queue bookkeeping as the reports read it from the host records
// (backlog.hip: sgn_backlog's rows; delay.hip: the packets standing at a router when sgn_delay_enable
// seeds the carry). One reader, so the two reports cannot disagree about what stands at a host.
#pragma once

#include <hip/hip_runtime.h>

#include "sgn_internal.h"

namespace sgn {
namespace backlog_read {

// what the kernels read of the simulation (plain pointers; the sizes that bound every index)
struct BkArgs {
  const HostRec* hrec;        // [nH] by slot
  const uint64_t* htile;      // PERIODIC: the hot lines, tiled (hot_idx), else null
  const uint32_t* sid_of;     // [n_all] HostId -> lo + slot
  const uint32_t* host_of;    // [nH] slot -> HostId
  const CodelEnt* codel;      // [cq_pages * CQ_PAGE]
  const FifoEnt* fifo;        // [nH * fifo_cap]
  const EvRec* pool;          // [(NB + 1) * G * CAP]
  const uint32_t* slab_n;     // [(NB + 1) * G]
  const uint32_t* bucket_slab;  // [NB]
  const uint64_t* ext;        // [(NB + 1) * G] or null
  const EvRec* ext_pool;      // [ext_total]
  uint64_t ext_total;
  uint32_t lo, nH, n_all, NB, G, CAP, gsh, fifo_cap, cq_pages, tkind;
};

// the queues' bookkeeping of owned host i (HostId lo + i)
struct BkHost {
  uint32_t slot, flags;  // SGN_BACKLOG_*
  uint32_t cq_len, cq_head, fq_head, fq_len;
  uint64_t cq_bytes;
};
// false: the host's slot is not this shard's. A PERIODIC host with F_COLD clear ended its last
// round idle: both queues empty, nothing held — its cold lines may hold what an earlier round left
// there and are not read (HostExec::load's rule).
__device__ __forceinline__ bool bk_load(const BkArgs& a, uint32_t i, BkHost* h) {
  const uint32_t slot = a.sid_of[a.lo + i] - a.lo;
  if (slot >= a.nH) return false;
  const HostRec* r = a.hrec + slot;
  uint32_t fl, cq_head;
  if (a.htile) {  // chunk 7 of the tiled hot line: {app_k, flags | cq_head << 32}
    const uint64_t w = a.htile[2 * hot_idx(slot, 7) + 1];
    fl = (uint32_t)w;
    cq_head = (uint32_t)(w >> 32);
  } else {
    fl = r->flags;
    cq_head = r->cq_head;
  }
  h->slot = slot;
  h->cq_head = cq_head;
  if (a.tkind == SGN_TRAFFIC_PERIODIC && !(fl & F_COLD)) {
    h->flags = 0;
    h->cq_len = h->fq_head = h->fq_len = 0;
    h->cq_bytes = 0;
    return true;
  }
  h->flags = (fl & F_RI_NEXT ? SGN_BACKLOG_ROUTER_HELD : 0u) | (fl & F_RO_NEXT ? SGN_BACKLOG_OUT_HELD : 0u);
  h->cq_len = r->cq_len;
  h->fq_head = r->fq_head;
  h->fq_len = r->fq_len;
  h->cq_bytes = r->cq_bytes;
  return true;
}
inline BkArgs bk_args(const sgn_ctx* ctx) {
  const DevSim& S = ctx->S;
  BkArgs a;
  a.hrec = (const HostRec*)S.hrec;
  a.htile = (const uint64_t*)S.htile;
  a.sid_of = (const uint32_t*)S.sid_of;
  a.host_of = (const uint32_t*)S.host_of;
  a.codel = (const CodelEnt*)S.codel;
  a.fifo = (const FifoEnt*)S.fifo;
  a.pool = (const EvRec*)S.pool;
  a.slab_n = (const uint32_t*)S.slab_n;
  a.bucket_slab = (const uint32_t*)S.bucket_slab;
  a.ext = (const uint64_t*)S.ext;
  a.ext_pool = (const EvRec*)S.ext_pool;
  a.ext_total = S.ext ? S.ext_total : 0;
  a.lo = S.lo;
  a.nH = S.nH;
  a.n_all = S.n_all;
  a.NB = S.NB;
  a.G = S.G;
  a.CAP = S.CAP;
  a.gsh = S.gsh;
  a.fifo_cap = S.fifo_cap;
  a.cq_pages = S.cq_pages;
  a.tkind = S.tkind;
  return a;
}

}  // namespace backlog_read
}  // namespace sgn
