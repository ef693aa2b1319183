// snapshot.hip — snapshot and restore of a running simulation (sgn_snapshot_*).
//
// A simulation is a set of device buffers plus a few host-side counters, and the engine is
// bit-deterministic, so "restore, then run" reproduces the run that followed the save. Every
// mutable buffer but one is copied whole; the event calendar — (NB + 1) * G slabs of CAP records
// of 32 B, gigabytes at config D with a small fraction of them live — is PACKED on the device:
// slab i's runs go to packed[off[i] ..), off the exclusive scan of the slab fills. The packed
// form does not depend on the slab capacity, so a snapshot taken before the calendar was re-laid
// out unpacks into the layout it recorded ("Snapshots").
#include <algorithm>
#include <cstring>

#include "snapshot_priv.h"
// (after the HIP runtime header above: its function qualifiers)
#include "report_common.h"  // (elapsed_ms)

using namespace sgn;

// ---- device side ----------------------------------------------------------------------------
namespace {

constexpr uint32_t kScanThreads = 256, kScanPer = 8, kScanTile = kScanThreads * kScanPer;
constexpr uint32_t kWaveSlabs = 64;   // slabs per wave of the copy kernels (one per lane)
constexpr uint32_t kCopyWaves = 4;    // waves per workgroup of the copy kernels

// the runs of slab i that the snapshot holds: its fill, never more than the slab has room for
// (at a resolved round edge nothing is in the spill area, so fill <= room; the bound keeps every
// access inside the pool and the extension whatever the fill word holds)
__device__ __forceinline__ uint32_t slab_runs(const uint32_t* __restrict__ slab_n, const uint64_t* __restrict__ ext,
                                              uint32_t cap, uint64_t i) {
  const uint32_t room = cap + (ext ? (uint32_t)(ext[i] >> 40) : 0u);
  return min(slab_n[i], room);
}

// block-wide exclusive scan of one u64 per thread (kScanThreads threads); *total: the block's sum
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t* sh, uint64_t* total) {
  const uint32_t t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
    const uint64_t a = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const uint64_t incl = sh[t];
  *total = sh[kScanThreads - 1];
  __syncthreads();
  return incl - v;
}

// scan, pass 1: the runs of each tile of kScanTile slabs
__global__ __launch_bounds__(kScanThreads) void k_snap_tile_sums(const uint32_t* __restrict__ slab_n,
                                                                 const uint64_t* __restrict__ ext, uint32_t cap,
                                                                 uint64_t n_slabs, uint64_t* __restrict__ tsum) {
  __shared__ uint64_t sh[kScanThreads];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
  uint64_t s = 0;
  for (uint32_t k = 0; k < kScanPer; k++) {
    const uint64_t i = base + (uint64_t)k * kScanThreads + threadIdx.x;
    if (i < n_slabs) s += slab_runs(slab_n, ext, cap, i);
  }
  uint64_t tot;
  (void)block_excl_scan(s, sh, &tot);
  if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
}

// scan, pass 2 (one workgroup): the tile sums to their exclusive prefix, in place; the grand
// total to *total
__global__ __launch_bounds__(kScanThreads) void k_snap_tile_scan(uint64_t* __restrict__ tsum, uint32_t n_tiles,
                                                                 uint64_t* __restrict__ total) {
  __shared__ uint64_t sh[kScanThreads];
  uint64_t carry = 0;
  for (uint32_t b = 0; b < n_tiles; b += kScanThreads) {
    const uint32_t i = b + threadIdx.x;
    const uint64_t v = i < n_tiles ? tsum[i] : 0;
    uint64_t tot;
    const uint64_t ex = block_excl_scan(v, sh, &tot);
    if (i < n_tiles) tsum[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

// scan, pass 3: off[i] for every slab (a thread takes kScanPer consecutive slabs); off[n_slabs]
// is the total, written by pass 2
__global__ __launch_bounds__(kScanThreads) void k_snap_offsets(const uint32_t* __restrict__ slab_n,
                                                               const uint64_t* __restrict__ ext, uint32_t cap,
                                                               uint64_t n_slabs, const uint64_t* __restrict__ tsum,
                                                               uint64_t* __restrict__ off) {
  __shared__ uint64_t sh[kScanThreads];
  const uint64_t first = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
  uint32_t n[kScanPer];
  uint64_t s = 0;
#pragma unroll
  for (uint32_t k = 0; k < kScanPer; k++) {
    n[k] = first + k < n_slabs ? slab_runs(slab_n, ext, cap, first + k) : 0u;
    s += n[k];
  }
  uint64_t tot;
  uint64_t o = tsum[blockIdx.x] + block_excl_scan(s, sh, &tot);
#pragma unroll
  for (uint32_t k = 0; k < kScanPer; k++) {
    if (first + k < n_slabs) off[first + k] = o;
    o += n[k];
  }
}

// The copy. A wave takes kWaveSlabs consecutive slabs, one per lane for the bookkeeping: their
// packed runs are ONE contiguous range (off is a scan), which the wave walks in 16-byte units —
// lane l moves unit u + l, so a full wave moves 1 KB of consecutive packed bytes per access and,
// inside a slab's run list, 1 KB of consecutive pool bytes; a record is the two units 2r, 2r + 1.
// The slab of a unit is found by a binary search over the 64 slab offsets in LDS. Empty and short
// slabs cost their lane a table entry, not a wave, so a calendar of a million mostly empty slabs
// is a few thousand waves of bookkeeping plus the live bytes. kPack: pool -> packed, else back.
template <bool kPack>
__global__ __launch_bounds__(kWaveSlabs * kCopyWaves) void k_snap_copy(
    EvRec* __restrict__ pool, EvRec* __restrict__ ext_pool, const uint64_t* __restrict__ ext, uint32_t cap,
    const uint64_t* __restrict__ off, uint64_t n_slabs, EvRec* __restrict__ packed) {
  __shared__ uint32_t rel_[kCopyWaves][kWaveSlabs + 1];  // record offsets from the wave's first slab
  __shared__ uint64_t eo_[kCopyWaves][kWaveSlabs];       // extension offsets (records into ext_pool)
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t sb = ((uint64_t)blockIdx.x * kCopyWaves + wv) * kWaveSlabs;
  uint32_t* rel = rel_[wv];
  uint64_t* eo = eo_[wv];
  uint64_t o0 = 0;
  if (sb < n_slabs) {  // (the last workgroup's waves past the calendar only keep the barrier)
    const uint64_t i = sb + lane;
    // off has n_slabs + 1 entries: lanes past the calendar's end read the total
    const uint64_t last = sb + kWaveSlabs < n_slabs ? sb + kWaveSlabs : n_slabs;
    o0 = off[sb];
    rel[lane] = (uint32_t)(off[i < last ? i : last] - o0);
    if (lane == 0) rel[kWaveSlabs] = (uint32_t)(off[last] - o0);
    eo[lane] = (ext && i < n_slabs) ? (ext[i] & EXT_OFF_MASK) : 0;
  }
  __syncthreads();
  if (sb >= n_slabs) return;
  const uint32_t tot = rel[kWaveSlabs];
  uint4* pk = (uint4*)(packed + o0);
  // where unit u of the wave's packed range lives in the calendar
  auto locate = [&](uint64_t u) -> uint4* {
    const uint32_t r = (uint32_t)(u >> 1), half = (uint32_t)(u & 1);
    // the last slab s with rel[s] <= r (empty slabs share their successor's offset: skipped)
    uint32_t lo = 0, hi = kWaveSlabs;  // invariant: rel[lo] <= r < rel[hi]
#pragma unroll
    for (uint32_t step = 0; step < 6; step++) {
      const uint32_t mid = (lo + hi) >> 1;
      if (rel[mid] <= r) lo = mid; else hi = mid;
    }
    const uint32_t j = r - rel[lo];
    // (j < this slab's runs <= cap + its extension's capacity, by slab_runs)
    EvRec* rec = j < cap ? pool + (sb + lo) * cap + j : ext_pool + eo[lo] + (j - cap);
    return (uint4*)rec + half;
  };
  // two 16-byte accesses per lane and step, both loads issued before either store
  const uint64_t nu = 2ull * tot;
  uint64_t u = lane;
  for (; u + 64 < nu; u += 128) {
    uint4* p0 = locate(u);
    uint4* p1 = locate(u + 64);
    if (kPack) {
      const uint4 a = *p0, b = *p1;
      pk[u] = a;
      pk[u + 64] = b;
    } else {
      const uint4 a = pk[u], b = pk[u + 64];
      *p0 = a;
      *p1 = b;
    }
  }
  if (u < nu) {
    uint4* p = locate(u);
    if (kPack) pk[u] = *p; else *p = pk[u];
  }
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
using Buf = sgn_snapshot::Buf;

// The mutable buffers of DevSim that never move or change size after sgn_sim_init, in a fixed
// order (null: this simulation has none). Decided field by field (DESIGN.md lists the rest):
// constants (routing tables, hconst, sid_of, peer*, host_of, dns_*, servers, rank_lo) are not
// state; the round buffers (rb_min, rb_keep, rb_cnt, rb_occ, fin_*) are idle at a round edge —
// the per-round finalize exchanges them back to their reset values and a persistent launch resets
// them itself before its census; rb_free is three words of that kind, saved anyway.
std::vector<StateBuf> sgn::state_buffers(const DevSim& S) {
  const size_t nH = S.nH, n_slabs = (size_t)(S.NB + 1) * S.G;
  return {
      {"hrec", (void*)S.hrec, nH * sizeof(HostRec)},
      {"htile", (void*)S.htile, S.htile ? (nH + 63) / 64 * 8 * 64 * 16 : 0},
      {"n_cnt", (void*)S.n_cnt, (size_t)N_CNT * nH * 8},
      {"maxq", (void*)S.maxq, nH * 4},
      {"nextloc", (void*)S.nextloc, nH * 8},
      {"npeer", (void*)S.npeer, S.npeer ? nH * 4 : 0},
      {"rb_free", (void*)S.rb_free, 3 * 8},
      {"fifo", (void*)S.fifo, nH * (size_t)S.fifo_cap * sizeof(FifoEnt)},
      {"fifo_addr", (void*)S.fifo_addr, S.fifo_addr ? nH * (size_t)S.fifo_cap * 4 : 0},
      {"slab_n", (void*)S.slab_n, n_slabs * 4},
      {"bucket_slab", (void*)S.bucket_slab, (size_t)S.NB * 4},
      {"bucket_min", (void*)S.bucket_min, (size_t)S.NB * 8},
      {"w_cnt", (void*)S.w_cnt, (size_t)W_N * S.G * 8},
  };
}
const Buf* sgn::snap_fixed(const sgn_snapshot* s, const DevSim& S, const void* p) {
  const auto v = state_buffers(S);
  for (size_t k = 0; k < v.size() && k < s->fixed.size(); k++)
    if (v[k].p == p) return &s->fixed[k];
  return nullptr;
}

bool sgn::snap_buf_alloc(Buf* b, size_t bytes) {
  b->d = nullptr;
  b->bytes = bytes;
  return bytes == 0 || hipMalloc(&b->d, bytes) == hipSuccess;
}
void sgn::snap_release(sgn_snapshot* s) {
  auto buf_free = [](Buf& b) {
    if (b.d) (void)hipFree(b.d);
  };
  for (Buf& b : s->fixed) buf_free(b);
  for (Buf& b : s->pool) buf_free(b);
  buf_free(s->packed);
  buf_free(s->trace);
  delete s;
}
void sgn::snap_fill_info(sgn_snapshot* s, uint64_t n_slabs) {
  sgn_snapshot_info& in = s->info;
  in.rounds = s->ctrl.rounds;
  in.window_start = s->ctrl.ws;
  in.window_end = s->ctrl.we;
  in.device_bytes = s->packed.bytes + s->trace.bytes;
  for (const Buf& b : s->fixed) in.device_bytes += b.bytes;
  for (const Buf& b : s->pool) in.device_bytes += b.bytes;
  in.host_bytes = sizeof(sgn_snapshot) + s->fixed.size() * sizeof(Buf) + s->handles.size() * 8 + s->submit_seq.size() * 4 +
                  s->drain_held.size() * sizeof(sgn_drain_rec) + s->h_ext.size() * 8;
  in.calendar_runs = s->runs;
  in.calendar_bytes = s->runs * sizeof(EvRec);
  in.calendar_pool_bytes = (n_slabs * s->lay.cap + s->lay.ext_total) * sizeof(EvRec);
}
namespace {
// the scan's scratch: off (n_slabs + 1 words, the last the total) and the tile sums
struct Scan {
  uint64_t* off = nullptr;
  uint64_t* tsum = nullptr;
  uint32_t n_tiles = 0;
  ~Scan() {
    if (off) (void)hipFree(off);
    if (tsum) (void)hipFree(tsum);
  }
  bool alloc(uint64_t n_slabs) {
    n_tiles = (uint32_t)((n_slabs + kScanTile - 1) / kScanTile);
    return hipMalloc((void**)&off, (n_slabs + 1) * 8) == hipSuccess &&
           hipMalloc((void**)&tsum, (size_t)std::max(1u, n_tiles) * 8) == hipSuccess;
  }
};
// off = exclusive scan of the slab fills, stream-ordered
void launch_scan(hipStream_t st, const Scan& sc, const uint32_t* slab_n, const uint64_t* ext, uint32_t cap,
                 uint64_t n_slabs) {
  hipLaunchKernelGGL(k_snap_tile_sums, dim3(sc.n_tiles), dim3(kScanThreads), 0, st, slab_n, ext, cap, n_slabs, sc.tsum);
  hipLaunchKernelGGL(k_snap_tile_scan, dim3(1), dim3(kScanThreads), 0, st, sc.tsum, sc.n_tiles, sc.off + n_slabs);
  hipLaunchKernelGGL(k_snap_offsets, dim3(sc.n_tiles), dim3(kScanThreads), 0, st, slab_n, ext, cap, n_slabs,
                     (const uint64_t*)sc.tsum, sc.off);
}
template <bool kPack>
void launch_copy(hipStream_t st, const Scan& sc, EvRec* pool, EvRec* ext_pool, const uint64_t* ext, uint32_t cap,
                 uint64_t n_slabs, EvRec* packed) {
  const uint64_t per_wg = (uint64_t)kWaveSlabs * kCopyWaves;
  hipLaunchKernelGGL((k_snap_copy<kPack>), dim3((uint32_t)((n_slabs + per_wg - 1) / per_wg)),
                     dim3(kWaveSlabs * kCopyWaves), 0, st, pool, ext_pool, ext, cap, (const uint64_t*)sc.off, n_slabs,
                     packed);
}

int sharded(sgn_ctx* ctx, const char* what) {
  return set_error(ctx, SGN_ESTATE, std::string(what) + ": a sharded context cannot be snapshotted (a multi-shard "
                                        "snapshot needs a collective over every shard at one round edge)");
}

sgn_snapshot* owned(sgn_ctx* ctx, const sgn_snapshot* s) {
  auto it = std::find(ctx->snapshots.begin(), ctx->snapshots.end(), s);
  return it == ctx->snapshots.end() ? nullptr : *it;
}

}  // namespace

void sgn::snapshots_release(sgn_ctx* ctx) {
  for (sgn_snapshot* s : ctx->snapshots) snap_release(s);
  ctx->snapshots.clear();
}

namespace {

// One context's snapshot. A shard of a sharded run comes here from sgn_shards_snapshot_save with
// its round edge already resolved across the shards.
int save_one(sgn_ctx* ctx, sgn_snapshot** out) {
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  // CPU-held RNG states back to the device, then a resolved round edge (what sgn_run does on entry)
  if (int e = rng_release(ctx)) return e;
  int rc = sync_ctrl(ctx);
  if (rc) return rc;
  if (ctx->h_ctrl->hold || ctx->h_ctrl->spill_n) {
    ctx->ctrl_fresh = false;
    if ((rc = resolve_hold(ctx)) || (rc = sync_ctrl(ctx))) return rc;
    ctx->paused = false;
  }
  const DevSim& S = ctx->S;
  const Ctrl& c = *ctx->h_ctrl;
  if (c.spill_n) return set_error(ctx, SGN_ESTATE, "sgn_snapshot_save: the calendar's spill area is not empty");
  const uint64_t n_slabs = (uint64_t)(S.NB + 1) * S.G;
  hipStream_t st = ctx->stream;

  sgn_snapshot* s = new sgn_snapshot();
  Scan sc;
  report::ReportEvents<5> ev;  // around the scan, around the pack, after the copies
  auto fail = [&](int code, const std::string& msg) {
    (void)hipStreamSynchronize(st);
    snap_release(s);
    return set_error(ctx, code, msg);
  };
  const char* oom = "device allocation failed (snapshot)";
  if (!ev.make()) return fail(SGN_EDEVICE, "hipEventCreate failed (snapshot)");
  // every buffer but the packed calendar (its size is the scan's result)
  const auto src = state_buffers(S);
  const auto pools = pool_buffers(S, layout_of(S), std::min<uint64_t>(c.spill_n, S.spill_cap),
                                  S.drain ? std::min<uint64_t>(c.drain_n, S.drain_cap) : 0);
  s->fixed.resize(src.size());
  bool ok = sc.alloc(n_slabs);
  for (size_t k = 0; ok && k < src.size(); k++) ok = snap_buf_alloc(&s->fixed[k], src[k].bytes);
  for (size_t k = 0; ok && k < POOL_N; k++) ok = snap_buf_alloc(&s->pool[k], pools[k].bytes);
  if (!ok) return fail(SGN_ENOMEM, oom);

  // the scan first: the host needs its total before it can size the packed section
  (void)hipEventRecord(ev[0], st);
  launch_scan(st, sc, (const uint32_t*)S.slab_n, (const uint64_t*)S.ext, S.CAP, n_slabs);
  (void)hipEventRecord(ev[1], st);
  uint64_t total = 0;
  if (hipMemcpyAsync(&total, sc.off + n_slabs, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return fail(SGN_EDEVICE, "snapshot: the calendar scan failed");
  if (total > n_slabs * S.CAP + S.ext_total) return fail(SGN_ESTATE, "snapshot: calendar fill above its capacity");
  if (!snap_buf_alloc(&s->packed, total * sizeof(EvRec))) return fail(SGN_ENOMEM, oom);
  s->runs = total;

  auto d2d = [&](Buf& b, const void* from) {
    return b.bytes == 0 || hipMemcpyAsync(b.d, from, b.bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
  };
  (void)hipEventRecord(ev[2], st);
  if (total)  // (an empty calendar — a save right after sgn_sim_init — launches nothing)
    launch_copy<true>(st, sc, (EvRec*)S.pool, (EvRec*)S.ext_pool, (const uint64_t*)S.ext, S.CAP, n_slabs,
                      (EvRec*)s->packed.d);
  (void)hipEventRecord(ev[3], st);
  ok = hipGetLastError() == hipSuccess;
  for (size_t k = 0; ok && k < src.size(); k++) ok = d2d(s->fixed[k], src[k].p);
  for (size_t k = 0; ok && k < POOL_N; k++) ok = d2d(s->pool[k], pools[k].p);
  ok = ok && hipEventRecord(ev[4], st) == hipSuccess;
  ok = ok && hipStreamSynchronize(st) == hipSuccess;
  if (!ok) return fail(SGN_EDEVICE, "snapshot: a device copy failed");
  const double ms_scan = report::elapsed_ms(ev[0], ev[1]), ms_pack = report::elapsed_ms(ev[2], ev[3]),
               ms_rest = report::elapsed_ms(ev[3], ev[4]);

  s->ctx = ctx;
  s->gen = ctx->sim_gen;
  s->lay = layout_of(S);
  s->ctrl = c;
  s->counters = ctx->counters;
  s->handles = ctx->handles;
  s->submit_seq = ctx->submit_seq;
  s->drain_held = ctx->drain_held;
  s->h_ext = ctx->h_ext;
  sgn_snapshot_info& in = s->info;
  snap_fill_info(s, n_slabs);
  in.save_ms = ms_scan + ms_pack + ms_rest;
  in.pack_ms = ms_scan + ms_pack;
  ctx->snapshots.push_back(s);
  *out = s;
  return 0;
}

}  // namespace

// what a restore (and an export) checks before it touches anything (what: the entry point's name)
int sgn::snap_check(sgn_ctx* ctx, const sgn_snapshot* snap, const char* what, sgn_snapshot** s_out) {
  const std::string w(what);
  sgn_snapshot* s = owned(ctx, snap);
  if (!s) return set_error(ctx, SGN_EINVAL, w + ": not a snapshot of this context");
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (s->gen != ctx->sim_gen)
    return set_error(ctx, SGN_ESTATE, w + ": the snapshot was taken before the last sgn_sim_init");
  if (!ctx->failed.empty()) return set_error(ctx, SGN_ESTATE, "simulation unusable: " + ctx->failed);
  // A snapshot saved here keeps no trace records: the records [trace_base, N) it stands for are in
  // the trace buffer. For a snapshot ahead of the position (N past the live count: the run was
  // rewound since) that holds only while the cursor has not moved since they were written.
  if (ctx->trace_buf && !s->imported && s->ctrl.trace_n > ctx->trace_base) {
    uint64_t live = 0;
    SGN_HIP(ctx, hipSetDevice(ctx->device));
    SGN_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SGN_HIP(ctx, hipMemcpy(&live, (const char*)ctx->S.ctrl + offsetof(Ctrl, trace_n), 8, hipMemcpyDeviceToHost));
    if (s->ctrl.trace_n > std::max(live, ctx->trace_held))
      return set_error(ctx, SGN_ESTATE, w + ": the trace records up to this snapshot are no longer in the trace buffer (the "
                                            "run was rewound and the cursor moved since: a take, or a restore of an earlier "
                                            "snapshot); run forward past its round, or import it from a file");
  }
  *s_out = s;
  return 0;
}

int sgn::snap_scan_total(sgn_ctx* ctx, const uint32_t* slab_n, const uint64_t* ext, uint32_t cap, uint64_t n_slabs,
                         uint64_t* total) {
  Scan sc;
  if (!sc.alloc(n_slabs)) return set_error(ctx, SGN_ENOMEM, "device allocation failed (calendar scan)");
  launch_scan(ctx->stream, sc, slab_n, ext, cap, n_slabs);
  if (hipMemcpyAsync(total, sc.off + n_slabs, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return set_error(ctx, SGN_EDEVICE, "snapshot: the calendar scan failed");
  return 0;
}

namespace {

// One context back to its snapshot s (checked by snap_check). shard: a shard of a sharded run
// — the exchange words of the control block belong to the launch sequence and stay live.
int restore_one(sgn_ctx* ctx, sgn_snapshot* s, bool shard) {
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SGN_HIP(ctx, hipStreamSynchronize(st));
  DevSim& S = ctx->S;
  const SnapLayout L = layout_of(S), Z = s->lay;
  const uint64_t n_slabs = (uint64_t)(S.NB + 1) * S.G;
  // the launch sequence's words keep their live values (below): read them now
  Ctrl live{};
  SGN_HIP(ctx, hipMemcpy(&live, (const void*)S.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost));

  // ---- the snapshot's pool layout: every buffer it needs that the context does not have at
  // that size is allocated before anything changes (SGN_ENOMEM leaves the context as it was)
  const bool cap_re = L.cap != Z.cap, ext_re = ctx->h_ext != s->h_ext;
  // the buffers to replace: a growing pool by its index, then the calendar's three
  enum { ST_POOL = POOL_N, ST_EXT_POOL, ST_EXT, ST_N };
  struct Staged {
    bool on = false;        // replaced ...
    void* fresh = nullptr;  // ... by this one (null: by none — a layout without extensions)
    size_t bytes = 0;
    void* old = nullptr;
    size_t old_bytes = 0;
  } staged[ST_N];
  Scan sc;
  bool ok = sc.alloc(n_slabs), relaid = false;
  auto stage = [&](uint32_t which, void* old, size_t old_bytes, size_t bytes) {
    Staged& g = staged[which];
    g = {true, nullptr, bytes, old, old_bytes};
    relaid = true;
    if (ok && bytes) ok = (g.fresh = dev_alloc(ctx, bytes, false)) != nullptr;
  };
  // (the pools at their capacity, in this layout and in the snapshot's; drain has no layout scalar)
  const auto have = pool_buffers(S, L, L.spill_cap, 0), want = pool_buffers(S, Z, Z.spill_cap, 0);
  for (uint32_t k = 0; k < POOL_N; k++)
    if (want[k].bytes != have[k].bytes) stage(k, have[k].p, have[k].bytes, want[k].bytes);
  if (cap_re) stage(ST_POOL, (void*)S.pool, n_slabs * L.cap * sizeof(EvRec), n_slabs * Z.cap * sizeof(EvRec));
  if (ext_re) {
    stage(ST_EXT_POOL, (void*)S.ext_pool, L.ext_total * sizeof(EvRec), Z.ext_total * sizeof(EvRec));
    stage(ST_EXT, (void*)S.ext, n_slabs * 8, Z.ext_total ? n_slabs * 8 : 0);
  }
  if (!ok) {
    for (const Staged& g : staged) dev_free(ctx, g.fresh, g.bytes);
    return set_error(ctx, SGN_ENOMEM, "device allocation failed (snapshot restore)");
  }
  // ---- from here the context changes: the pools the run grew since go, the saved sizes return
  ctx->ctrl_fresh = false;
  ctx->rng_held.clear();  // (CPU-held draws belong to the state being replaced)
  for (const Staged& g : staged) dev_free(ctx, g.old, g.old_bytes);
  for_each_pool(S, Z, 0, 0, [&](uint32_t k, const char*, auto& member, size_t) {
    if (staged[k].on) member = (std::remove_reference_t<decltype(member)>)staged[k].fresh;
  });
  if (L.cq_pages != Z.cq_pages) S.div_cq.init(Z.cq_pages);  // (the free ring's index divides by cq_pages)
  S.cq_pages = (uint32_t)Z.cq_pages;
  S.spill_cap = Z.spill_cap;
  if (cap_re) S.pool = (decltype(S.pool))staged[ST_POOL].fresh;
  S.CAP = (uint32_t)Z.cap;
  if (ext_re) {
    void* n_ext = staged[ST_EXT].fresh;
    S.ext_pool = (decltype(S.ext_pool))staged[ST_EXT_POOL].fresh;
    S.ext = (decltype(S.ext))n_ext;
    S.ext_total = Z.ext_total;
    ctx->h_ext = s->h_ext;
    if (n_ext) SGN_HIP(ctx, hipMemcpy(n_ext, s->h_ext.data(), n_slabs * 8, hipMemcpyHostToDevice));
  }
  S.gspec = (uint32_t)Z.gspec;
  // (with the layout, before the copies that can fail: the big-slab path of the round kernels follows it)
  ctx->counters.ext_slabs = s->counters.ext_slabs;
  if (cap_re) size_round_kernels(ctx, ctx->S);  // the LDS table and the persistent grid follow the slab size
  if (relaid) {
    if (int rc = upload_sim(ctx)) {
      ctx->failed = "sgn_snapshot_restore failed half way";
      return rc;
    }
  } else {
    drop_graph(ctx);
  }

  // ---- the state
  auto d2d = [&](void* to, const Buf& b) {
    return b.bytes == 0 || hipMemcpyAsync(to, b.d, b.bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
  };
  const auto dst = state_buffers(S);
  const auto pools = pool_buffers(S, Z, 0, 0);  // (where the pools are now: the sizes copied are the snapshot's own)
  ok = dst.size() == s->fixed.size();
  for (size_t k = 0; ok && k < dst.size(); k++) ok = dst[k].bytes == s->fixed[k].bytes && d2d(dst[k].p, s->fixed[k]);
  for (size_t k = 0; ok && k < POOL_N; k++) ok = d2d(pools[k].p, s->pool[k]);
  // an imported snapshot brings the trace records up to its save (import checked that they fit);
  // one saved here has none: this context's trace buffer still holds them
  // The cursor of sgn_trace_take: an imported snapshot's records [b, N) go to the buffer's start
  // and b is the cursor; for one saved here the records [trace_base, N) are still pending, unless
  // a take since the save moved the cursor past N — then it goes back to N, and the re-run
  // produces the records from N on again (they are taken again, like drain records already taken).
  if (ctx->trace_buf) {
    ctx->trace_held = std::max(ctx->trace_held, live.trace_n);  // (the records past N stay in place)
    uint64_t base = std::min<uint64_t>(ctx->trace_base, s->ctrl.trace_n);
    if (s->trace.bytes) {
      ok = ok && s->trace.bytes <= ctx->trace_cap * sizeof(sgn_trace_rec) && d2d((void*)ctx->trace_buf, s->trace);
      base = s->trace_b;
    } else if (s->imported) {
      base = s->trace_b;  // (a file without records: everything up to N was taken before its export)
    }
    if (ok && base != ctx->trace_base) ok = trace_view_set(ctx, base) == 0;
    if (s->imported) ctx->trace_held = s->ctrl.trace_n;  // (the buffer starts with the file's records now)
  } else {
    ok = ok && s->trace.bytes == 0;
  }
  if (ok && s->runs) {
    // (the fills just restored, in stream order; the same scan as at save: the same offsets)
    launch_scan(st, sc, (const uint32_t*)S.slab_n, (const uint64_t*)S.ext, S.CAP, n_slabs);
    launch_copy<false>(st, sc, (EvRec*)S.pool, (EvRec*)S.ext_pool, (const uint64_t*)S.ext, S.CAP, n_slabs,
                       (EvRec*)s->packed.d);
    ok = hipGetLastError() == hipSuccess;
  }
  // The control block as saved, except what belongs to the launch sequence and not to the
  // simulation: the residency census (res_arrive counts every workgroup of every persistent
  // launch since sgn_sim_init against sgn_ctx::res_base; the verdicts carry the launch epoch) and
  // the barrier epoch. Rewinding them breaks the census arithmetic exactly as a memset would.
  Ctrl c = s->ctrl;
  c.res_arrive = live.res_arrive;
  c.res_verdict = live.res_verdict;
  c.res_xverdict = live.res_xverdict;
  c.epoch = live.epoch;
  if (shard) {
    // the exchange layer is not rewound (inboxes, slots and send size keep their live sizes):
    // the send size the per-round path moves, the largest per-peer count the sizes follow, and
    // no round waiting for a full-slot exchange (a restore starts from a resolved edge)
    c.xsz = live.xsz;
    c.xhwm = live.xhwm;
    c.xspill = 0;
    c.imp_done = 0;
  }
  c.hold = 0;
  c.pause_at = EMU_MAX;
  *ctx->h_ctrl = c;
  ok = ok && hipMemcpyAsync((void*)S.ctrl, ctx->h_ctrl, sizeof(Ctrl), hipMemcpyHostToDevice, st) == hipSuccess;
  ok = hipStreamSynchronize(st) == hipSuccess && ok;
  if (!ok) {
    ctx->failed = "sgn_snapshot_restore failed half way";
    return set_error(ctx, SGN_EDEVICE, ctx->failed);
  }
  // ---- the host side of the simulation (the launch sequence — res_epoch, res_base, persist_off,
  // persist_fallbacks — the kernel-time samples and the mirror's stale word stay as they are)
  ctx->counters = s->counters;
  ctx->handles = s->handles;
  ctx->submit_seq = s->submit_seq;
  ctx->drain_held = s->drain_held;
  ctx->paused = false;
  return 0;
}

}  // namespace

extern "C" {

int sgn_snapshot_save(sgn_ctx* ctx, sgn_snapshot** out) {
  if (out) *out = nullptr;
  if (!ctx || !out) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_snapshot_save: null argument") : SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (ctx->nranks > 1 || ctx->comm_local) return sharded(ctx, "sgn_snapshot_save");
  return save_one(ctx, out);
}

int sgn_snapshot_restore(sgn_ctx* ctx, const sgn_snapshot* snap) {
  if (!ctx || !snap) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_snapshot_restore: null argument") : SGN_EINVAL;
  // (snap_check asks the first two again: a foreign snapshot and a context without a simulation are
  // refused before a sharded context is, a stale snapshot or a failed context after)
  sgn_snapshot* s = owned(ctx, snap);
  if (!s) return set_error(ctx, SGN_EINVAL, "sgn_snapshot_restore: not a snapshot of this context");
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (ctx->nranks > 1 || ctx->comm_local) return sharded(ctx, "sgn_snapshot_restore");
  if (int rc = snap_check(ctx, snap, "sgn_snapshot_restore", &s)) return rc;
  return restore_one(ctx, s, false);
}

// ---- sharded runs: the same two operations over every shard at one round edge ----------------
int sgn_shards_snapshot_save(sgn_ctx* const* ctxs, uint32_t n, sgn_snapshot** out) {
  if (out && ctxs)
    for (uint32_t i = 0; i < n; i++) out[i] = nullptr;
  if (!out) return SGN_EINVAL;
  std::vector<sgn_ctx*> sh;
  bool peers = false;
  if (int rc = shard_set(ctxs, n, "sgn_shards_snapshot_save", &sh, &peers)) return rc;
  sgn_ctx* c0 = sh[0];
  for (sgn_ctx* c : sh) {
    SGN_HIP(c, hipSetDevice(c->device));
    if (int rc = rng_release(c)) return rc;
  }
  // a resolved round edge everywhere: no run waits in a sender's spill area for a peer's inbox,
  // no bin or slot holds one (a launch's end), every shard's calendar is within its slabs
  if (int rc = shards_resolve(sh, peers)) return rc;
  for (sgn_ctx* c : sh) c->paused = false;
  // every shard at the same round and window (ranks: by an all-reduce of min and max)
  {
    const Ctrl& a = *c0->h_ctrl;
    uint64_t v[3] = {a.rounds, a.ws, a.we}, lo[3] = {v[0], v[1], v[2]}, hi[3] = {v[0], v[1], v[2]};
    for (sgn_ctx* c : sh) {
      const uint64_t w[3] = {c->h_ctrl->rounds, c->h_ctrl->ws, c->h_ctrl->we};
      for (int k = 0; k < 3; k++) {
        lo[k] = std::min(lo[k], w[k]);
        hi[k] = std::max(hi[k], w[k]);
      }
    }
    if (peers)
      if (int rc = comm_agree(c0, v, 3, lo, hi)) return rc;
    if (lo[0] != hi[0] || lo[1] != hi[1] || lo[2] != hi[2])
      return set_error(c0, SGN_ESTATE, "sgn_shards_snapshot_save: the shards do not stand at the same round edge");
  }
  int rc = 0;
  for (uint32_t i = 0; i < n && !rc; i++) rc = save_one(sh[i], &out[i]);
  if (peers) {  // all or nothing across the ranks too
    uint64_t bad = rc ? 1 : 0;
    const int rc2 = comm_allreduce_max_u64(c0, &bad, 1);
    if (!rc && rc2) rc = rc2;
    if (!rc && bad) rc = set_error(c0, SGN_ESTATE, "sgn_shards_snapshot_save: another rank's snapshot failed");
  }
  if (rc)
    for (uint32_t i = 0; i < n; i++) {
      if (out[i]) sgn_snapshot_free(sh[i], out[i]);
      out[i] = nullptr;
    }
  return rc;
}

int sgn_shards_snapshot_restore(sgn_ctx* const* ctxs, uint32_t n, sgn_snapshot* const* snaps) {
  if (!snaps) return SGN_EINVAL;
  std::vector<sgn_ctx*> sh;
  bool peers = false;
  if (int rc = shard_set(ctxs, n, "sgn_shards_snapshot_restore", &sh, &peers)) return rc;
  sgn_ctx* c0 = sh[0];
  // everything is validated before anything changes
  std::vector<sgn_snapshot*> ss(n, nullptr);
  int rc = 0;
  for (uint32_t i = 0; i < n && !rc; i++) {
    if (!snaps[i]) rc = set_error(sh[i], SGN_EINVAL, "sgn_shards_snapshot_restore: null snapshot");
    else rc = snap_check(sh[i], snaps[i], "sgn_shards_snapshot_restore", &ss[i]);
  }
  for (uint32_t i = 1; i < n && !rc; i++)
    if (ss[i]->info.rounds != ss[0]->info.rounds || ss[i]->info.window_start != ss[0]->info.window_start)
      rc = set_error(sh[i], SGN_EINVAL, "sgn_shards_snapshot_restore: the snapshots are of different round edges");
  if (peers) {
    // (stream-ordered after this rank's last launch: when it returns, no peer's kernel still
    // writes this rank's inbox) every rank valid, and every rank's snapshot of the same round
    uint64_t v[2] = {rc ? 1ull : 0ull, rc ? 0ull : ss[0]->info.rounds}, lo[2], hi[2];
    if (int rc2 = comm_agree(c0, v, 2, lo, hi)) return rc ? rc : rc2;
    if (!rc && hi[0]) rc = set_error(c0, SGN_ESTATE, "sgn_shards_snapshot_restore: refused on another rank");
    if (!rc && lo[1] != hi[1])
      rc = set_error(c0, SGN_EINVAL, "sgn_shards_snapshot_restore: the ranks' snapshots are of different round edges");
  }
  if (rc) return rc;
  for (uint32_t i = 0; i < n && !rc; i++) {
    rc = restore_one(sh[i], ss[i], true);
    if (!rc) rc = xlayer_rewind(sh[i]);
    if (!rc && hipStreamSynchronize(sh[i]->stream) != hipSuccess) rc = set_error(sh[i], SGN_EDEVICE, "restore: exchange layer");
  }
  if (rc)  // (a shard went back and another did not: no round can run on this group)
    for (sgn_ctx* c : sh)
      if (c->failed.empty()) c->failed = "sgn_shards_snapshot_restore failed half way";
  if (peers) {  // no rank launches a round into an inbox its owner has not yet reset
    uint64_t bad = rc ? 1 : 0;
    const int rc2 = comm_allreduce_max_u64(c0, &bad, 1);
    if (!rc && rc2) rc = rc2;
    if (!rc && bad) {
      c0->failed = "sgn_shards_snapshot_restore failed on another rank";
      rc = set_error(c0, SGN_ESTATE, c0->failed);
    }
  }
  return rc;
}

void sgn_snapshot_free(sgn_ctx* ctx, sgn_snapshot* snap) {
  if (!ctx || !snap) return;
  auto it = std::find(ctx->snapshots.begin(), ctx->snapshots.end(), snap);
  if (it == ctx->snapshots.end()) return;  // (another context's, or freed already)
  ctx->snapshots.erase(it);
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  snap_release(snap);
}

int sgn_snapshot_info_get(const sgn_snapshot* snap, sgn_snapshot_info* out) {
  if (!snap || !out) return SGN_EINVAL;
  *out = snap->info;
  return 0;
}

}  // extern "C"
