// engine.hip — the per-round packet path of Shadow on gfx950.
//
// One wave of 64 lanes per host group (64 consecutive hosts, lane = host). A simulation
// round (core/manager.rs:541-656) for a group is exec_group():
//   gather   the group's calendar slabs of the window's buckets -> LDS (device-scope loads);
//            runs due later in the last bucket move to the spare slab set
//   order    counting sort of the due event runs by destination lane, rank sort inside each
//            lane's segment by (time, src host, src event id) (core/work/event.rs:84-183)
//   execute  every lane runs Host::execute (host/host.rs:762-830) over its segment merged
//            with its three local event slots: router/CoDel, relays and token buckets,
//            Worker::send_packet (loss draws from the host's Xoshiro256++), emitting event
//            runs into the destinations' calendar slabs
//   edge     minimum next event, bucket bookkeeping, Controller::manager_finished_current_
//            round (controller.rs:88-112) — run by the last wave to arrive
// Kernels: k_rounds (single shard, persistent: up to 128 rounds per launch with an atomic
// grid barrier per round), k_execute (one round per launch: sgn_round, multi-shard) with
// k_import after the RCCL exchange (comm.cpp; its last block advances the window), k_inject
// (sgn_submit), k_rng (sgn_rng_*). The window lives in device memory (Ctrl), so rounds run
// back to back without a host round trip.
//
// Bit-exactness notes: all time/byte/event-id arithmetic is u64 integer; the only floating
// point is (a) reliability = (f64)(1.0f - loss) vs the f64 draw (x >> 11) * 2^-53
// (core/worker.rs:363-371, exact on any IEEE device), and (b) the CoDel control law
// round(1e8 / sqrt(count)) in f64 (router/codel_queue.rs:285-298), which relies on
// correctly rounded f64 sqrt/div (checked on the GPU by tests/test_gpu_parity.py).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <tuple>

#include "sgn_internal.h"
#include "sgn_workload.h"

// Cost experiments only (tools/build_exp.sh builds them as separate libraries; results are
// not parity-valid): digests off, loss draws off.
#ifdef SGN_EXP_NODIGEST
#define sgn_drun_add_seq(...) ((void)0)
#define sgn_drun_add_same(...) ((void)0)
#define sgn_drun_flush_seq(...) ((void)0)
#define sgn_drun_flush_same(...) ((void)0)
#define sgn_digest3(h, ...) (h)
#endif

// Diagnostic build (libsgn_diag.so, -DSGN_DIAG): per-lane counts of the work kinds that
// carry dependent global-memory round trips, reported through sgn_debug_stamps.
#ifdef SGN_DIAG
#define DG(i) ((void)0)  // per-lane work counts: off (registers; see DGT sections)
#define DGT_BEGIN(v) const uint64_t v = __builtin_amdgcn_s_memtime()
// wave time in a section: added by the section's lowest active lane only (the lanes in a
// section entered it together), so the wave's sum over lanes is the section's wave time
#define DGT_END(i, v)                                                                  \
  do {                                                                                 \
    const uint64_t dgt_t = __builtin_amdgcn_s_memtime();                               \
    if ((uint32_t)(__ffsll((long long)__ballot(1)) - 1) == (threadIdx.x & 63))         \
      dgt[i] += (uint32_t)(dgt_t - (v));                                               \
  } while (0)
#else
#define DG(i) ((void)0)
#define DGT_BEGIN(v) ((void)0)
#define DGT_END(i, v) ((void)0)
#endif
enum { DG_RO = 0, DG_RI, DG_APP, DG_BATCH, DG_HDLOAD, DG_FQLOAD, DG_RMISS, DG_POPRUN, DG_N };
// diagnostic timers: cycles while this lane was inside ...
enum { DGT_SEND = 0, DGT_FWDOUT, DGT_FWDIN, DGT_POP, DGT_APP, DGT_LOAD,
       DGT_HDLD, DGT_FHLD, DGT_RTLD, DGT_SVLD, DGT_SLAB,
       DGT_DRAWS,   // (counts, not cycles) loss draws of this lane's trains
       DGT_RENTRY,  // ... and the wave's entries into the draw loop (its lowest lane counts)
       DGT_LLANE,   // (counts) this lane's entries with a long train (more than kTrainWait draws)
       DGT_LENTRY,  // ... and the wave's entries in which some lane draws a long train
       DGT_CQALLOC, DGT_CQFREE, DGT_TBRM, DGT_DELIV,  // CoDel page alloc / free, token bucket, delivery
       DGT_N };
#ifdef SGN_DIAG
#define DGT_WAIT() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#else
#define DGT_WAIT() ((void)0)
#endif

namespace sgn {

enum : uint32_t { RELAY_IDLE = 0, RELAY_PENDING = 1, RELAY_FORWARDING = 2 };

constexpr uint64_t CODEL_TARGET = 10000000ULL;      // codel_queue.rs:23
constexpr uint64_t CODEL_INTERVAL = 100000000ULL;   // codel_queue.rs:28
constexpr uint64_t SIMTIME_MAX = 17500059273709551614ULL;

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int k) {
  return (x << k) | (x >> (64 - k));
}
// xoshiro256++'s operations on 32-bit halves for gfx950's VALU: a 64-bit rotate is two
// v_alignbit_b32 (the compiler's shift pair + or takes three), and a ^ b ^ c is one
// v_bitop3_b32 per half (LUT 0x96) where the compiler emits two v_xor_b32.
__device__ __forceinline__ uint32_t lo32(uint64_t x) { return (uint32_t)x; }
__device__ __forceinline__ uint32_t hi32(uint64_t x) { return (uint32_t)(x >> 32); }
__device__ __forceinline__ uint64_t mk64(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
template <int K>  // rotate left by K, 0 < K < 64, K != 32
__device__ __forceinline__ uint64_t rotl64c(uint64_t x) {
  static_assert(K > 0 && K < 64 && K != 32, "rotate amount");
  if constexpr (K < 32)
    return mk64(__builtin_amdgcn_alignbit(lo32(x), hi32(x), 32 - K), __builtin_amdgcn_alignbit(hi32(x), lo32(x), 32 - K));
  else
    return mk64(__builtin_amdgcn_alignbit(hi32(x), lo32(x), 64 - K), __builtin_amdgcn_alignbit(lo32(x), hi32(x), 64 - K));
}
__device__ __forceinline__ uint64_t xor3_64(uint64_t a, uint64_t b, uint64_t c) {
  return mk64(__builtin_amdgcn_bitop3_b32(lo32(a), lo32(b), lo32(c), 0x96),
              __builtin_amdgcn_bitop3_b32(hi32(a), hi32(b), hi32(c), 0x96));
}
// one xoshiro256++ step (rand_xoshiro 0.7.0 Xoshiro256PlusPlus::next_u64) on state s0..s3
__device__ __forceinline__ void xoshiro_step(uint64_t& s0, uint64_t& s1, uint64_t& s2, uint64_t& s3) {
  // s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3; s2 ^= s1 << 17 (old s1); s3 = rotl(s3, 45)
  const uint64_t t = s1 << 17;
  const uint64_t n1 = xor3_64(s1, s2, s0);
  const uint64_t n0 = xor3_64(s0, s3, s1);
  const uint64_t n2 = xor3_64(s2, s0, t);
  s3 = rotl64c<45>(s3 ^ s1);
  s0 = n0;
  s1 = n1;
  s2 = n2;
}
__device__ __forceinline__ uint64_t xoshiro_out(uint64_t s0, uint64_t s3) { return rotl64c<23>(s0 + s3) + s0; }
__device__ __forceinline__ uint32_t xoshiro_out_hi_nc(uint64_t s0, uint64_t s3) {
  const uint64_t a = s0 + s3;
  return __builtin_amdgcn_alignbit(hi32(a), lo32(a), 9) + hi32(s0);  // hi32(rotl(a, 23)) + hi32(s0)
}
__device__ __forceinline__ uint64_t sat_sub(uint64_t a, uint64_t b) { return a > b ? a - b : 0; }
__device__ __forceinline__ uint64_t mul_sat(uint64_t a, uint64_t b, uint64_t cap) {
  uint64_t hi = __umul64hi(a, b);
  uint64_t lo = a * b;
  return (hi != 0 || lo > cap) ? cap : lo;
}
// EmulatedTime::saturating_add (emulated_time.rs:106-111)
__device__ __forceinline__ uint64_t emu_sat_add(uint64_t t, uint64_t d) {
  uint64_t x = t + d;
  return (x < t || x > EMU_MAX) ? EMU_MAX : x;
}

__device__ __forceinline__ bool ev_less(const EvRec& a, const EvRec& b) {
  if (a.time != b.time) return a.time < b.time;
  if (a.src != b.src) return a.src < b.src;
  return a.eid < b.eid;
}

// ---- cross-workgroup data inside one launch (persistent rounds; MI355X L2s are per XCD and
// not coherent): data another workgroup reads in a later round is stored write-through with
// device-scope atomic stores, and control words are read with device-scope atomic loads.
template <typename T>
__device__ __forceinline__ T ld_dev(SGN_GLB T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void st_dev(SGN_GLB T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ EvRec ld_dev_rec(SGN_GLB const EvRec* p) {
  SGN_GLB uint64_t* q = (SGN_GLB uint64_t*)p;
  EvRec r;
  r.time = ld_dev(q);
  r.eid = ld_dev(q + 1);
  const uint64_t sd = ld_dev(q + 2), pt = ld_dev(q + 3);
  r.src = (uint32_t)sd;
  r.dst = (uint32_t)(sd >> 32);
  r.pc = (uint32_t)pt;
  r.tag = (uint32_t)(pt >> 32);
  return r;
}
// A 16-byte write-through store (global_store_dwordx4 sc1: the agent-scope form of a store,
// MI355X_MICROARCH.md's store table): a 32-byte record as two of them is two 32-B fabric
// writes, where four 8-byte sc1 stores were four (tools/pmc_calib.sh: an 8-B sc1 store costs
// a 32-B write). hipcc does not count an asm store in its waits: the round's arrival waits for
// every store with its own s_waitcnt vmcnt(0); the s_nop keeps the data registers from being
// overwritten under the store.
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_wt16(SGN_GLB void* p, uint64_t lo, uint64_t hi) {
  u64x2 v;
  v.x = lo;
  v.y = hi;
  // (no "memory" clobber: nothing in this wave reads the stored bytes before the round's
  // arrival, whose own volatile asm s_waitcnt stays after this one; the clobber made hipcc
  // keep a local aggregate in scratch)
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"((uint64_t)p), "v"(v));
}
__device__ __forceinline__ void st_dev_rec(SGN_GLB EvRec* p, const EvRec& r) {
  SGN_GLB char* q = (SGN_GLB char*)p;
  st_wt16(q, r.time, r.eid);
  st_wt16(q + 16, (uint64_t)r.src | ((uint64_t)r.dst << 32), (uint64_t)r.pc | ((uint64_t)r.tag << 32));
}

// Multi-shard exchange data (a peer shard's inbox: another GPU's memory over xGMI, or the
// RCCL transport's send block): written through to memory at system scope (sc0 sc1), so the
// record is in the receiver's memory when the writing wave's s_waitcnt vmcnt(0) completes — the
// sender publishes its round-edge message only after every such store has completed.
__device__ __forceinline__ void st_sys16(SGN_GLB void* p, uint64_t lo, uint64_t hi) {
  u64x2 v;
  v.x = lo;
  v.y = hi;
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"((uint64_t)p), "v"(v));
}
__device__ __forceinline__ void st_sys_rec(SGN_GLB EvRec* p, const EvRec& r) {
  SGN_GLB char* q = (SGN_GLB char*)p;
  st_sys16(q, r.time, r.eid);
  st_sys16(q + 16, (uint64_t)r.src | ((uint64_t)r.dst << 32), (uint64_t)r.pc | ((uint64_t)r.tag << 32));
}
__device__ __forceinline__ void st_sys(SGN_GLB uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint64_t ld_sys(SGN_GLB uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ EvRec ld_sys_rec(SGN_GLB const EvRec* p) {
  SGN_GLB uint64_t* q = (SGN_GLB uint64_t*)p;
  EvRec r;
  r.time = ld_sys(q);
  r.eid = ld_sys(q + 1);
  const uint64_t sd = ld_sys(q + 2), pt = ld_sys(q + 3);
  r.src = (uint32_t)sd;
  r.dst = (uint32_t)(sd >> 32);
  r.pc = (uint32_t)pt;
  r.tag = (uint32_t)(pt >> 32);
  return r;
}

// CoDel pool entries: a page serves other hosts (other workgroups, other XCDs) after it is
// freed, so its entries are written through and read from memory like other cross-workgroup
// data (a dirty L2 line of the previous owner must never overwrite the new owner's runs)
__device__ __forceinline__ CodelEnt ld_dev_cq(SGN_GLB const CodelEnt* p) {
#ifdef SGN_EXP_PLAINCQ  // cost experiment only (build_exp.sh): what device scope costs config C
  return *p;
#endif
  SGN_GLB uint64_t* q = (SGN_GLB uint64_t*)p;
  CodelEnt e;
  e.enqueue_ts = ld_dev(q);
  e.eid = ld_dev(q + 1);
  const uint64_t a = ld_dev(q + 2), b = ld_dev(q + 3);
  e.src = (uint32_t)a;
  e.payload = (uint32_t)(a >> 32);
  e.tag = (uint32_t)b;
  e.count = (uint32_t)(b >> 32);
  return e;
}
__device__ __forceinline__ void st_dev_cq(SGN_GLB CodelEnt* p, const CodelEnt& e) {
#ifdef SGN_EXP_PLAINCQ
  *p = e;
  return;
#endif
  SGN_GLB char* q = (SGN_GLB char*)p;
  st_wt16(q, e.enqueue_ts, e.eid);
  st_wt16(q + 16, (uint64_t)e.src | ((uint64_t)e.payload << 32), (uint64_t)e.tag | ((uint64_t)e.count << 32));
}

// device-scope atomic min whose result is not used: the wave does not wait for it here (a
// returning one costs a round trip per call); the arrival's s_waitcnt vmcnt(0) completes it
// before the round edge reads the minima
__device__ __forceinline__ void min_nr(SGN_GLB uint64_t* p, uint64_t v) {
  (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a rare per-host counter in the host record: a no-return atomic add, so the lane does not
// wait for a load of the old value
__device__ __forceinline__ void cnt_add(SGN_GLB uint64_t* p, uint64_t v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- DevSim as the round kernels see it ----
// Device code reads a uniform DevSim field as SK(field), with S in scope: either the struct in
// memory (const DevSim&: SK is plain S.field, a scalar load where it is used) or the lane table
// (SimTab, sgn_internal.h: one v_readlane_b32 per dword). The functions of the event path take
// S as a template parameter; k_rounds<TGEN, *> passes the table, every other kernel the struct.
struct SimTab {
  uint32_t r[KTAB_REGS];
  const DevSim* g;  // the struct in memory (sk_mem: fields indexed per lane, the rare paths)
};
// Filled at kernel entry, before any divergent branch: lane i of register j holds dword
// ktab_src(j, i). The empty asm pins each load where it is (a load sunk into a divergent branch
// would leave inactive lanes' dwords unloaded) and makes the value opaque, so the compiler
// cannot turn a readlane back into a scalar load.
__device__ __forceinline__ SimTab ktab_fill(const DevSim* __restrict__ g) {
  SimTab t;
  t.g = g;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t* p = (const uint32_t*)g;
#pragma unroll
  for (uint32_t j = 0; j < KTAB_REGS; j++) {
    uint32_t v = p[ktab_src(j, lane)];
    asm volatile("" : "+v"(v));
    t.r[j] = v;
  }
  return t;
}
template <class T, uint32_t OFF>
__device__ __forceinline__ T ktab_get(const SimTab& t) {
  static_assert(sizeof(T) % 4 == 0 && OFF % 4 == 0 && OFF + sizeof(T) <= sizeof(DevSim), "whole dwords of DevSim");
  uint32_t w[sizeof(T) / 4];
#pragma unroll
  for (uint32_t k = 0; k < sizeof(T) / 4; k++)
    w[k] = (uint32_t)__builtin_amdgcn_readlane((int)t.r[ktab_reg(OFF + 4 * k)], (int)ktab_lane(OFF + 4 * k));
  T v;
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}
template <uint32_t OFF, class F>
__device__ __forceinline__ decltype(auto) sk_read(const DevSim& s, F f) {
  return f(s);  // (a reference to the member: the expression S.field itself)
}
template <uint32_t OFF, class F>
__device__ __forceinline__ auto sk_read(const SimTab& t, F f) {
  return ktab_get<std::remove_cv_t<std::remove_reference_t<decltype(f(*t.g))>>, OFF>(t);
}
__device__ __forceinline__ const DevSim& sk_mem(const DevSim& s) { return s; }
__device__ __forceinline__ const DevSim& sk_mem(const SimTab& t) { return *t.g; }
#define SK(f) sk_read<(uint32_t)offsetof(DevSim, f)>(S, [](const DevSim& d_) -> decltype(auto) { return (d_.f); })
// element i (a constant) of an array field
#define SKE(f, i) \
  sk_read<(uint32_t)(offsetof(DevSim, f) + (i) * sizeof(DevSim::f[0]))>(S, [](const DevSim& d_) -> decltype(auto) { return (d_.f[i]); })
template <uint32_t kApp>
constexpr bool kKtab = kApp == SGN_TRAFFIC_TGEN;  // (PERIODIC: 249-251 VGPRs, no room for four more)

template <class SV>
__device__ __forceinline__ uint32_t bucket_of(const SV& S, uint64_t t) {
  return (uint32_t)SK(bw_div).div(t - SIM_START) & (SK(NB) - 1);
}

// CoDel control law (router/codel_queue.rs:285-298)
__device__ __forceinline__ uint64_t codel_law(uint64_t time, uint64_t count) {
  double sq = count == 0 ? 1.0 : sqrt((double)count);
  double div = 100000000.0 / sq;
  uint64_t inc = (uint64_t)round(div);
  uint64_t orig = time - SIM_START;
  uint64_t adj = orig + inc;
  if (adj < orig || adj > SIMTIME_MAX) adj = SIMTIME_MAX;
  return SIM_START + adj;
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uint32_t lo = __shfl_xor((uint32_t)v, off, 64);
    uint32_t hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
    uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

// wave-uniform values (the same in every lane) into scalar registers: vector registers are the
// round kernels' scarce resource
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return ((uint64_t)uni32((uint32_t)(v >> 32)) << 32) | uni32((uint32_t)v);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uint32_t lo = __shfl_xor((uint32_t)v, off, 64);
    uint32_t hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
    uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

// ---- a big slab's order key: Shadow's (time, src host, src event id) (core/work/event.rs:84-155)
// as one 160-bit string (time - tmin, src, eid) in three words, for a radix select over it ----
struct BigKey {
  uint64_t hi, mid, lo;  // time - tmin | src << 32 | eid >> 32 | eid << 32 (low 32 bits zero)
};
__device__ __forceinline__ BigKey big_key(const EvRec& r, uint64_t tmin) {
  return {r.time - tmin, ((uint64_t)r.src << 32) | (r.eid >> 32), r.eid << 32};
}
__device__ __forceinline__ bool bk_less(const BigKey& a, const BigKey& b) {
  return a.hi != b.hi ? a.hi < b.hi : a.mid != b.mid ? a.mid < b.mid : a.lo < b.lo;
}
// the 8-bit digit at bit p from the top (p a multiple of 8, < 192)
__device__ __forceinline__ uint32_t bk_digit(const BigKey& k, uint32_t p) {
  const uint64_t w = p < 64 ? k.hi : p < 128 ? k.mid : k.lo;
  return (uint32_t)(w >> (56 - (p & 63))) & 0xFFu;
}
__device__ __forceinline__ BigKey bk_set_digit(BigKey k, uint32_t p, uint32_t d) {
  const uint64_t v = (uint64_t)d << (56 - (p & 63));
  if (p < 64) k.hi |= v; else if (p < 128) k.mid |= v; else k.lo |= v;
  return k;
}
// k with every bit below the top p set (the largest key with k's top p bits)
__device__ __forceinline__ uint64_t bk_fill_w(uint64_t w, int keep) {
  return keep >= 64 ? w : keep <= 0 ? ~0ULL : (w | (~0ULL >> keep));
}
__device__ __forceinline__ BigKey bk_fill(const BigKey& k, uint32_t p) {
  return {bk_fill_w(k.hi, (int)p), bk_fill_w(k.mid, (int)p - 64), bk_fill_w(k.lo, (int)p - 128)};
}
// the masks of a key's top p bits (wave-uniform: scalar registers)
__device__ __forceinline__ BigKey bk_mask(uint32_t p) {
  auto m = [](int keep) -> uint64_t { return keep >= 64 ? ~0ULL : keep <= 0 ? 0ULL : ~(~0ULL >> keep); };
  return {m((int)p), m((int)p - 64), m((int)p - 128)};
}
__device__ __forceinline__ bool bk_prefix_eq(const BigKey& a, const BigKey& b, const BigKey& m) {
  return (((a.hi ^ b.hi) & m.hi) | ((a.mid ^ b.mid) & m.mid) | ((a.lo ^ b.lo) & m.lo)) == 0;
}
// the key fields of a record written by another workgroup (device-scope loads)
__device__ __forceinline__ void ld_dev_key(SGN_GLB const EvRec* p, uint64_t& t, uint64_t& e, uint32_t& src) {
  SGN_GLB uint64_t* q = (SGN_GLB uint64_t*)p;
  t = ld_dev(q);
  e = ld_dev(q + 1);
  src = (uint32_t)ld_dev(q + 2);
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int off) {
  const uint32_t lo = __shfl_xor((uint32_t)v, off, 64);
  const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), off, 64);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// block-wide (256 threads) minimum, result valid in every thread
__device__ __forceinline__ uint64_t block_min_u64(uint64_t v, uint64_t* sh) {
  v = wave_min_u64(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  uint64_t r = sh[0];
  const int nw = blockDim.x >> 6;
  for (int i = 1; i < nw; i++) r = sh[i] < r ? sh[i] : r;
  __syncthreads();
  return r;
}

struct Pkt {
  uint32_t src;
  uint32_t dst_ip;
  uint32_t payload;
  uint32_t tag;
  uint64_t eid;
};

// ------------------------------------------------------------------------------------
// Per-host executor: the host's whole state lives in registers for the round.
// ------------------------------------------------------------------------------------
// A lane's LDS slot: the pending digest runs and the digests themselves (touched once per
// run), and the CoDel queue's cached head and open tail runs.

// The wave's outbox: event records for this shard's calendar, placed after the event loop
// by all 64 lanes at once (one round trip for all the slab reservations of the wave instead
// of one per send in the sending lane's serial path). A full outbox falls back to placing
// the record at once.
// Its size is per kernel: 40 records for TGEN (config C: ~100 of 1563 server groups send more
// than 24 records a round, up to ~90; same-box A/B 24 -> 40: -0.5 % per launch, and 40 still
// leaves C at 7 workgroups per CU), 24 for the others (config D's PERIODIC kernel must keep 8
// workgroups per CU WITH its bucket-minimum table of 256 buckets: at 48 records the table no
// longer fit and D ran 3.4x slower; 32 measured the same as 24, round 4).
// a forwarding step of more packets than this waits for the wave's other lanes (HostExec::run)
#ifndef SGN_TRAIN_WAIT
#define SGN_TRAIN_WAIT 8
#endif
constexpr uint32_t kTrainWait = SGN_TRAIN_WAIT;
// PERIODIC forwarding waits only in waves with at least this many lanes in their event loops
#ifndef SGN_FWD_WAIT_LANES
#define SGN_FWD_WAIT_LANES 24
#endif
constexpr uint32_t kFwdWaitLanes = SGN_FWD_WAIT_LANES;
template <uint32_t kApp>
#ifndef SGN_OBOX_PERIODIC
#define SGN_OBOX_PERIODIC 24
#endif
constexpr uint32_t kObox = kApp == SGN_TRAFFIC_TGEN ? 40 : kApp == SGN_TRAFFIC_PERIODIC ? SGN_OBOX_PERIODIC : 24;
struct OutboxHdr {
  uint32_t n;          // records appended (may exceed the outbox: those were placed directly)
  uint64_t xmin;       // earliest run exported to another shard this round (multi-shard)
  uint64_t hz;         // calendar horizon: a run at or after it would alias a live bucket
  SGN_GLB uint64_t* keepmin;  // minimum of this round's new runs for the window's last bucket
  uint32_t* bmin;             // LDS minima per bucket (+ [NB]: the spare slab) or null (below),
  uint64_t bbase;             // ... as offsets from this time (the round's window start)
  uint64_t pg_avail;          // CoDel page pool: free-ring entries allocations may use this round
  SGN_GLB uint64_t* pg_freed; // ... and the round's freed-page counter
  SGN_GLB uint64_t* pg_allocd;// ... and allocated-page counter (the round edge's guard)
  SGN_GLB uint64_t* spilled;  // runs this round put in the calendar's spill area
  SGN_GLB uint32_t* xn;       // multi-shard: this round's per-peer run counters
  uint32_t* xc;               // k_rounds_x: this workgroup's runs per peer this round (LDS; null:
                              // no inbox bins, every remote run goes to its peer's slot)
  uint32_t xbuf;              // ... and the peer blocks they go to (XPeer::runs[xbuf])
};
template <uint32_t N>
struct OutboxN : OutboxHdr {
  EvRec rec[N];
  uint32_t idx[N];  // (slab set, group) slab index
};
template <uint32_t kApp>
using Outbox = OutboxN<kObox<kApp>>;
#ifdef SGN_EXP_NOPAIR  // cost experiment (build_exp.sh): one lane per outbox record
constexpr bool kPairOff = true;
#else
constexpr bool kPairOff = false;
#endif

// A run whose calendar slab is full goes to the spill area with its slab index (lossless; the
// round edge holds and the host re-lays the calendar out before the run can be due). Only a
// full spill area is an overflow.
template <class SV>
__device__ __forceinline__ void spill_run(const SV& S, OutboxHdr* ob, uint32_t idx, const EvRec& r) {
  SGN_GLB Ctrl* C = SK(ctrl);
  const uint64_t i = __hip_atomic_fetch_add(&C->spill_n, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ob) cnt_add(ob->spilled, 1);
  if (i < SK(spill_cap)) {
    st_dev_rec(SK(spill) + i, r);
    st_dev(&SK(spill_idx)[i], idx);
  } else if ((atomicOr(&C->overflow, OVF_BUCKET) & OVF_BUCKET) == 0) {
    C->overflow_info = r.dst;
  }
}

// A run at position pos >= CAP of slab idx: the slab's extension when it has room, else the
// spill area (lossless either way).
template <class SV>
__device__ __forceinline__ void place_overflow(const SV& S, OutboxHdr* ob, uint32_t idx, uint32_t pos,
                                               const EvRec& r) {
  if (SK(ext)) {
    const uint64_t x = SK(ext)[idx];
    const uint32_t k = pos - SK(CAP);
    if (k < (uint32_t)(x >> 40)) {
      st_dev_rec(SK(ext_pool) + (x & EXT_OFF_MASK) + k, r);
      return;
    }
  }
  spill_run(S, ob, idx, r);
}

// LDS copies of queue entries need only 8-byte alignment (a 16-byte-aligned member would
// pad every lane's slot to a multiple of 16 B and cost a workgroup per CU)
// (copies between them and the 16-byte-aligned global entries are compiled as 8-byte LDS
// pairs, ds_write2_b64 / ds_read2_b64; clang's align-mismatch note on them is expected)
#pragma clang diagnostic ignored "-Walign-mismatch"
typedef CodelEnt CodelEnt8 __attribute__((aligned(8)));
typedef FifoEnt FifoEnt8 __attribute__((aligned(8)));
// Per-lane state in the lane's LDS slot or, for the PERIODIC kernels (configs B and D, whose
// occupancy LDS limits: config D's 15,625 groups on the resident grid), elsewhere (every
// field keeps its full width: no limit beyond the reference's):
// * CoDel drop state (interval end, drop next, current / previous count): the PERIODIC
//   kernels keep it in the host record only (HostRec::cq_*, touched only when the queue
//   stands);
// * route cache, token-bucket increments, app counter, send-queue head index: the PERIODIC
//   kernels keep them in registers (they have ~40 VGPRs to spare below the 256 of two waves
//   per SIMD; the TGEN kernel, whose occupancy is fine, keeps its registers).
// Config D's per-workgroup LDS went 26.1 -> 23.1 -> 20.0 KB: 6 -> 7 -> 8 workgroups per CU.
struct LaneCq {
  uint64_t cq[4];
};
struct LaneNoCq {};
struct LaneRc {
  uint64_t rc_lat;   // route cache: latency and loss threshold (send_batch) ...
  uint64_t rc_T;
  uint64_t tbc[2];   // token buckets' refill increments (capacity = increment + MTU)
  uint64_t app_k;    // synthetic app counter
  uint32_t rc_dst;   // ... to this peer (NO_HOST: none)
  uint32_t rc_sid;   // ... whose slot id is this
  uint32_t fh_idx;   // the send queue head copy's ring index (NO_HOST: none)
};
struct LaneNoRc {};
template <uint32_t kApp>
constexpr bool kRcReg = kApp == SGN_TRAFFIC_PERIODIC;
// the hot host line in per-64-host tiles, field-major (DevSim::htile, hot_idx): every chunk load
// or store of a wave is one contiguous access instead of one line per lane. PERIODIC only:
// same-box A/B, D 4.45 -> 4.61 G, B +0.3 %; the TGEN kernel of config C
// measured 1.1 % slower (its cold lines are read with the hot one anyway)
template <uint32_t kApp>
constexpr bool kSoa = kApp == SGN_TRAFFIC_PERIODIC;  // (TGEN with them in registers: C unchanged)
// the kernels whose sends fold their bucket minima in an LDS table (S.agg_bmin, flush_bmin):
// PERIODIC (configs B and D: ~1 M sends a round on a few bucket words at D). TGEN has the LDS
// since round 3's slimmer lane slots, but measured 2 % slower with the table on C.
template <uint32_t kApp>
constexpr bool kAggBmin = kApp == SGN_TRAFFIC_PERIODIC;
// a pending digest run (sgn_drun of sgn_workload.h) with its count kept apart (LaneLDS::rn):
// sgn_drun's 4-byte count pads it to 32 bytes, three of them 12 bytes of every lane's slot
struct DRunL {
  uint64_t a, b, c;
};
template <uint32_t kApp>
struct LaneLDS : std::conditional_t<kApp == SGN_TRAFFIC_PERIODIC, LaneNoCq, LaneCq>,
                 std::conditional_t<kRcReg<kApp>, LaneNoRc, LaneRc> {
  DRunL run[3];      // tx, rx, app pending runs (sgn_workload.h) ...
  uint64_t dig[3];   // tx, rx, app digests
  CodelEnt8 hd, tl;  // head run being consumed / tail run being extended
  FifoEnt8 fh;       // copy of the send queue's head entry (ring index: LaneRc::fh_idx)
  uint32_t cq_tp;    // CoDel chain's tail page
  uint32_t rn[3];    // ... and their counts
};

// A slab with more due runs than the LDS holds (a hot spot: thousands of sources sending to one
// host group within a bucket width) is ordered and executed in pieces of at most CAP runs in
// Shadow's key order: piece k holds the runs with keys in (bound k-1, bound k]. The piece state
// lives in LDS across the pieces' event loops (registers are the round kernel's scarce resource:
// nothing of it is live in registers across HostExec::run, which reads the piece's tail time
// and flush flag from here — INVALID and 1 outside the big-slab path).
struct BigLDS {
  uint64_t tmin, range;  // earliest due run's time, latest - earliest
  uint64_t kp[3];        // the last piece's upper bound (BigKey)
  uint64_t ib;           // the slab
  uint64_t tail;         // run(): a host's next packet time after its runs of this piece
  uint64_t spill_imp;    // spill-area entries that may hold imported runs (multi-shard): set by
                         // the round kernels (k_import's count, or k_rounds_x's after its imports)
  uint32_t ndue, done, have_prev, nraw, flush, pad;
};

// kTrace: the per-packet trace can be on (k_execute). The persistent k_rounds is built
// without it (its registers are fully used; a traced run executes round by round).
// kApp: the traffic kind (SGN_TRAFFIC_*), fixed per instantiation so that each kernel
// carries only its application's code (fewer registers, no dead branches).
template <bool kTrace, uint32_t kApp, class SV = DevSim>
struct HostExec {
  const SV& S;
  SGN_GLB Ctrl* C;
  uint32_t h, gid, my_ip, my_unode;
  uint64_t now, we;
  uint32_t b1, keep_slab;  // the window's last bucket (its new events go to the spare slab)
  // RNG (host/host.rs:234) and counters (host.rs:259-263)
  uint64_t r0, r1, r2, r3;
  uint64_t eid;
  uint64_t st0, st1, st2, se0, se1, se2;  // local event slots: relay out, relay in, app
  uint32_t fl;
  uint32_t ro_dst, ro_pay, ro_tag;
  uint32_t ri_src, ri_pay, ri_tag;
  uint64_t ri_eid;
  uint64_t tbb0, tbl0, tbb1, tbl1;  // balances / last refills (capacity, increment: memory)
  uint32_t cq_head, cq_nr, cq_len;  // head run's pool index (page * CQ_PAGE + offset), runs, packets queued
  uint64_t cq_bytes;  // (CoDel drop state: the lane's LDS slot)
  uint32_t fq_head, fq_len;
  // per-round counter increments (a host cannot see 2^32 events in one window)
  uint32_t c_sent, c_loss, c_popped, c_deliv, c_localev, c_maxcodel;
  uint32_t c_runs;  // event runs this host appended to this shard's calendar (occupancy)
  uint64_t c_bytes;
  // CoDel run cache: the head run being consumed and the tail run being extended live in
  // registers; their ring slots are stale until store() (or until the tail is closed).
  bool hd_valid, tl_open;
  // state touched O(1) times per run lives in this lane's LDS slot (registers are the
  // scarce resource: they set how many waves are resident)
  LaneLDS<kApp>* L;
  std::conditional_t<kRcReg<kApp>, LaneRc, LaneNoRc> rr;  // (see LaneLDS)
  __device__ __forceinline__ LaneRc& lr() {
    if constexpr (kRcReg<kApp>) return rr;
    else return *L;
  }
  __device__ __forceinline__ const LaneRc& lr() const {
    if constexpr (kRcReg<kApp>) return rr;
    else return *L;
  }
  SGN_GLB HostRec* R;     // this host's record (set by load())
  const uint16_t* bslab;  // LDS copy of the bucket -> slab table (when NB <= LDS_BSLAB)
  Outbox<kApp>* ob;       // the wave's outbox (LDS)
  const BigLDS* bg;       // the big-slab piece state (LDS)
#ifdef SGN_DIAG
  uint32_t dgt[DGT_N];
  uint32_t wk[5];
#endif

  __device__ HostExec(const SV& s, uint32_t hh, uint64_t w, uint32_t bucket1, uint32_t ks,
                      LaneLDS<kApp>* l, const uint16_t* bs, Outbox<kApp>* o, const BigLDS* b)
      : S(s), C(SK(ctrl)), h(hh), now(0), we(w), b1(bucket1), keep_slab(ks), L(l), bslab(bs), ob(o), bg(b) {}

  // the host's state into registers (once per round, only for hosts with something due);
  // fresh = false: a reload after park() (the pending digest runs in LDS continue)
  __device__ __forceinline__ void load(bool fresh = true) {
    R = SK(hrec) + h;
    const HostRec& r = *R;
    if constexpr (kApp == SGN_TRAFFIC_PERIODIC) {
      const HostConst& k = SK(hconst)[h];
      gid = k.gid;
      my_ip = k.ip;
      my_unode = k.unode;
      lr().tbc[0] = k.tb_inc[0];
      lr().tbc[1] = k.tb_inc[1];
    } else {  // (in the cold lines these kinds read anyway)
      gid = r.k_gid;
      my_ip = r.k_ip;
      my_unode = r.k_unode;
      lr().tbc[0] = r.k_tbinc[0];
      lr().tbc[1] = r.k_tbinc[1];
    }
    // the hot line
    if constexpr (kSoa<kApp>) {
      const SGN_GLB u64x2* T = (const SGN_GLB u64x2*)SK(htile) + hot_idx(h, 0);
      // (chunk 7 first: the flags decide the cold loads below; then the rest in order of use)
      const u64x2 c7 = T[448];
      fl = (uint32_t)c7.y;
      cq_head = (uint32_t)(c7.y >> 32);
      lr().app_k = c7.x;
      const u64x2 c0 = T[0], c1 = T[64], c2 = T[128], c3 = T[192], c4 = T[256], c5 = T[320], c6 = T[384];
      r0 = c0.x;
      r1 = c0.y;
      r2 = c1.x;
      r3 = c1.y;
      eid = c2.x;
      st2 = c2.y;
      se2 = c3.x;
      tbb0 = c3.y;
      tbb1 = c4.x;
      tbl0 = c4.y;
      tbl1 = c5.x;
      L->dig[0] = c5.y;
      L->dig[1] = c6.x;
      L->dig[2] = c6.y;
    } else {
    r0 = r.rng[0];
    r1 = r.rng[1];
    r2 = r.rng[2];
    r3 = r.rng[3];
    eid = r.eid;
    st2 = r.st2;
    se2 = r.se2;
    fl = r.flags;
    tbb0 = r.tb_bal[0];
    tbl0 = r.tb_last[0];
    tbb1 = r.tb_bal[1];
    tbl1 = r.tb_last[1];
    cq_head = r.cq_head;
    lr().app_k = r.app_k;
    L->dig[0] = r.dig[0];
    L->dig[1] = r.dig[1];
    L->dig[2] = r.dig[2];
    }
    // the cold lines (PERIODIC: only when the host ended its last round with state there)
    if (kApp != SGN_TRAFFIC_PERIODIC || (fl & F_COLD)) {
      st0 = r.st0;
      st1 = r.st1;
      se0 = r.se0;
      se1 = r.se1;
      ro_dst = r.ro_dst;
      ro_pay = r.ro_pay;
      ro_tag = r.ro_tag;
      ri_src = r.ri_src;
      ri_pay = r.ri_pay;
      ri_tag = r.ri_tag;
      ri_eid = r.ri_eid;
      L->cq_tp = r.cq_tp;
      cq_nr = r.cq_nr;
      cq_len = r.cq_len;
      cq_bytes = r.cq_bytes;
      fq_head = r.fq_head;
      fq_len = r.fq_len;
      lr().rc_dst = r.rc_dst;
      lr().rc_sid = r.rc_sid;
      lr().rc_lat = r.rc_lat;
      lr().rc_T = r.rc_T;
      if constexpr (kApp != SGN_TRAFFIC_PERIODIC) {
        L->cq[0] = r.cq_ie;
        L->cq[1] = r.cq_dn;
        L->cq[2] = r.cq_cur;
        L->cq[3] = r.cq_prev;
      }
    } else {  // an idle host: both relays idle, no cached packets, both queues empty
      st0 = st1 = INVALID;
      se0 = se1 = 0;
      ro_dst = ro_pay = ro_tag = ri_src = ri_pay = ri_tag = 0;
      ri_eid = 0;
      L->cq_tp = cq_head / CQ_PAGE;  // (an empty queue keeps its page: head and tail)
      cq_nr = cq_len = 0;
      cq_bytes = 0;
      fq_head = fq_len = 0;
      lr().rc_dst = NO_HOST;
      lr().rc_sid = 0;
      lr().rc_lat = lr().rc_T = 0;
    }
    c_sent = c_loss = c_popped = c_deliv = c_localev = c_bytes = 0;
    c_runs = 0;
    c_maxcodel = kApp == SGN_TRAFFIC_PERIODIC ? 0u : r.max_codel;
    hd_valid = tl_open = false;
    if (cq_nr > 0) {
      L->hd = ld_dev_cq(cq_head_slot());
      hd_valid = true;
    }
    lr().fh_idx = NO_HOST;
    if (fq_len > 0) {
      L->fh = *fq_slot(0);
      lr().fh_idx = fq_head;
    }
    if (fresh) L->rn[0] = L->rn[1] = L->rn[2] = 0;
#ifdef SGN_DIAG
    for (int i = 0; i < DGT_N; i++) dgt[i] = 0;
    for (int i = 0; i < 5; i++) wk[i] = 0;
#endif
  }

  // PERIODIC traffic: the app's next datagram goes to a peer that is a hash of the app counter
  // (sgn_periodic_dst), so its route can be in the route cache before the event loop needs it.
  // store() leaves that peer in S.npeer; the next round's prefetch_peer(np) issues the peer's
  // load beside the host record's (one round trip for both, not one after the other);
  // prefetch_route() (after the gather's sort, so the load's latency hides behind it) fetches
  // the route entry. A cache fill only: the entry is a pure function of (this host's node, the
  // peer), so a hint that is not the next peer costs a miss, never a different result.
  uint32_t pf_peer;
  uint64_t pf_pi;
  // a peer's slot id | used-node index << 32: from the 4-byte table when sim_init built one
  // (half the bytes of the 8-byte one: config D's 1 M-host table is 4 MB, about an XCD's L2)
  __device__ __forceinline__ uint64_t peer_info(uint32_t dst) const {
    if (SK(peer32)) {
      const uint32_t v = SK(peer32)[dst];
      return (v & ((1u << SK(peer_sb)) - 1u)) | ((uint64_t)(v >> SK(peer_sb)) << 32);
    }
    return SK(peer)[dst];
  }
  __device__ __forceinline__ void prefetch_peer(uint32_t np) {
    pf_peer = np;
    pf_pi = np != NO_HOST ? peer_info(np) : 0;
  }
  __device__ __forceinline__ uint32_t next_peer() const {
    uint32_t peer = NO_HOST, uip = 0;
    if (!periodic_dst(lr().app_k, &peer, &uip)) peer = NO_HOST;
    return peer;
  }
  // sgn_periodic_dst / sgn_tgen_fetch (sgn_workload.h) with the remainders by multiply-high
  // (u64 % is a long software routine on the GPU; the results are the same integers)
  __device__ __forceinline__ uint64_t mod_by(const UDiv64& d, uint64_t x, uint64_t n) const { return x - d.div(x) * n; }
  __device__ __forceinline__ bool periodic_dst(uint64_t k, uint32_t* peer, uint32_t* uip) const {
    const uint64_t r = sgn_flow_hash(SK(flow_seed), gid, k);
    if ((uint32_t)mod_by(SK(div_1000), r, 1000u) < SK(unknown_permille)) {
      *uip = SGN_UNKNOWN_IP_BASE + (uint32_t)((r >> 32) & 0xFFFFu);
      return false;
    }
    *peer = (uint32_t)mod_by(SK(div_n), r >> 16, SK(n_all));
    return true;
  }
  __device__ __forceinline__ void prefetch_route() {
    if (pf_peer == NO_HOST) return;
    const RouteEnt re = SK(route)[(size_t)my_unode * SK(U) + (uint32_t)(pf_pi >> 32)];
    lr().rc_dst = pf_peer;
    lr().rc_sid = (uint32_t)pf_pi;
    lr().rc_lat = re.lat;
    lr().rc_T = re.T;
  }

  // old_next / old_peer: this host's S.nextloc / S.npeer as the round read them (a value that did
  // not change is not stored again: a host-round that only took deliveries writes neither,
  // and at config B's 16-host waves each was a partial-line write of its own)
  __device__ __forceinline__ void store(uint64_t old_next, uint32_t old_peer) {
    HostRec& r = *R;
    if constexpr (!kSoa<kApp>) {
    r.rng[0] = r0;
    r.rng[1] = r1;
    r.rng[2] = r2;
    r.rng[3] = r3;
    r.eid = eid;
    r.st2 = st2;
    r.se2 = se2;
    r.tb_bal[0] = tbb0;
    r.tb_bal[1] = tbb1;
    r.tb_last[0] = tbl0;
    r.tb_last[1] = tbl1;
    r.dig[0] = L->dig[0];
    r.dig[1] = L->dig[1];
    r.dig[2] = L->dig[2];
    r.app_k = lr().app_k;
    r.cq_head = cq_head;
    }
    if (fl & F_FH_DIRTY) *fq_slot(0) = L->fh;  // a queued head that lived in LDS
    // the cold lines: PERIODIC writes them only when the host leaves state there (load() gives
    // an idle host its defaults: this must list every field that differs from them)
    const bool cold = kApp != SGN_TRAFFIC_PERIODIC || st0 != INVALID || st1 != INVALID ||
                      (fl & (F_RO_STATE | (3u << F_RI_STATE_SHIFT) | F_RO_NEXT | F_RI_NEXT | F_CODEL_IE |
                             F_CODEL_DN | F_CODEL_DROP)) ||
                      cq_nr || cq_len || cq_bytes || fq_len || fq_head;
    if constexpr (kSoa<kApp>) {
      SGN_GLB u64x2* T = (SGN_GLB u64x2*)SK(htile) + hot_idx(h, 0);
      const uint32_t f = (fl & ~(F_FH_DIRTY | F_COLD)) | (cold ? F_COLD : 0u);
      T[0] = u64x2{r0, r1};
      T[64] = u64x2{r2, r3};
      T[128] = u64x2{eid, st2};
      T[192] = u64x2{se2, tbb0};
      T[256] = u64x2{tbb1, tbl0};
      T[320] = u64x2{tbl1, L->dig[0]};
      T[384] = u64x2{L->dig[1], L->dig[2]};
      T[448] = u64x2{lr().app_k, (uint64_t)f | ((uint64_t)cq_head << 32)};
    } else {
      r.flags = (fl & ~(F_FH_DIRTY | F_COLD)) | (cold ? F_COLD : 0u);
    }
    if (cold) {
      r.st0 = st0;
      r.st1 = st1;
      r.se0 = se0;
      r.se1 = se1;
      r.ri_eid = ri_eid;
      r.cq_bytes = cq_bytes;
      r.rc_lat = lr().rc_lat;
      r.rc_T = lr().rc_T;
      r.ro_dst = ro_dst;
      r.ro_pay = ro_pay;
      r.ro_tag = ro_tag;
      r.ri_src = ri_src;
      r.ri_pay = ri_pay;
      r.ri_tag = ri_tag;
      r.cq_tp = L->cq_tp;
      r.cq_nr = cq_nr;
      r.cq_len = cq_len;
      r.fq_head = fq_head;
      r.fq_len = fq_len;
      r.rc_dst = lr().rc_dst;
      r.rc_sid = lr().rc_sid;
      if constexpr (kApp != SGN_TRAFFIC_PERIODIC) {
        r.cq_ie = L->cq[0];
        r.cq_dn = L->cq[1];
        r.cq_cur = L->cq[2];
        r.cq_prev = L->cq[3];
      }
    }
    // the per-host totals: PERIODIC no-return adds into dense arrays (no load of the old
    // value, no cold line); the other kinds in their cold lines
    if constexpr (kApp == SGN_TRAFFIC_PERIODIC) {
#ifndef SGN_EXP_NOCNT  // (cost experiments only, build_exp.sh: the traffic of each per-host stream)
      const size_t nH = SK(nH);
      if (c_sent) cnt_add(&SK(n_cnt)[N_SENT * nH + h], c_sent);
      if (c_popped) cnt_add(&SK(n_cnt)[N_POPPED * nH + h], c_popped);
      if (c_deliv) cnt_add(&SK(n_cnt)[N_DELIVERED * nH + h], c_deliv);
      if (c_maxcodel)
        (void)__hip_atomic_fetch_max(&SK(maxq)[h], c_maxcodel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    } else {
      r.max_codel = c_maxcodel;
      r.n_sent += c_sent;
      r.n_popped += c_popped;
      r.n_delivered += c_deliv;
    }
#ifndef SGN_EXP_NONEXT
    const uint64_t nl = next_local_time();
    if (nl != old_next) SK(nextloc)[h] = nl;
    if (kApp == SGN_TRAFFIC_PERIODIC) {
      const uint32_t p = next_peer();
      if (p != old_peer) SK(npeer)[h] = p;
    }
#endif
    if (hd_valid) st_dev_cq(cq_head_slot(), L->hd);
    if (tl_open) st_dev_cq(cq_tail_slot(), L->tl);
  }

  // The register state is dead from here (a big slab's passes run with the whole register file;
  // park: the state went to memory with store(), and loaded lanes reload it): constants in every
  // field that load() defines, on every path, so no earlier value stays live across the passes.
  __device__ __forceinline__ void kill() {
    gid = my_ip = my_unode = 0;
    r0 = r1 = r2 = r3 = eid = 0;
    st0 = st1 = st2 = se0 = se1 = se2 = 0;
    fl = ro_dst = ro_pay = ro_tag = ri_src = ri_pay = ri_tag = 0;
    ri_eid = tbb0 = tbl0 = tbb1 = tbl1 = 0;
    cq_head = cq_nr = cq_len = fq_head = fq_len = 0;
    cq_bytes = 0;
    c_sent = c_loss = c_popped = c_deliv = c_localev = c_maxcodel = c_runs = 0;
    c_bytes = 0;
    hd_valid = tl_open = false;
    if constexpr (kRcReg<kApp>) rr = LaneRc{};
    pf_peer = 0;
    pf_pi = 0;
    R = nullptr;
  }



  __device__ __forceinline__ uint64_t next_local_time() const {
    uint64_t m = st0;
    m = st1 < m ? st1 : m;
    m = st2 < m ? st2 : m;
    return m;
  }

  // ---- Xoshiro256++ (rand_xoshiro 0.7.0) + rand 0.9.2 StandardUniform f64 ----
  __device__ __forceinline__ uint64_t rng_next() {
    const uint64_t result = xoshiro_out(r0, r3);
    xoshiro_step(r0, r1, r2, r3);
    return result;
  }
  __device__ __forceinline__ void rng_skip() { xoshiro_step(r0, r1, r2, r3); }  // rng_next without its output
  // rng_next's high word without the carry out of its low word (the true high word is this
  // or this + 1): three VALU ops where the whole output takes six
  __device__ __forceinline__ uint32_t rng_next_hi_nc() {
    const uint32_t h = xoshiro_out_hi_nc(r0, r3);
    xoshiro_step(r0, r1, r2, r3);
    return h;
  }
  __device__ __forceinline__ double rng_f64() {
    return (double)(rng_next() >> 11) * 0x1.0p-53;
  }

  // A traced simulation runs the kTrace kernels only, and sgn_sim_init sets F_TRACED in the flags
  // of every host it traces — all of them, or those sgn_trace_hosts listed; load() / store() carry
  // the bit like the other constant ones. (Testing DevSim::trace_on as well, 1 = all / 2 = flagged,
  // measured 5 % slower on a full trace than the parent's test of trace_on alone; this form runs at
  // the parent's rate)
  __device__ __forceinline__ bool tr() const {
    if constexpr (!kTrace) return false;
    return (fl & F_TRACED) != 0u;
  }
  __device__ __forceinline__ void trace(uint32_t kind, uint32_t peer, uint32_t flags, uint64_t a, uint64_t b,
                        uint64_t c) {
    if (!tr()) return;
    const uint64_t seq = R->tseq++;
    uint64_t pos = atomicAdd((unsigned long long*)&C->trace_n, 1ULL);
    if (pos >= SK(trace_cap)) {
      atomicOr(&C->overflow, OVF_TRACE);
      return;
    }
    sgn_trace_rec r;
    r.kind = kind;
    r.host = gid;
    r.peer = peer;
    r.flags = flags;
    r.a = a;
    r.b = b;
    r.c = c;
    r.seq = seq;
    r.rng_pos = R->rng_pos;
    SK(trace)[pos] = r;
  }

  __device__ __forceinline__ void overflow(uint32_t bit) {
    if ((atomicOr(&C->overflow, bit) & bit) == 0) C->overflow_info = gid;
  }

  // EXTERNAL traffic: a datagram's fate for the CPU-side applications (sgn_drain)
  __device__ __forceinline__ void drain_rec(uint32_t status, uint32_t src, uint32_t dst, uint64_t seid,
                            uint32_t payload, uint32_t tag) {
    const uint64_t pos = atomicAdd((unsigned long long*)&C->drain_n, 1ULL);
    if (pos >= SK(drain_cap)) {
      overflow(OVF_DRAIN);
      return;
    }
    sgn_drain_rec r;
    r.time = now;
    r.src_eid = seid;
    r.handle = 0;
    r.host = gid;
    r.src_host = src;
    r.dst_host = dst;
    r.status = status;
    r.payload_len = payload;
    r.tag = tag;
    SK(drain)[pos] = r;
  }
  __device__ __forceinline__ bool external() const { return kApp == SGN_TRAFFIC_EXTERNAL; }

  // ---- local event slots: Host::schedule_task_* / push_local_event (host.rs:703-722);
  //      Event::new_local consumes an event id even if the event is then dropped ----
  template <int SL>
  __device__ __forceinline__ void schedule(uint64_t t) {
    uint64_t e = eid++;
    if (t >= SK(end_time)) return;
    if (SL == SLOT_RO) { st0 = t; se0 = e; }
    if (SL == SLOT_RI) { st1 = t; se1 = e; }
    if (SL == SLOT_APP) { st2 = t; se2 = e; }
  }

  template <int W>
  __device__ __forceinline__ uint32_t relay_state() const {
    return W == 0 ? (fl & 3u) : ((fl >> F_RI_STATE_SHIFT) & 3u);
  }
  template <int W>
  __device__ __forceinline__ void set_relay_state(uint32_t v) {
    if (W == 0)
      fl = (fl & ~3u) | v;
    else
      fl = (fl & ~(3u << F_RI_STATE_SHIFT)) | (v << F_RI_STATE_SHIFT);
  }

  // Relay::notify (relay/mod.rs:111-136) and forward_later (:145-163)
  template <int W>
  __device__ __forceinline__ void forward_later(uint64_t delay) {
    set_relay_state<W>(RELAY_PENDING);
    schedule<W == 0 ? SLOT_RO : SLOT_RI>(now + delay);
  }
  template <int W>
  __device__ __forceinline__ void relay_notify() {
    if (relay_state<W>() == RELAY_IDLE) forward_later<W>(0);
  }

  // ---- TokenBucket::comforming_remove (network/relay/token_bucket.rs:65-154) ----
  // n comforming_remove(dec) calls at one `now`, n >= 1 packets of one wire length: how many
  // conform. Only the first call can refill (`now` does not move), so after it balance / dec
  // conform in all; when fewer than n do, *dur is the conforming duration the first refused
  // call returns. One instance of the refill and one of the duration per call site.
  template <int W>
  __device__ __forceinline__ uint32_t tb_take(uint64_t dec, uint32_t n, uint64_t* dur) {
    DGT_BEGIN(tt);
    const uint32_t m = tb_take_<W>(dec, n, dur);
    DGT_END(DGT_TBRM, tt);
    return m;
  }
  template <int W>
  __device__ __forceinline__ uint32_t tb_take_(uint64_t dec, uint32_t n, uint64_t* dur) {
    uint64_t& bal = W == 0 ? tbb0 : tbb1;
    uint64_t& last = W == 0 ? tbl0 : tbl1;
    const uint64_t interval = 1000000ULL;  // relay/mod.rs:279
    // lazy_refill. The refill increment and capacity stay in memory (they are only read
    // when a refill is due or a removal fails, not on the per-packet fast path).
    uint64_t span = now - last;
    if (span >= interval) {
      const uint64_t inc = lr().tbc[W];
      uint64_t nref = span / interval;
      uint64_t ntok = mul_sat(inc, nref, ~0ULL);
      uint64_t b = bal + ntok;
      if (b < bal) b = ~0ULL;
      const uint64_t cap = inc + SGN_CONFIG_MTU;  // every relay's bucket: sim_init
      bal = b > cap ? cap : b;
      uint64_t adv = mul_sat(interval, nref, SIMTIME_MAX);
      last = emu_sat_add(last, adv);
      span = now - last;
    }
    const uint32_t m = tb_conforming(bal, dec, n);
    bal -= (uint64_t)m * dec;
    if (m < n) {
      // compute_conforming_duration (:91-117) of the refused removal: dec > bal, so
      // 0 < req <= dec and at least one refill is needed (tb_refills: never 0)
      const uint64_t next_refill_span = interval - span;
      const uint64_t nr = tb_refills(dec - bal, lr().tbc[W]);
      if (nr == 1)
        *dur = next_refill_span;
      else {
        uint64_t a = mul_sat(interval, nr - 1, SIMTIME_MAX);
        uint64_t s = next_refill_span + a;
        if (s < next_refill_span || s > SIMTIME_MAX) s = SIMTIME_MAX;
        *dur = s;
      }
    }
    return m;
  }

  // sgn_drun_{flush,add}_{seq,same} (sgn_workload.h) over LaneLDS::run / rn
  template <int K>
  __device__ __forceinline__ void dr_flush_seq() {
#ifndef SGN_EXP_NODIGEST
    const uint32_t n = L->rn[K];
    if (n) L->dig[K] = sgn_digest3(L->dig[K], L->run[K].a, L->run[K].b | ((uint64_t)n << 32), L->run[K].c - n);
    L->rn[K] = 0;
#endif
  }
  template <int K>
  __device__ __forceinline__ void dr_flush_same() {
#ifndef SGN_EXP_NODIGEST
    const uint32_t n = L->rn[K];
    if (n) L->dig[K] = sgn_digest3(L->dig[K], L->run[K].a, L->run[K].b | ((uint64_t)n << 34), L->run[K].c);
    L->rn[K] = 0;
#endif
  }
  template <int K>
  __device__ __forceinline__ void dr_add_seq(uint64_t a, uint64_t b, uint64_t c0, uint32_t n) {
#ifndef SGN_EXP_NODIGEST
    DRunL& r = L->run[K];
    if (L->rn[K] && r.a == a && r.b == b && r.c == c0) {
      L->rn[K] += n;
      r.c += n;
      return;
    }
    dr_flush_seq<K>();
    r.a = a;
    r.b = b;
    r.c = c0 + n;
    L->rn[K] = n;
#endif
  }
  template <int K>
  __device__ __forceinline__ void dr_add_same(uint64_t a, uint64_t b, uint64_t c, uint32_t n) {
#ifndef SGN_EXP_NODIGEST
    DRunL& r = L->run[K];
    if (L->rn[K] && r.a == a && r.b == b && r.c == c) {
      L->rn[K] += n;
      return;
    }
    dr_flush_same<K>();
    r.a = a;
    r.b = b;
    r.c = c;
    L->rn[K] = n;
#endif
  }

  // the CoDel drop state (LaneCq / HostRec::cq_*, see LaneLDS)
  template <int I>
  __device__ __forceinline__ uint64_t cqg() const {
    if constexpr (kApp == SGN_TRAFFIC_PERIODIC)
      return I == 0 ? R->cq_ie : I == 1 ? R->cq_dn : I == 2 ? R->cq_cur : R->cq_prev;
    else
      return L->cq[I];
  }
  template <int I>
  __device__ __forceinline__ void cqs(uint64_t v) {
    if constexpr (kApp == SGN_TRAFFIC_PERIODIC) {
      if (I == 0) R->cq_ie = v;
      if (I == 1) R->cq_dn = v;
      if (I == 2) R->cq_cur = v;
      if (I == 3) R->cq_prev = v;
    } else {
      L->cq[I] = v;
    }
  }

  // ---- CoDel (router/codel_queue.rs) on a chain of pool pages ----
  // The queue's runs in order fill the head page from cq_head's offset, whole pages, and the
  // tail page (L->cq_tp) up to run cq_nr - 1; only the head and tail runs are ever touched.
  __device__ __forceinline__ SGN_GLB CodelEnt* cq_head_slot() { return SK(codel) + cq_head; }
  __device__ __forceinline__ SGN_GLB CodelEnt* cq_tail_slot() {
    return SK(codel) + ((size_t)L->cq_tp * CQ_PAGE + ((cq_head + cq_nr - 1) & (CQ_PAGE - 1)));
  }
  // a page from the pool: the free ring's next entry, if it was freed before this round
  // (the entries of the current round are still being written by other waves)
  __device__ __forceinline__ uint32_t cq_alloc_page() {
    DGT_BEGIN(ta);
    const uint64_t i = __hip_atomic_fetch_add(&C->pg_alloc, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cnt_add(ob->pg_allocd, 1);
    if (i >= ob->pg_avail) return NO_HOST;
    const uint32_t pg = ld_dev(&SK(cq_free)[umod64(SK(div_cq), i, SK(cq_pages))]);
#ifdef SGN_DIAG
    DGT_WAIT();
    DGT_END(DGT_CQALLOC, ta);
#endif
    return pg;
  }
  __device__ __forceinline__ void cq_free_page(uint32_t pg) {
    DGT_BEGIN(tf);
    const uint64_t j = __hip_atomic_fetch_add(&C->pg_tail, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    st_dev(&SK(cq_free)[umod64(SK(div_cq), j, SK(cq_pages))], pg);
    cnt_add(ob->pg_freed, 1);
    DGT_END(DGT_CQFREE, tf);
  }
  // the head run left the queue: next run, next page (the old one back to the pool), or an
  // empty queue that keeps its page from the start
  __device__ __forceinline__ void cq_pop_head() {
    cq_nr--;
    if (cq_nr == 0) {
      cq_head &= ~(CQ_PAGE - 1);
      L->cq_tp = cq_head / CQ_PAGE;
    } else if (((cq_head + 1) & (CQ_PAGE - 1)) != 0) {
      cq_head++;
    } else {
      const uint32_t pg = cq_head / CQ_PAGE;
      const uint32_t nx = ld_dev(&SK(cq_next)[pg]);  // (neighbouring links belong to other hosts)
      cq_free_page(pg);
      cq_head = nx * CQ_PAGE;
    }
  }
  // Router::route_incoming_packet (router/mod.rs:55-57) -> CoDelQueue::push (:303-317) for a
  // run of n packets arriving at `now`: extends the open tail run when it continues it.
  __device__ __forceinline__ void codel_push_run(uint32_t src, uint64_t eid0, uint32_t payload, uint32_t tag,
                                 uint32_t n) {
    const auto continues = [&](const CodelEnt& r) {
      return r.enqueue_ts == now && r.src == src && r.eid + r.count == eid0 &&
             r.payload == payload && r.tag == tag;
    };
    if (tl_open && continues(L->tl)) {
      L->tl.count += n;
    } else if (!tl_open && hd_valid && cq_nr == 1 && continues(L->hd)) {
      L->hd.count += n;
    } else {
      if (tl_open) {
        st_dev_cq(cq_tail_slot(), L->tl);
        tl_open = false;
      }
      if (cq_nr > 0 && ((cq_head + cq_nr) & (CQ_PAGE - 1)) == 0) {
        // the tail page is full: link a page from the pool
        const uint32_t np = cq_alloc_page();
        if (np == NO_HOST) {
          overflow(OVF_CODEL);
          return;
        }
        st_dev(&SK(cq_next)[L->cq_tp], np);
        L->cq_tp = np;
      }
      L->tl.enqueue_ts = now;
      L->tl.eid = eid0;
      L->tl.src = src;
      L->tl.payload = payload;
      L->tl.tag = tag;
      L->tl.count = n;
      tl_open = true;
      cq_nr++;
    }
    cq_len += n;
    cq_bytes += (uint64_t)n * ((uint64_t)payload + sgn_header_bytes(tag));
    if (cq_len > c_maxcodel) c_maxcodel = cq_len;
  }
  // process_standing_delay (:231-262)
  __device__ __forceinline__ bool codel_standing(uint64_t sd) {
    if (sd < CODEL_TARGET || cq_bytes <= SGN_CONFIG_MTU) {
      fl &= ~F_CODEL_IE;
      return false;
    }
    if (fl & F_CODEL_IE) return now >= cqg<0>();
    fl |= F_CODEL_IE;
    cqs<0>(emu_sat_add(now, CODEL_INTERVAL));
    return false;
  }
  // the head run into registers (queue not empty)
  __device__ __forceinline__ void load_head() {
    if (hd_valid) return;
    if (tl_open && cq_nr == 1) {  // the only run is the open tail: take it over
      L->hd = L->tl;
      tl_open = false;
    } else {
      DG(DG_HDLOAD);
      DGT_BEGIN(th);
      L->hd = ld_dev_cq(cq_head_slot());
      DGT_WAIT();
      DGT_END(DGT_HDLD, th);
    }
    hd_valid = true;
  }
  // codel_pop (:204-227)
  __device__ __forceinline__ bool codel_pop_raw(Pkt* p, bool* ok_to_drop) {
    if (cq_len == 0) {
      fl &= ~F_CODEL_IE;
      return false;
    }
    load_head();
    const CodelEnt e = L->hd;
    L->hd.eid++;
    if (--L->hd.count == 0) {
      hd_valid = false;
      cq_pop_head();
    }
    cq_len--;
    cq_bytes = sat_sub(cq_bytes, (uint64_t)e.payload + sgn_header_bytes(e.tag));
    *ok_to_drop = codel_standing(sat_sub(now, e.enqueue_ts));
    p->src = e.src;
    p->dst_ip = my_ip;
    p->payload = e.payload;
    p->tag = e.tag;
    p->eid = e.eid;
    return true;
  }
  __device__ __forceinline__ void codel_drop(const Pkt& p) {  // drop_packet (:319-321)
    cnt_add(&R->n_codel, 1);
    if (external()) drain_rec(SGN_DRAIN_CODEL, p.src, gid, p.eid, p.payload, p.tag);
    dr_add_seq<2>(now, (uint64_t)p.src | (1ULL << 63), p.eid, 1);
    trace(SGN_TRACE_CODEL_DROP, p.src, 0, now, 0, p.eid);
  }
  __device__ __forceinline__ bool codel_was_dropping_recently() const {  // :273-281
    if (!(fl & F_CODEL_DN)) return false;
    return sat_sub(now, cqg<1>()) < CODEL_INTERVAL * 16;
  }
  // CoDelQueue::pop (:125-201)
  __device__ __forceinline__ bool codel_pop(Pkt* out) {
    Pkt p;
    bool okd;
    if (!codel_pop_raw(&p, &okd)) {
      fl &= ~F_CODEL_DROP;
      return false;
    }
    if (!okd) {
      fl &= ~F_CODEL_DROP;
      *out = p;
      return true;
    }
    if (!(fl & F_CODEL_DROP)) {
      // drop_from_store_mode (:150-170)
      codel_drop(p);
      Pkt n;
      bool nok;
      bool has_n = codel_pop_raw(&n, &nok);
      fl |= F_CODEL_DROP;
      uint64_t delta = sat_sub(cqg<2>(), cqg<3>());
      const uint64_t cur = (codel_was_dropping_recently() && delta > 1) ? delta : 1;
      cqs<2>(cur);
      fl |= F_CODEL_DN;
      cqs<1>(codel_law(now, cur));
      cqs<3>(cur);
      if (has_n) *out = n;
      return has_n;
    }
    // drop_from_drop_mode (:172-201)
    bool has_item = true;
    Pkt item = p;
    while (has_item && (fl & F_CODEL_DROP) && (fl & F_CODEL_DN) && now >= cqg<1>()) {
      codel_drop(item);
      cqs<2>(cqg<2>() + 1);
      bool iok = false;
      has_item = codel_pop_raw(&item, &iok);
      if (has_item && iok)
        cqs<1>(codel_law(cqg<1>(), cqg<2>()));
      else
        fl &= ~F_CODEL_DROP;
    }
    if (has_item) *out = item;
    return has_item;
  }

  // ---- synthetic socket send queue (interface qdisc source for relay_inet_out) ----
  __device__ __forceinline__ FifoEnt* fq_slot(uint32_t i) {
    uint32_t idx = fq_head + i;
    if (idx >= SK(fifo_cap)) idx -= SK(fifo_cap);
    return SK(fifo) + (size_t)h * SK(fifo_cap) + idx;
  }
  // dst NO_HOST: a datagram to `addr`, an address outside the simulation (the trace keeps
  // it in a side array, S.fifo_addr, for the capture record)
  __device__ __forceinline__ bool fifo_push(uint32_t dst, uint32_t payload, uint32_t last, uint32_t count,
                            uint32_t tag, uint32_t addr = 0) {
    if (fq_len >= SK(fifo_cap)) return false;
    if (tr() && dst == NO_HOST) SK(fifo_addr)[fq_slot(fq_len) - SK(fifo)] = addr;
    FifoEnt e;
    e.dst = dst;
    e.pay = (payload & 0xFFFFu) | (last << 16);
    e.count = count;
    e.tag = tag;
    if (fq_len == 0) {
      // the new head lives in LDS only: most are sent within the round, and a global store
      // here would hold up the wave's next dependent load (stores and loads share vmcnt);
      // store() writes it back if it is still queued
      L->fh = e;
      lr().fh_idx = fq_head;
      fl |= F_FH_DIRTY;
    } else {
      *fq_slot(fq_len) = e;
    }
    fq_len++;
    return true;
  }
  // the head entry (from the LDS copy when it is current)
  __device__ __forceinline__ FifoEnt fifo_head() {
    if (lr().fh_idx == fq_head) return L->fh;
    DGT_BEGIN(tf);
    const FifoEnt e = *fq_slot(0);
    DGT_WAIT();
    DGT_END(DGT_FHLD, tf);
    L->fh = e;
    lr().fh_idx = fq_head;
    return e;
  }

  // ---- Dns::addr_to_host_id (network/dns.rs:174) ----
  __device__ __forceinline__ bool dns_lookup(uint32_t ip, uint32_t* host) const {
    uint32_t i = (ip * 0x9E3779B1u) & SK(dns_mask);
    while (true) {
      uint32_t k = SK(dns_key)[i];
      if (k == ip) {
        *host = SK(dns_val)[i];
        return true;
      }
      if (k == 0) return false;
      i = (i + 1) & SK(dns_mask);
    }
  }

  // interface delivery to the synthetic app (NetworkInterface::push -> socket) of m packets
  // from src with consecutive event ids e0.. at `now` (one run-encoded app digest step)
  __device__ __forceinline__ void deliver_run(uint32_t src, uint64_t e0, uint32_t m, uint32_t payload,
                              uint32_t tag) {
    c_deliv += m;
    c_bytes += (uint64_t)m * payload;
    dr_add_seq<2>(now, src, e0, m);
    if (tr())
      for (uint32_t k = 0; k < m; k++)
        trace(SGN_TRACE_DELIVER, src, 0, now, (uint64_t)payload | ((uint64_t)tag << 32), e0 + k);
    if (external())
      for (uint32_t k = 0; k < m; k++) drain_rec(SGN_DRAIN_DELIVERED, src, gid, e0 + k, payload, tag);
    if (kApp == SGN_TRAFFIC_TGEN && (fl & F_SERVER) && (tag & SGN_TAG_REQ)) {
      const uint32_t c = tag & 3u;  // the class picks one of three (scalar) sizes
      const uint64_t size = c == 0 ? SKE(file_bytes, 0) : (c == 1 ? SKE(file_bytes, 1) : SKE(file_bytes, 2));
      const uint64_t n = (size + SGN_TGEN_MSS - 1) / SGN_TGEN_MSS;
      if (n == 0) return;
      const uint32_t last = (uint32_t)(size - (n - 1) * SGN_TGEN_MSS);
      for (uint32_t k = 0; k < m; k++) {
        if (fifo_push(src, SGN_TGEN_MSS, last, (uint32_t)n, SGN_TAG_RESP))
          relay_notify<0>();
        else
          cnt_add(&R->n_blocked, 1);
      }
    }
  }
  __device__ __forceinline__ void deliver_local(const Pkt& p) {  // loopback: a digest run of its own
    cnt_add(&R->n_local_deliv, 1);
    if (tr()) trace(SGN_TRACE_LOCAL, gid, 0, now, (uint64_t)p.payload | ((uint64_t)p.tag << 32), 0);
    if (external()) drain_rec(SGN_DRAIN_LOCAL, gid, gid, 0, p.payload, p.tag);
    dr_flush_seq<2>();
    L->dig[2] = sgn_digest3(L->dig[2], now, (uint64_t)p.src | (1ULL << 62) | (1ULL << 32), p.payload);
  }

  // ---- Relay::forward_until_blocked (network/relay/mod.rs:201-273) for relay_inet_in:
  //      the router's CoDel queue -> the interface (relay_inet_out uses forward_out) ----
  __device__ __forceinline__ bool forward_in(uint64_t* dur) {
    const bool boot = now < SK(boot_end);
    set_relay_state<1>(RELAY_FORWARDING);
    while (true) {
      Pkt p;
      if (fl & F_RI_NEXT) {
        fl &= ~F_RI_NEXT;
        p.src = ri_src;
        p.dst_ip = my_ip;
        p.payload = ri_pay;
        p.tag = ri_tag;
        p.eid = ri_eid;
      } else {
        if (cq_len > 0) {
          load_head();
          // Fast path over the head run: every packet of it has the same standing delay and
          // wire size, and all removals happen at the same `now`. CoDelQueue::pop returns
          // each of them (codel_queue.rs:125-262) unless the delay is standing (>= TARGET)
          // past an interval end that is already due: below TARGET it clears interval_end
          // and drop mode; at or above it clears drop mode and only moves interval_end (set
          // to now + INTERVAL by the first pop that leaves more than an MTU queued, cleared
          // by the first that leaves less; the queued bytes only fall here, so the last pop
          // decides). After the first comforming_remove (which applies the lazy refill)
          // balance / wire more packets conform; the first that does not is cached.
          // In drop mode before drop_next, pop returns every packet without a drop too
          // (drop_from_drop_mode's loop does not run, :172-201) and changes nothing until a
          // pop leaves <= MTU queued (then interval_end and drop mode end).
          const bool standing = sat_sub(now, L->hd.enqueue_ts) >= CODEL_TARGET;
          const bool ie_due = (fl & F_CODEL_IE) && now >= cqg<0>();
          const bool drop_quiet = (fl & F_CODEL_DROP) && (fl & F_CODEL_DN) && now < cqg<1>();
          if (!standing || !ie_due || drop_quiet) {
            const uint32_t n = L->hd.count;
            const uint64_t wire = (uint64_t)L->hd.payload + sgn_header_bytes(L->hd.tag);
            uint32_t m = n;
            bool blocked = false;
            if (!boot) {
              m = tb_take<1>(wire, n, dur);
              blocked = m < n;
            }
            const uint32_t used = m + (blocked ? 1u : 0u);
            const CodelEnt r = L->hd;
            L->hd.eid += used;
            L->hd.count -= used;
            cq_len -= used;
            cq_bytes = sat_sub(cq_bytes, (uint64_t)used * wire);
            if (!standing || cq_bytes <= SGN_CONFIG_MTU) {
              fl &= ~(F_CODEL_IE | F_CODEL_DROP);
            } else if (!ie_due) {
              fl &= ~F_CODEL_DROP;
              if (!(fl & F_CODEL_IE)) {
                fl |= F_CODEL_IE;
                cqs<0>(emu_sat_add(now, CODEL_INTERVAL));
              }
            }  // else drop mode before drop_next: unchanged
            if (L->hd.count == 0) {
              hd_valid = false;
              cq_pop_head();
            }
            if (m) deliver_run(r.src, r.eid, m, r.payload, r.tag);
            if (blocked) {
              fl |= F_RI_NEXT;
              ri_src = r.src;
              ri_pay = r.payload;
              ri_tag = r.tag;
              ri_eid = r.eid + m;
              set_relay_state<1>(RELAY_IDLE);
              return true;
            }
            continue;
          }
        }
        const bool gotp = codel_pop(&p);
        if (!gotp) {
          set_relay_state<1>(RELAY_IDLE);
          return false;
        }
        DG(DG_FQLOAD);
      }
      // the source address is the router's (0.0.0.0), never this host's: no local bypass
      if (!boot && tb_take<1>((uint64_t)p.payload + sgn_header_bytes(p.tag), 1, dur) == 0) {
        fl |= F_RI_NEXT;
        ri_src = p.src;
        ri_pay = p.payload;
        ri_tag = p.tag;
        ri_eid = p.eid;
        set_relay_state<1>(RELAY_IDLE);
        return true;
      }
      deliver_run(p.src, p.eid, 1, p.payload, p.tag);
    }
  }

  // A run of n identical datagrams pushed to the router at the same `now`: n consecutive
  // Worker::send_packet calls (core/worker.rs:330-403). The DNS lookup, route entry,
  // reliability and delivery time are the same for all of them, so they are computed
  // once; the per-packet loss draws stay sequential (same RNG stream, same order) and the
  // digest takes runs of equal outcomes. Sent packets take consecutive source event ids and
  // share one delivery time, so their events are reserved with one atomic and written as
  // one contiguous run.
  // pop: (trace) the index of the first packet that was just popped from the interface (an
  // IF_POP record precedes its SEND record, as NetworkInterface::pop precedes send_packet);
  // the packets before it were popped earlier (a cached packet), NO_POP: none was
  static constexpr uint32_t NO_POP = ~0u;
  __device__ __forceinline__ void send_batch(uint32_t dst, uint32_t payload, uint32_t tag, uint32_t n,
                                             uint32_t pop = NO_POP) {
    DGT_BEGIN(t0);
    send_batch_(dst, payload, tag, n, pop);
    DGT_END(DGT_SEND, t0);
  }
  // one loss-draw outcome of send_batch_'s record-free path (tx digest runs only)
  __device__ __forceinline__ void loss_step(bool lost, uint32_t& run, uint32_t& sent, uint32_t dst,
                                            uint64_t deliver) {
    if (lost) {
      c_loss++;
      if (run) dr_add_same<0>(now, (uint64_t)dst, deliver, run);
      run = 0;
      dr_add_same<0>(now, (uint64_t)dst | (1ULL << 32), 0, 1);
    } else {
      run++;
      sent++;
    }
  }
  // dst: the HostId the address resolves to (FifoEnt), NO_HOST: not in the simulation
  // IF_POP of the send queue's head entry (an unknown address from the trace's side array)
  __device__ __forceinline__ void trace_pop(uint32_t dst, uint32_t payload, uint32_t tag) {
    trace(SGN_TRACE_IF_POP, dst, 0, now, (uint64_t)payload | ((uint64_t)tag << 32),
          dst == NO_HOST ? SK(fifo_addr)[fq_slot(0) - SK(fifo)] : 0);
  }
  __device__ __forceinline__ void send_batch_(uint32_t dst, uint32_t payload, uint32_t tag, uint32_t n, uint32_t pop) {
    if (n == 0 || now >= SK(end_time)) return;
    DG(DG_BATCH);
    const bool boot = now < SK(boot_end);
    // (only the TGEN kernels send a cached packet with popped ones: elsewhere pop is 0 or NO_POP)
    const auto popped = [&](uint32_t j) { return kApp == SGN_TRAFFIC_TGEN ? j >= pop : pop == 0; };
    if (dst == NO_HOST) {  // resolve_ip_to_host_id failed: InetDropped (worker.rs:347-357)
      cnt_add(&R->n_unknown, n);
      dr_add_same<0>(now, 0xFFFFFFFFULL | (2ULL << 32), 0, n);
      if (tr())
        for (uint32_t j = 0; j < n; j++) {
          if (popped(j)) trace_pop(NO_HOST, payload, tag);
          trace(SGN_TRACE_SEND, 0xFFFFFFFFu, 2, now, 0, 0);
        }
      if (external())
        for (uint32_t j = 0; j < n; j++) drain_rec(SGN_DRAIN_UNKNOWN, gid, NO_HOST, 0, payload, tag);
      return;
    }
    // the route (WorkerShared::latency / reliability, worker.rs:523-537): a train goes to
    // one peer for many rounds, so the host keeps its last (peer, latency, threshold)
    uint64_t delay, T;
    uint32_t dsid;  // the destination's slot id (where its events are filed)
    if (lr().rc_dst == dst) {
      delay = lr().rc_lat;
      T = lr().rc_T;
      dsid = lr().rc_sid;
    } else {
      DG(DG_RMISS);
      DGT_BEGIN(trt);
      // the peer's slot and used node (one load), then its route entry (one 16-byte load):
      // drop iff chance >= reliability (worker.rs:366-371) with chance = (x >> 11) * 2^-53;
      // reliability = (f64)(1.0f - loss) is 0 or >= 2^-24, so reliability * 2^53 is an exact
      // integer T (precomputed per route, sim_init) and the test is (x >> 11) >= T, bit for
      // bit the same decision
      const uint64_t pi = peer_info(dst);
      dsid = (uint32_t)pi;
      const RouteEnt re = SK(route)[(size_t)my_unode * SK(U) + (uint32_t)(pi >> 32)];
      delay = re.lat;
      T = re.T;
      DGT_WAIT();
      DGT_END(DGT_RTLD, trt);
      lr().rc_dst = dst;
      lr().rc_sid = dsid;
      lr().rc_lat = delay;
      lr().rc_T = T;
    }
    uint64_t deliver = now + delay;
    if (deliver < we) deliver = we;
    const uint64_t eid0 = eid;
    const bool can_drop = !boot && payload > 0;
    uint32_t run = 0;  // consecutive sent packets not yet folded into the digest
    DGT_BEGIN(tr0);
#ifdef SGN_DIAG
    dgt[DGT_DRAWS] += n;
    if ((uint32_t)(__ffsll((long long)__ballot(1)) - 1) == (threadIdx.x & 63)) dgt[DGT_RENTRY] += 1;
    {
      const uint64_t lb = __ballot(n > kTrainWait);
      if (n > kTrainWait) dgt[DGT_LLANE] += 1;
      if (lb && (uint32_t)(__ffsll((long long)lb) - 1) == (threadIdx.x & 63)) dgt[DGT_LENTRY] += 1;
    }
#endif
#ifdef SGN_EXP_NORNG
    if (true) {
      run = n;
      eid += n;
    } else
#endif
    if (tr() || external()) {  // per-packet records
      for (uint32_t j = 0; j < n; j++) {
        if (tr() && popped(j)) trace_pop(dst, payload, tag);
        const uint64_t x = rng_next() >> 11;
        if (tr()) R->rng_pos++;
        if (can_drop && x >= T) {
          c_loss++;
          if (run) dr_add_same<0>(now, (uint64_t)dst, deliver, run);
          run = 0;
          dr_add_same<0>(now, (uint64_t)dst | (1ULL << 32), 0, 1);
          if (tr()) trace(SGN_TRACE_SEND, dst, 1, now, 0, 0);
          if (external()) drain_rec(SGN_DRAIN_LOSS, gid, dst, 0, payload, tag);
        } else {
          const uint64_t e = eid++;
          run++;
          if (tr()) trace(SGN_TRACE_SEND, dst, 0, now, deliver, e);
        }
      }
    } else if (!can_drop || T >= (1ULL << 53)) {
      // nothing can drop (bootstrapping, empty payload, or a lossless path: chance < 1.0 =
      // reliability always); the draws still advance the stream (worker.rs:366 draws first)
#pragma unroll 8
      for (uint32_t j = 0; j < n; j++) rng_skip();
      run = n;
      eid += n;
    } else {
      // x >> 11 >= T  <=>  x >= T << 11 (T < 2^53); eight, then four draws per test
      const uint64_t Tx = T << 11;
      uint32_t sent = 0, j = 0;
      // eight draws per test (same-box A/B on config C: +1.3 % over four, sixteen was slower;
      // the loop's scalar control and test sit on the slowest waves' chain). The test is a
      // screen: a draw drops only if its high word is >= Tx's, and the high word is at most
      // the carry-less one + 1, so when the eight carry-less high words' maximum + 1 is below
      // Tx's high word none drops; otherwise the eight draws are redone exactly from the saved
      // state (probability ~ 8 x the path's loss). The stream advances the same either way.
      // Paths losing more than 1/32 of their packets would redo most batches (~1.7x the
      // exact test's cost), so they keep the exact test below. Same-box A/B: C -2.2 % per
      // launch (3486 -> 3411 us); micro-benchmark 126 -> 87 cycles per draw for a lone lane.
      // (TGEN kernel only: its servers send trains; a PERIODIC host sends single datagrams,
      // and the screen's registers took that kernel from 231 to 256 VGPRs)
      const uint32_t Th = (uint32_t)(Tx >> 32);
      if (kApp == SGN_TRAFFIC_TGEN && Th >= 0xF8000000u) for (; j + 8 <= n; j += 8) {
        const uint64_t a0 = r0, a1 = r1, a2 = r2, a3 = r3;
        const uint32_t h0 = rng_next_hi_nc(), h1 = rng_next_hi_nc(), h2 = rng_next_hi_nc(), h3 = rng_next_hi_nc();
        const uint32_t h4 = rng_next_hi_nc(), h5 = rng_next_hi_nc(), h6 = rng_next_hi_nc(), h7 = rng_next_hi_nc();
        const uint32_t hm = max(max(max(h0, h1), max(h2, h3)), max(max(h4, h5), max(h6, h7)));
        if (hm >= Th - 1 || Th == 0) {  // (hm + 1 >= Th without the wrap)
          r0 = a0;
          r1 = a1;
          r2 = a2;
          r3 = a3;
          const uint64_t x0 = rng_next(), x1 = rng_next(), x2 = rng_next(), x3 = rng_next();
          const uint64_t x4 = rng_next(), x5 = rng_next(), x6 = rng_next(), x7 = rng_next();
          loss_step(x0 >= Tx, run, sent, dst, deliver);
          loss_step(x1 >= Tx, run, sent, dst, deliver);
          loss_step(x2 >= Tx, run, sent, dst, deliver);
          loss_step(x3 >= Tx, run, sent, dst, deliver);
          loss_step(x4 >= Tx, run, sent, dst, deliver);
          loss_step(x5 >= Tx, run, sent, dst, deliver);
          loss_step(x6 >= Tx, run, sent, dst, deliver);
          loss_step(x7 >= Tx, run, sent, dst, deliver);
        } else {
          run += 8;
          sent += 8;
        }
      }
      for (; j + 8 <= n; j += 8) {
        const uint64_t x0 = rng_next(), x1 = rng_next(), x2 = rng_next(), x3 = rng_next();
        const uint64_t x4 = rng_next(), x5 = rng_next(), x6 = rng_next(), x7 = rng_next();
        if ((x0 >= Tx) | (x1 >= Tx) | (x2 >= Tx) | (x3 >= Tx) | (x4 >= Tx) | (x5 >= Tx) | (x6 >= Tx) |
            (x7 >= Tx)) {
          loss_step(x0 >= Tx, run, sent, dst, deliver);
          loss_step(x1 >= Tx, run, sent, dst, deliver);
          loss_step(x2 >= Tx, run, sent, dst, deliver);
          loss_step(x3 >= Tx, run, sent, dst, deliver);
          loss_step(x4 >= Tx, run, sent, dst, deliver);
          loss_step(x5 >= Tx, run, sent, dst, deliver);
          loss_step(x6 >= Tx, run, sent, dst, deliver);
          loss_step(x7 >= Tx, run, sent, dst, deliver);
        } else {
          run += 8;
          sent += 8;
        }
      }
      for (; j + 4 <= n; j += 4) {
        const uint64_t x0 = rng_next(), x1 = rng_next(), x2 = rng_next(), x3 = rng_next();
        if ((x0 >= Tx) | (x1 >= Tx) | (x2 >= Tx) | (x3 >= Tx)) {
          loss_step(x0 >= Tx, run, sent, dst, deliver);
          loss_step(x1 >= Tx, run, sent, dst, deliver);
          loss_step(x2 >= Tx, run, sent, dst, deliver);
          loss_step(x3 >= Tx, run, sent, dst, deliver);
        } else {
          run += 4;
          sent += 4;
        }
      }
      for (; j < n; j++) loss_step(rng_next() >= Tx, run, sent, dst, deliver);
      eid += sent;
    }
    DGT_END(DGT_APP, tr0);
    if (run) dr_add_same<0>(now, (uint64_t)dst, deliver, run);
    const uint32_t nsent = (uint32_t)(eid - eid0);
    if (nsent == 0) return;
    c_sent += nsent;
    // sent packets have consecutive ids (drops take none): one event run record each
    // RUN_MAX packets
    const uint32_t nrec = (nsent + RUN_MAX - 1) / RUN_MAX;
    if (SK(dynamic)) {  // Worker::update_lowest_used_latency (no return value: fire and forget)
      min_nr(&C->min_used, delay);
    }
    SGN_GLB EvRec* dstp;
    uint32_t cap;
    uint32_t pos;
    uint32_t sidx = 0;  // owned: the slab index (its spill tag)
    const bool owned = dst - SK(lo) < SK(nH);
    if (owned) {
      if (deliver >= ob->hz) {  // past the calendar's horizon (sim_init sizes NB so it cannot be)
        overflow(OVF_HORIZON);
        return;
      }
      c_runs += nrec;
      const uint32_t b = bucket_of(S, deliver);
      const uint32_t slab = b == b1 ? keep_slab : (SK(NB) <= LDS_BSLAB ? bslab[b] : ld_dev(&SK(bucket_slab)[b]));
      const size_t idx = (size_t)slab * SK(G) + ((dsid - SK(lo)) >> SK(gsh));
      // the bucket's pending minimum: folded in the workgroup's LDS table when it has one
      // (flush_bmin publishes it before the round's arrival), else one device atomic per run
      // (compiled for PERIODIC traffic only — configs B and D, where every host sends every
      // round; the TGEN kernel of config C keeps its per-run atomic, uncontended there)
      if (kAggBmin<kApp> && SK(agg_bmin))
        atomicMin(&ob->bmin[b == b1 ? SK(NB) : b], (uint32_t)(deliver - ob->bbase));
      else
        min_nr(b == b1 ? ob->keepmin : &SK(bucket_min)[b], deliver);
      if (nrec == 1) {
        const uint32_t k = atomicAdd(&ob->n, 1u);  // LDS
        if (k < kObox<kApp>) {
          EvRec& r = ob->rec[k];
          r.time = deliver;
          r.eid = eid0;
          r.src = gid;
          r.dst = dsid;
          r.pc = payload | (nsent << 16);
          r.tag = tag;
          ob->idx[k] = (uint32_t)idx;
          return;
        }
      }
      DGT_BEGIN(tsl);
      pos = atomicAdd(&SK(slab_n)[idx], nrec);
      DGT_WAIT();
      DGT_END(DGT_SLAB, tsl);
      dstp = SK(pool) + idx * SK(CAP);
      cap = SK(CAP);
      sidx = (uint32_t)idx;
    } else {
      uint32_t lo = 0, hi = SK(n_ranks), lov = 0;  // (rank_lo[0] = 0)
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint32_t v = SK(rank_lo)[mid];
        if (v <= dst) {
          lo = mid;
          lov = v;
        } else {
          hi = mid;
        }
      }
      atomicMin((unsigned long long*)&ob->xmin, (unsigned long long)deliver);  // LDS
      sidx = SPILL_PEER | lo;  // (runs beyond the peer's slot: the slot grows at a held round)
      bool binned = false;
      if (ob->xc) {
        // persistent rounds: the receiving host group's bin in the peer's inbox (its gather
        // reads it next round); a full bin sends the run to the peer's slot instead
        atomicAdd(&ob->xc[lo], nrec);  // LDS
        const uint32_t gr = (dsid - lov) >> SK(gsh);
        pos = atomicAdd(&SK(xbin_n)[((size_t)ob->xbuf * SK(n_ranks) + lo) * SK(xgx) + gr], nrec);
        if (pos + nrec <= SK(xbk)) {
          binned = true;
          dstp = SK(xp)[lo].bins[ob->xbuf] + (size_t)gr * SK(xbk);
          cap = SK(xbk);
        }
      }
      if (!binned) {
        pos = atomicAdd(&ob->xn[lo], nrec);
        // the peer's block: the RCCL transport's send block (after its message records), or the
        // peer's inbox slot for this shard and round parity (persistent rounds: peer-mapped memory)
        dstp = SK(xp)[lo].runs[ob->xbuf];
        cap = ob->xbuf == 2 ? SK(xslot) : SK(xislot);
      }
    }
    for (uint32_t m = 0; m < nrec; m++) {
      const uint32_t k = min(RUN_MAX, nsent - m * RUN_MAX);
      EvRec r;
      r.time = deliver;
      r.eid = eid0 + (uint64_t)m * RUN_MAX;
      r.src = gid;
      r.dst = dsid;
      r.pc = payload | (k << 16);
      r.tag = tag;
      if (pos + m < cap) {
        if (owned || !SK(xsys))
          st_dev_rec(dstp + pos + m, r);
        else  // (another GPU's inbox)
          st_sys_rec(dstp + pos + m, r);
      } else if (owned)  // the slab is full: its extension, or the spill area
        place_overflow(S, ob, sidx, pos + m, r);
      else  // the peer's exchange slot is full
        spill_run(S, ob, sidx, r);
    }
  }

  // Relay::forward_until_blocked for relay_inet_out (network/relay/mod.rs:201-273), taking
  // the send queue a run at a time: a run is the leading datagrams of the head train that
  // share a payload size. All of them see the same `now`, so after the first
  // comforming_remove (which applies the lazy refill) no further refill happens and the
  // number that conform is balance / wire_len; the first that does not is cached exactly
  // like Relay::next_packet.
  // One step = the cached packet or one send-queue entry. The task runs step by step, one
  // step per iteration of the wave's event loop (F_RO_CONT: the host stays inside the task,
  // `now` does not move and none of its other events run until the queue is empty or the
  // bucket blocks), so lanes forwarding long trains send them side by side instead of one
  // after another (a train's per-packet loss draws are the serial part of a round).
  // TGEN: a cached packet that the head entry's run continues (a train the bucket blocked
  // in mid-file: the same peer, tag and size) goes out with that run in one step — one
  // removal from the bucket for both (tb_take's n calls at one `now`), one send_batch: the
  // same draws in the same order, one event run at the receiver instead of two that it
  // would merge again.
  __device__ __forceinline__ bool merges_cached(const FifoEnt& h) const {
    if constexpr (kApp != SGN_TRAFFIC_TGEN) return false;
    const uint32_t hp = h.count == 1 ? (h.pay >> 16) : (h.pay & 0xFFFFu);
    return h.dst == ro_dst && h.tag == ro_tag && hp == ro_pay && ro_dst != gid && !(SK(qdisc_rr) && fq_len > 1);
  }
  __device__ __forceinline__ void forward_out_step() {
    DGT_BEGIN(tf0);
    const bool boot = now < SK(boot_end);
    uint64_t dur = 0;
    bool blocked = false;
    // the cached packet, or the head entry's run: one instance of the bucket and of the send
    // for both (the cached packet is a run of one that is not in the queue)
    const bool cached = (fl & F_RO_NEXT) != 0;
    if (cached || fq_len > 0) {
      FifoEnt e;
      bool rr = false;
      bool merge = false;  // the cached packet and the head entry's run together
      uint32_t run = 1, payload;
      if (cached) {
        fl &= ~F_RO_NEXT;
        e.dst = ro_dst;
        e.tag = ro_tag;
        e.count = 1;
        payload = ro_pay;
        if constexpr (kApp == SGN_TRAFFIC_TGEN) {
          if (fq_len > 0) {
            const FifoEnt h = fifo_head();
            if (merges_cached(h)) {
              merge = true;
              e = h;
              run = h.count == 1 ? 2u : h.count;  // the cached packet + the run
            }
          }
        }
      } else {
        e = fifo_head();
        // round-robin qdisc with other sockets waiting: one packet, then this socket goes to
        // the back (NetworkInterface::pop, interface.rs:216-256); otherwise the leading
        // datagrams of the train that share a payload size
        rr = SK(qdisc_rr) && fq_len > 1;
        run = (e.count == 1 || rr) ? 1u : e.count - 1;
        payload = e.count == 1 ? (e.pay >> 16) : (e.pay & 0xFFFFu);
      }
      const uint64_t wire = (uint64_t)payload + sgn_header_bytes(e.tag);
      const bool is_local = e.dst == gid;
      uint32_t n_ok = run;
      if (!boot && !is_local) {
        n_ok = tb_take<0>(wire, run, &dur);
        blocked = n_ok < run;
      }
      if (is_local) {
        Pkt p;
        p.src = gid;
        p.dst_ip = my_ip;
        p.payload = payload;
        p.tag = e.tag;
        p.eid = 0;
        for (uint32_t j = 0; j < n_ok; j++) {
          if (tr() && !cached) trace_pop(gid, payload, e.tag);
          deliver_local(p);
        }
      } else {
        // (the cached packet was popped before)
        send_batch(e.dst, payload, e.tag, n_ok, merge ? 1u : cached ? NO_POP : 0u);
      }
      // a cached packet alone is not in the send queue, and a merged step that sent nothing
      // leaves the queue as it is (the cached packet stays cached)
      const bool outq = cached && !(merge && n_ok > 0);
      // the packet the bucket refused was popped too: it waits in Relay::next_packet
      if (tr() && blocked && !outq) trace_pop(e.dst, payload, e.tag);
      const uint32_t consumed = n_ok + (blocked ? 1u : 0u) - (merge ? 1u : 0u);
      if (outq) {
        // not in the send queue
      } else if (consumed == e.count) {
        fq_head = fq_head + 1 == SK(fifo_cap) ? 0 : fq_head + 1;
        fq_len--;
        if (fq_len == 0) fq_head = 0;  // (an empty queue's head is 0: an idle host's default)
        fl &= ~F_FH_DIRTY;
      } else if (rr) {
        // the socket still has data: re-queued behind the others (same length)
        FifoEnt m = e;
        m.count = e.count - consumed;
        fq_head = fq_head + 1 == SK(fifo_cap) ? 0 : fq_head + 1;
        *fq_slot(fq_len - 1) = m;
        lr().fh_idx = NO_HOST;  // the cached head is stale
        fl &= ~F_FH_DIRTY;
      } else {
        if (!(fl & F_FH_DIRTY)) fq_slot(0)->count = e.count - consumed;
        L->fh.count = e.count - consumed;
      }
      if (blocked) {
        fl |= F_RO_NEXT;
        ro_dst = e.dst;
        ro_pay = payload;
        ro_tag = e.tag;
      }
    }
    if (blocked || (fq_len == 0 && !(fl & F_RO_NEXT))) {  // the task returns
      fl &= ~F_RO_CONT;
      set_relay_state<0>(RELAY_IDLE);
      if (blocked) forward_later<0>(dur);
    }
    DGT_END(DGT_FWDOUT, tf0);
  }

  // run_forward_task + forward_now (relay/mod.rs:166-187)
  template <int W>
  __device__ __forceinline__ void run_forward_task() {
    set_relay_state<W>(RELAY_IDLE);
    uint64_t dur;
    DGT_BEGIN(t0);
    const bool blocked = forward_in(&dur);
    DGT_END(DGT_FWDIN, t0);
    if (blocked) forward_later<W>(dur);
  }

  __device__ __forceinline__ void app_task() {
    const uint64_t k = lr().app_k++;
    uint32_t dst, payload, tag, uip = 0;
    uint64_t next_delay;
    if (kApp == SGN_TRAFFIC_PERIODIC) {
      uint32_t peer = 0;
      // an address outside the simulation (10.255.0.0/16, never registered) is NO_HOST
      dst = periodic_dst(k, &peer, &uip) ? peer : NO_HOST;
      payload = SK(payload_len);
      tag = SGN_TAG_DATA;
      next_delay = SK(period);
    } else {
      uint32_t si = 0, cls = 0;
      {  // sgn_tgen_fetch
        const uint64_t r = sgn_flow_hash(SK(flow_seed), gid, k);
        si = (uint32_t)mod_by(SK(div_ns), r >> 8, SK(n_servers));
        cls = (uint32_t)((r >> 40) % 3u);
      }
      DGT_BEGIN(tsv);
      dst = SK(servers)[si];
      DGT_WAIT();
      DGT_END(DGT_SVLD, tsv);
      payload = SK(req_payload);
      tag = SGN_TAG_REQ | cls;
      next_delay = sgn_tgen_think(SK(flow_seed), gid, k, SK(period), SK(period_jitter));
    }
    if (fifo_push(dst, payload, payload, 1, tag, uip))
      relay_notify<0>();  // Host::notify_socket_has_packets (host.rs:969-983)
    else
      cnt_add(&R->n_blocked, 1);
    schedule<SLOT_APP>(now + next_delay);
  }

  // EXTERNAL traffic: the application's socket write (sgn_submit) enters the socket send
  // queue and notifies relay_inet_out (Host::notify_socket_has_packets, host.rs:969-983),
  // as app_task does for the synthetic apps. The record carries the destination address in
  // the low half of its event id (the high half is the submission order).
  __device__ __forceinline__ void app_submit(const EvRec& e) {
    uint32_t dst;
    if (!dns_lookup((uint32_t)e.eid, &dst)) dst = NO_HOST;
    const uint32_t payload = ev_payload(e);
    if (fifo_push(dst, payload, payload, 1, e.tag, (uint32_t)e.eid)) {
      relay_notify<0>();
    } else {
      cnt_add(&R->n_blocked, 1);
      drain_rec(SGN_DRAIN_BLOCKED, gid, NO_HOST, 0, payload, e.tag);
    }
  }

  // Is local slot W (0: relay_inet_out, 1: relay_inet_in) due at `now` and the host's next
  // event? No packet run at `now` (pt: the next due run's time) and every other local event
  // later by (time, event id).
  template <int W>
  __device__ __forceinline__ bool next_local_now(uint64_t pt) const {
    const uint64_t t = W == 0 ? st0 : st1, e = W == 0 ? se0 : se1;
    const uint64_t ta = W == 0 ? st1 : st0, ea = W == 0 ? se1 : se0;
    return t == now && pt > now && (ta > now || (ta == now && ea > e)) && (st2 > now || (st2 == now && se2 > e));
  }

  // ---- Host::execute (host.rs:762-830) over the host's due event runs + local slots ----
  // ev[ord[s0 .. s1)] are the host's runs due before `until` in Shadow's order, (time, src
  // host, src event id) (core/work/event.rs:84-155), in LDS; local events run while their
  // time < until. A window is executed as consecutive sub-windows (one per calendar
  // bucket): nothing created inside a window is due in it (packet deliveries are >= the
  // window end, worker.rs:386-390), so this is the same sequence of events.
  // bg->tail: the time of the host's next packet run after ev[ord[s1 - 1]] (INVALID: none) — a
  // slab ordered in pieces (exec_group's big-slab path) runs a host's runs over several calls,
  // each up to the next piece's bound; bg->flush: close the digests' pending runs (the last
  // piece of the sub-window only, so the digest steps are those of one call over all runs)
  __device__ __forceinline__ void run(const EvRec* ev, const uint16_t* ord, uint32_t s0, uint32_t s1,
                      uint64_t until) {
    uint32_t pi = s0;
    // (bg null: kernels without the big-slab path — no later piece, digests close here; the
    // tail is re-read from LDS where it is needed: a register across the loop spilled the
    // PERIODIC big-slab kernel)
    uint64_t pt = pi < s1 ? ev[ord[pi]].time : bg ? bg->tail : INVALID;  // next due packet run's time
#ifdef SGN_DIAG
#endif
    while (true) {
      const uint64_t act = __ballot(1);  // (the wave's lanes still in their event loops)
      // earliest local event by (time, event id)
      uint64_t lt = st0, le = se0;
      int ls = 0;
      if (st1 < lt || (st1 == lt && se1 < le)) { lt = st1; le = se1; ls = 1; }
      if (st2 < lt || (st2 == lt && se2 < le)) { lt = st2; le = se2; ls = 2; }
#ifdef SGN_DIAG
      {  // wave-level: iterations, and iterations in which some lane runs each handler;
         // the previous iteration's cycles are added to its handler combination's slot
        const bool ispop = pi < s1 && ev[ord[pi]].time <= lt;
        const int kind = (fl & F_RO_CONT) ? 1 : ispop ? 0 : (lt >= until ? 4 : 1 + ls);
        const uint64_t act = __ballot(1);
        const uint64_t b0 = __ballot(kind == 0), b1 = __ballot(kind == 1),
                       b2 = __ballot(kind == 2), b3 = __ballot(kind == 3);
        const uint64_t tnow = __builtin_amdgcn_s_memtime();
        if ((uint32_t)(__ffsll((long long)act) - 1) == (threadIdx.x & 63)) {
          wk[0]++;
          wk[1] += b0 != 0;
          wk[2] += b1 != 0;
          wk[3] += b2 != 0;
          wk[4] += b3 != 0;
          // (per-combination cycles: off — a global read-modify-write per iteration would
          // add a dependent round trip to every iteration of the diag build)
        }
        (void)tnow;
      }
#endif
      // inside relay_inet_out's forwarding task: its next step (the one call site of
      // forward_out_step below), no other event of the host
      if (!(fl & F_RO_CONT)) {
        int run_ls;
        if (pi < s1 && pt <= lt) {  // Packet < Local at equal times (event.rs:102-110)
          const EvRec& e = ev[ord[pi]];
          pi++;
          pt = pi < s1 ? ev[ord[pi]].time : bg ? bg->tail : INVALID;  // the next run's time, ahead of need
          now = e.time;
          if (external() && e.src == gid) {  // a CPU application's datagram (sgn_submit)
            app_submit(e);
            continue;
          }
          DG(DG_POPRUN);
          DGT_BEGIN(t0);
          // the run's packets pop back to back (nothing sorts between them); each is
          // routed into CoDel and notifies relay_inet_in, which schedules its task on
          // the first notification only (Relay::notify, relay/mod.rs:111-136)
          const uint32_t n = ev_count(e);
          const uint32_t src = e.src;
          const uint64_t eid0 = e.eid;
          c_popped += n;
          dr_add_seq<1>(now, src, eid0, n);
          if (tr())
            for (uint32_t k = 0; k < n; k++) trace(SGN_TRACE_POP, src, 0, now, 0, eid0 + k);
          // Router::route_incoming_packet (router/mod.rs:55-57)
          codel_push_run(src, eid0, ev_payload(e), e.tag, n);
          relay_notify<1>();  // Host::notify_router_has_packets (host.rs:958-960)
          DGT_END(DGT_POP, t0);
          // the relay_inet_in task at `now` is the host's next event when no packet is due at
          // `now` (Packet < Local at equal times) and no other local event precedes it by
          // (time, event id): it runs in this iteration (the same sequence of events; the wave
          // saves a trip round the loop)
          if (!next_local_now<1>(pt)) continue;
          run_ls = 1;
        } else {
          if (lt >= until) break;
          now = lt;
          run_ls = ls;
        }
        c_localev++;
        if (run_ls != 0) {
          if (run_ls == 1) {
            st1 = INVALID;
            run_forward_task<1>();
          } else {
            st2 = INVALID;
            DGT_BEGIN(t0);
            app_task();
            DGT_END(DGT_LOAD, t0);
          }
          // a send queued at `now` makes relay_inet_out's task the next event: start it here
          if (!next_local_now<0>(pt)) continue;
          c_localev++;
        }
        // run_forward_task for relay_inet_out (relay/mod.rs:166-187): Idle, then Forwarding
        st0 = INVALID;
        set_relay_state<0>(RELAY_FORWARDING);
        fl |= F_RO_CONT;
      }
      // Trains side by side (TGEN: the servers' responses): a lane whose step is a long train
      // waits while other lanes of the wave are still on other events — they may reach a train
      // of their own, and then the trains' per-packet loss draws run in one pass instead of one
      // pass per lane (config C's slowest waves ran their servers' draw loops 3 to 7 times
      // over, diag build). Waiting changes nothing of the host's own sequence: `now` is fixed
      // inside the forwarding task, and other lanes are other hosts.
      if constexpr (kApp == SGN_TRAFFIC_TGEN) {
        // (a cached packet that the head run continues goes out with it: the step's length
        // is then the entry's count as well)
        bool lng = false;
        if (fq_len > 0) {
          const FifoEnt h = fifo_head();
          lng = h.count > kTrainWait && (!(fl & F_RO_NEXT) || merges_cached(h));
        }
        if (lng && __ballot(1) != act) continue;
      }
      // Forwarding side by side (PERIODIC, waves with many lanes in their loops — config D, where
      // every host sends every round): a lane about to forward waits until every lane still in
      // its event loop is about to forward too, so the wave runs the forwarding step once for
      // all of them instead of once per iteration in which some lane reaches it. Same argument as
      // the trains: `now` is fixed inside the forwarding task. Few lanes (config B's waves of 16
      // hosts, 2-6 busy) lose more in extra loop trips than they share (same-box A/B: D +6.4 %,
      // B -1.0 % when every wave waits).
      if constexpr (kApp == SGN_TRAFFIC_PERIODIC) {
        if (__popcll(act) >= kFwdWaitLanes && __ballot(1) != act) continue;
      }
      forward_out_step();
    }
    // the sub-window is done: close the digests' pending runs (sgn_workload.h)
    if (!bg || bg->flush) flush_digests();
  }
  __device__ __forceinline__ void flush_digests() {
    dr_flush_same<0>();
    dr_flush_seq<1>();
    dr_flush_seq<2>();
  }
};

// ------------------------------------------------------------------------------------
// Round kernels
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64);
  const uint32_t hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}

// exclusive position of this lane among the lanes where m has a bit set
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  const uint32_t lane = threadIdx.x & 63;
  return (uint32_t)__popcll(lane ? (m & ((~0ULL) >> (64 - lane))) : 0ULL);
}

template <class SV>
__device__ __forceinline__ uint64_t codel_round_bound(const SV& S, uint64_t occ, uint64_t ws, uint64_t we) {
  const uint32_t nbk = ((bucket_of(S, we - 1) - bucket_of(S, ws)) & (SK(NB) - 1)) + 1;
  const uint64_t capb = (uint64_t)nbk * SK(G) * SK(CAP) + SK(ext_total);
  return codel_pages_bound(occ < capb ? occ : capb, SK(nH));
}
__device__ __forceinline__ uint64_t pages_free(uint64_t avail, uint64_t alloc) {
  return avail > alloc ? avail - alloc : 0;
}

// finalize_round for the fused single-shard path, run by the last wave of k_execute: the
// waves' minima come from the chunk slots; every value another wave changed during this
// launch is read with a device-scope atomic (plain loads could hit a stale L2 line).
// local != 0 (multi-shard): instead of moving the window, the shard's {min next event, min
// used latency} and its per-peer run counts go into the round-edge messages (comm.cpp sends
// them with the runs; k_import's last block reduces them on every shard).
__device__ void finalize_fused(const DevSim& S, uint32_t lane, uint32_t nch, uint64_t ws,
                               uint64_t we, uint32_t ks, uint32_t slab_b1, int local = 0) {
  SGN_GLB Ctrl* C = SK(ctrl);
  const uint32_t b0 = bucket_of(S, ws), b1 = bucket_of(S, we - 1);
  // one round trip: every value to read (chunk minima, spare-slab minimum, bucket minima,
  // lowest used latency) is fetched at once; the buckets [b0, b1) are consumed and b1 is
  // replaced, so neither is read
  uint64_t kk = INVALID, wn = INVALID, m = INVALID, od = 0;
  for (uint32_t i = lane; i < nch; i += 64) {
    const uint64_t a = __hip_atomic_exchange(&SK(fin_keep)[i], (unsigned long long)INVALID,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t b = __hip_atomic_exchange(&SK(fin_next)[i], (unsigned long long)INVALID,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    od += __hip_atomic_exchange(&SK(fin_occ)[i], 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    kk = a < kk ? a : kk;
    wn = b < wn ? b : wn;
  }
  for (uint32_t b = lane; b < SK(NB); b += 64) {
    const bool consumed = ((b - b0) & (SK(NB) - 1)) < ((b1 - b0) & (SK(NB) - 1)) || b == b1;
    if (!consumed) {
      const uint64_t bm = ld_dev(&SK(bucket_min)[b]);
      m = bm < m ? bm : m;
    }
  }
  uint64_t km = INVALID, mu = INVALID;
  if (lane == 0) {
    km = __hip_atomic_exchange(&C->keep_min, (unsigned long long)INVALID, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    mu = ld_dev(&C->min_used);
  }
  kk = wave_min_u64(kk);
  wn = wave_min_u64(wn);
  m = wave_min_u64(m);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) od += shfl_xor64(od, off);
  // then the writes (the caller drains them before publishing the round edge)
  for (uint32_t i = lane; i <= nch; i += 64) st_dev(&SK(fin_cnt)[i], 0u);
  if (lane == 0) {
    for (uint32_t b = b0; b != b1; b = (b + 1) & (SK(NB) - 1))
      st_dev(&SK(bucket_min)[b], (uint64_t)INVALID);  // consumed
    // the spare slab set (survivors + this round's new runs for b1) becomes bucket b1
    st_dev(&SK(bucket_slab)[b1], ks);
    st_dev(&C->keep_slab, slab_b1);
    const uint64_t nb1 = km < kk ? km : kk;
    st_dev(&SK(bucket_min)[b1], nb1);
    // CoDel page pool: the pages freed this round become allocatable in the next
    const uint64_t fr = __hip_atomic_exchange(&C->pg_freed, 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t avail = ld_dev(&C->pg_avail) + fr;
    if (fr) st_dev(&C->pg_avail, avail);
    const uint64_t occ = ld_dev(&C->cal_occ) + od;  // (wraps back from a negative sum)
    st_dev(&C->cal_occ, occ);
    const uint64_t pfree = pages_free(avail, ld_dev(&C->pg_alloc));
    const bool spilled = ld_dev(&C->spill_n) != 0;
    m = nb1 < m ? nb1 : m;
    m = wn < m ? wn : m;
    if (local) {
      // word 3: this shard's largest per-peer run count this round (every shard compares the
      // maxima of all shards with the exchange size: the same decision everywhere), with the
      // spill flag in its high half; words 4-7 let every shard evaluate every shard's CoDel
      // guard for the next window alike (k_import): free pages, calendar occupancy, runs
      // exported this round (a bound on what any shard receives), slab runs per bucket
      uint64_t xmax = 0, xsum = 0;
      for (uint32_t p = 0; p < SK(n_ranks); p++) {
        const uint64_t cnt = p == SK(rank) ? 0 : ld_dev(&SK(xout_n)[p]);
        xmax = cnt > xmax ? cnt : xmax;
        xsum += cnt;
      }
      for (uint32_t p = 0; p < SK(n_ranks); p++) {
        const uint64_t cnt = p == SK(rank) ? 0 : ld_dev(&SK(xout_n)[p]);
        // the message records of the peer's outgoing block (travel with the runs); this
        // shard's own in its incoming block, where k_import reads every shard's message
        SGN_GLB uint64_t* o = (SGN_GLB uint64_t*)((p == SK(rank) ? SK(xin) : SK(xout)) + (size_t)p * (SK(xslot) + XHDR));
        st_dev(o, cnt);
        st_dev(o + 1, m);
        st_dev(o + 2, mu);
        st_dev(o + 3, (uint64_t)(xmax | ((spilled ? 1ULL : 0ULL) << 32)));
        st_dev(o + 4, pfree);
        st_dev(o + 5, occ);
        st_dev(o + 6, xsum);
        st_dev(o + 7, (uint64_t)SK(G) * SK(CAP) + SK(ext_total));
      }
      return;
    }
    const uint64_t min_next = m == INVALID ? EMU_MAX : m;  // unwrap_or(MAX)
    st_dev(&C->last_min_next, min_next);
    const uint64_t ne = window_end(min_next, mu, SK(dynamic), SK(min_possible), SK(runahead_cfg), SK(end_time));
    st_dev(&C->active, min_next < ne ? 1u : 0u);
    if (min_next < ne) {  // the next round's guards (hold before it runs)
      const uint64_t need = codel_round_bound(S, occ, min_next, ne);
      const uint32_t hold = (pfree < need ? HOLD_CODEL : 0u) | (spilled ? HOLD_SPILL : 0u) |
                            (min_next >= ld_dev(&C->pause_at) ? HOLD_PAUSE : 0u);  // (sgn_run_until)
      if (hold) {
        st_dev(&C->hold, hold);
        st_dev(&C->hold_need, need);
      }
    }
    st_dev(&C->prev_we, we);
    st_dev(&C->ws, min_next);
    st_dev(&C->we, ne);
    st_dev(&C->round_min, (uint64_t)INVALID);
    __hip_atomic_fetch_add(&C->rounds, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One wave per host group (GROUP consecutive hosts), lane = host. A round is:
//  1. gather: the group's slabs of the window's buckets are read; runs due in the window go
//     to LDS, the last bucket's later runs move to the spare slab (Ctrl::keep_slab);
//  2. order: counting sort of the due runs by destination lane (LDS atomics + wave scan),
//     then a rank sort inside each destination's segment by (time, src host, src event
//     id) — Shadow's EventQueue order (core/work/event.rs:84-155; keys are unique);
//  3. execute: every lane runs Host::execute (host.rs:762-830) for its host over its
//     segment and local slots, emitting new runs into the calendar / exchange slots;
//  4. the wave's minimum next local event time goes to Ctrl::round_min.
// LDS of the round kernels (one wave per workgroup)
// no-return LDS atomics on a workgroup's statistics (ds_add_u64 / ds_max_u64: the wave does not
// wait for them)
__device__ __forceinline__ void wacc_add(uint64_t* p, uint64_t v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void wacc_max(uint64_t* p, uint64_t v) {
  (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
struct ExecLDS {
  EvRec* lev;         // due runs of one bucket (dynamic LDS, CAP entries)
  uint16_t* lb;       // grouped by destination lane (unordered)
  uint16_t* lc;       // ... ordered inside each destination segment
  uint32_t* lcnt;
  uint32_t* lcur;     // placement cursors (after placement: segment ends, start = end - count)
  void* lslot;        // the lanes' LDS slots (LaneLDS<kApp>[64])
  uint16_t* lbs;      // bucket -> slab table for this round (when NB <= LDS_BSLAB; ids <= NB)
  OutboxHdr* ob;      // the wave's outbox (an Outbox<kApp>)
  uint32_t* bmin;     // per-bucket minima of the workgroup's sends this round (S.agg_bmin) or null
  struct BigLDS* big; // a big slab's piece state (exec_group)
  uint64_t* wacc;     // k_rounds: the workgroup's w_cnt sums (max for W_MAXFILL) over its whole
                      // launch, flushed once at its end; null: exec_group adds to w_cnt itself
};


// One group (2^gsh consecutive hosts, one per lane) through the window [ws, we):
//  1. gather: the group's slabs of the window's buckets are read; runs due in the window go
//     to LDS, the last bucket's later runs move to the spare slab set ks;
//  2. order: counting sort of the due runs by destination lane (LDS atomics + wave scan),
//     then a rank sort inside each destination's segment by (time, src host, src event
//     id) — Shadow's EventQueue order (core/work/event.rs:84-155; keys are unique);
//  3. execute: every lane runs Host::execute (host.rs:762-830) for its host over its
//     segment and local slots, emitting new runs into the calendar / exchange slots;
//  4. the group's minimum kept-event time and next local event time are returned.
// at_end(kmin, next) runs once the group's cross-workgroup data (calendar records, slab
// fills, minima) is issued and before the host records are written back: the round's
// arrival goes there, so its wait covers only what other workgroups read.
// kXb (k_rounds_x): the group's inbox bins (the runs other shards sent it last round) are read in
// the round trip of its first gather and taken into the calendar (see take_bins).
template <bool kTrace, uint32_t kApp, bool kBig, bool kXb = false, bool kDiag = true, typename AtEnd, class SV>
__device__ __forceinline__ void exec_group(const SV& S, uint32_t g, uint64_t ws, uint64_t we, uint32_t ks,
                           const ExecLDS& X, uint64_t* kmin_out, uint64_t* next_out,
                           AtEnd&& at_end) {
  SGN_GLB Ctrl* C = SK(ctrl);
  // per-wave diagnostics (SGN_STAMPS): compiled out of the kernels launched without them
  SGN_GLB uint64_t* const stamps = kDiag ? SK(stamps) : nullptr;
  EvRec* lev = X.lev;
  uint16_t* lb = X.lb;
  uint16_t* lc = X.lc;
  uint32_t* lcnt = X.lcnt;
  uint32_t* lcur = X.lcur;
  LaneLDS<kApp>* lslot = (LaneLDS<kApp>*)X.lslot;
  uint16_t* lbs = X.lbs;
  const uint32_t lane = threadIdx.x;
  const uint32_t gsz = 1u << SK(gsh);
  const uint32_t h = (g << SK(gsh)) + lane;  // local host index
  const bool valid = lane < gsz && h < SK(nH);
  const uint32_t bs = bucket_of(S, ws), be = bucket_of(S, we - 1);
  const uint32_t nbk = ((be + SK(NB) - bs) & (SK(NB) - 1)) + 1;  // buckets overlapping the window
  const uint32_t gbase = SK(lo) + (g << SK(gsh));  // HostId of lane 0
  const uint64_t clk0 = stamps ? __builtin_amdgcn_s_memtime() : 0;
#ifdef SGN_DIAG
  if (stamps && lane < 32) stamps[SGN_STAMP_WORDS * (size_t)g + 48 + lane] = 0;
  __syncthreads();
#endif
  const uint64_t rt0 = stamps ? __builtin_amdgcn_s_memrealtime() : 0;
  const size_t ik = (size_t)ks * SK(G) + g;
  SGN_GLB EvRec* pk = SK(pool) + ik * SK(CAP);

  uint64_t lmin = INVALID;
  uint32_t np = NO_HOST;  // PERIODIC: the next datagram's peer (store() of the host's last round)
  if (valid) {
    lmin = SK(nextloc)[h];
    if (kApp == SGN_TRAFFIC_PERIODIC) np = SK(npeer)[h];
  }
  Outbox<kApp>* ob = static_cast<Outbox<kApp>*>(X.ob);
  if (lane == 0) {
    ob->n = 0;
    ob->xmin = INVALID;
    ob->hz = SIM_START + (SK(bw_div).div(ws - SIM_START) + SK(NB)) * SK(BW);
  }
  __syncthreads();
  HostExec<kTrace, kApp, SV> ex(S, h, we, be, ks, lslot + lane, lbs, ob, kBig ? X.big : nullptr);
  bool loaded = false;
  uint32_t N_all = 0, sorted = 0;
  uint64_t kmin = INVALID;

  uint64_t t_gather = 0, t_exec = 0;
#ifdef SGN_DIAG
  uint64_t w_load = 0, w_run = 0;
#endif
  // a big slab's passes run with the lanes' host state parked in memory: store() (its round
  // counters here), then the registers are dead until the lanes that had state reload it
  uint32_t pk_runs = 0, pk_loss = 0, pk_lev = 0, n_pieces = 0;
  uint64_t pk_bytes = 0;
  auto park = [&]() {
    if (loaded) {
      ex.store(lmin, np);
      lmin = ex.next_local_time();  // (what memory holds now)
      if (kApp == SGN_TRAFFIC_PERIODIC) np = ex.next_peer();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (its write-through stores are asm)
      pk_runs += ex.c_runs;
      pk_loss += ex.c_loss;
      pk_lev += ex.c_localev;
      pk_bytes += ex.c_bytes;
    }
    ex.kill();
  };
  // the last bucket's later runs (keep: this lane's r) move to the spare slab set: through the
  // outbox (placed with the sends after the event loop), or at once when it is full
  auto keep_runs = [&](const EvRec& r, bool keep) {
    const uint64_t km = __ballot(keep);
    if (km) {
      uint32_t k = 0;
      if (lane == 0) k = atomicAdd(&ob->n, (uint32_t)__popcll(km));
      k = __shfl(k, 0, 64) + lanes_below(km);
      if (keep) {
        kmin = r.time < kmin ? r.time : kmin;
        if (k < kObox<kApp>) {
          ob->rec[k] = r;
          ob->idx[k] = (uint32_t)ik;
        } else {
          const uint32_t base = atomicAdd(&SK(slab_n)[ik], 1u);
          if (base < SK(CAP))
            st_dev_rec(pk + base, r);
          else
            place_overflow(S, ob, (uint32_t)ik, base, r);
        }
      }
    }
  };
  // Append the runs of one slab (fill n, its first GATHER_SPEC records already in r0) that
  // are due to lev[N..]; in the window's last bucket the runs at >= we move to the spare slab.
  auto gather_slab = [&](SGN_GLB const EvRec* pb, const EvRec& r0, uint32_t n, bool last, uint32_t& N) {
    for (uint32_t j0 = 0; j0 < n; j0 += 64) {
      const uint32_t j = j0 + lane;
      EvRec r = r0;
      if ((j0 > 0 || lane >= SK(gspec)) && j < n) r = ld_dev_rec(pb + j);
      const bool due = j < n && (!last || r.time < we);
      const bool keep = j < n && !due;
      const uint64_t dm = __ballot(due);
      if (due) lev[N + lanes_below(dm)] = r;
      N += (uint32_t)__popcll(dm);
      keep_runs(r, keep);
    }
  };
  // ---- a big slab (more runs than CAP: its extension, and multi-shard runs k_import spilled) ----
  // every pass reads the slab's runs from memory: the pool part, the extension, and (only when
  // the fill exceeds both) the spill area's entries tagged with this slab (f: per 64-run batch,
  // every lane; ok = the lane holds one of the slab's runs, si = its spill-area index or ~0)
  auto big_scan = [&](size_t ib, SGN_GLB const EvRec* pb, uint32_t nraw, auto&& f) {
    const uint32_t np = min(nraw, SK(CAP));
    for (uint32_t j0 = 0; j0 < np; j0 += 64) {
      const uint32_t j = j0 + lane;
      EvRec r{};
      if (j < np) r = ld_dev_rec(pb + j);
      f(r, j < np, ~0ULL);
    }
    const uint64_t x = SK(ext) ? SK(ext)[ib] : 0ULL;
    const uint32_t ecap = (uint32_t)(x >> 40), ne = min(nraw - np, ecap);
    SGN_GLB const EvRec* pe = SK(ext_pool) + (x & EXT_OFF_MASK);
    for (uint32_t j0 = 0; j0 < ne; j0 += 64) {
      const uint32_t j = j0 + lane;
      EvRec r{};
      if (j < ne) r = ld_dev_rec(pe + j);
      f(r, j < ne, ~0ULL);
    }
    if (nraw - np > ecap) {
      const uint64_t ns = min(X.big->spill_imp, SK(spill_cap));
      for (uint64_t i0 = 0; i0 < ns; i0 += 64) {
        const uint64_t i = i0 + lane;
        const bool mine = i < ns && ld_dev(&SK(spill_idx)[i]) == (uint32_t)ib;
        EvRec r{};
        if (mine) r = ld_dev_rec(SK(spill) + i);
        f(r, mine, i);
      }
    }
  };
  // big_scan over the key fields only (the radix select's passes)
  auto big_scan_keys = [&](size_t ib, SGN_GLB const EvRec* pb, uint32_t nraw, auto&& f) {
    const uint32_t np = min(nraw, SK(CAP));
    for (uint32_t j0 = 0; j0 < np; j0 += 64) {
      const uint32_t j = j0 + lane;
      uint64_t t = 0, e = 0;
      uint32_t src = 0;
      if (j < np) ld_dev_key(pb + j, t, e, src);
      f(t, e, src, j < np);
    }
    const uint64_t x = SK(ext) ? SK(ext)[ib] : 0ULL;
    const uint32_t ecap = (uint32_t)(x >> 40), ne = min(nraw - np, ecap);
    SGN_GLB const EvRec* pe = SK(ext_pool) + (x & EXT_OFF_MASK);
    for (uint32_t j0 = 0; j0 < ne; j0 += 64) {
      const uint32_t j = j0 + lane;
      uint64_t t = 0, e = 0;
      uint32_t src = 0;
      if (j < ne) ld_dev_key(pe + j, t, e, src);
      f(t, e, src, j < ne);
    }
    if (nraw - np > ecap) {
      const uint64_t ns = min(X.big->spill_imp, SK(spill_cap));
      for (uint64_t i0 = 0; i0 < ns; i0 += 64) {
        const uint64_t i = i0 + lane;
        const bool mine = i < ns && ld_dev(&SK(spill_idx)[i]) == (uint32_t)ib;
        uint64_t t = 0, e = 0;
        uint32_t src = 0;
        if (mine) ld_dev_key(SK(spill) + i, t, e, src);
        f(t, e, src, mine);
      }
    }
  };
  // first pass: the later runs of the window's last bucket move to the spare slab set; the due
  // runs' count and time range go to the piece state
  auto big_prepare = [&](size_t ib, uint32_t nraw, bool last) {
    SGN_GLB const EvRec* pb = SK(pool) + ib * SK(CAP);
    uint64_t tmin = INVALID, tmax = 0;
    uint32_t nd = 0;
    big_scan(ib, pb, nraw, [&](const EvRec& r, bool ok, uint64_t) {
      const bool due = ok && (!last || r.time < we);
      if (due) {
        tmin = r.time < tmin ? r.time : tmin;
        tmax = r.time > tmax ? r.time : tmax;
      }
      nd += (uint32_t)__popcll(__ballot(due));
      keep_runs(r, ok && !due);
    });
    tmin = wave_min_u64(tmin);
    tmax = wave_max_u64(tmax);
    if (lane == 0) {
      X.big->tmin = tmin;
      X.big->range = nd ? tmax - tmin : 0;
      X.big->ndue = nd;
      X.big->done = 0;
      X.big->have_prev = 0;
      X.big->ib = ib;
      X.big->nraw = nraw;
      X.big->pad = last ? 1u : 0u;  // (the window's last bucket)
    }
    __syncthreads();
  };
  // The next piece into lev[0, N): the due runs with keys above the last piece's bound, up to CAP
  // of them in key order. Its bound is found by a radix select over the 160-bit key (8-bit
  // digits from the top, one pass and an LDS histogram per digit): the largest prefix range
  // holding at most CAP of the remaining keys, taken at the first digit where it holds at least
  // half of what is still wanted. Returns true for the last piece; else *bound_t = the bound's
  // time part: the piece's runs are at or before it, every later run at or after it.
  auto big_piece = [&](uint32_t& N) -> bool {
    BigLDS& B = *X.big;
    const size_t ib = uni64(B.ib);
    const uint32_t nraw = uni32(B.nraw);
    const bool last = uni32(B.pad) != 0;
    SGN_GLB const EvRec* pb = SK(pool) + ib * SK(CAP);
    const uint64_t tmin = uni64(B.tmin);
    const bool have = uni32(B.have_prev) != 0;
    const BigKey kp = {uni64(B.kp[0]), uni64(B.kp[1]), uni64(B.kp[2])};
    const bool fin = uni32(B.ndue - B.done) <= SK(CAP);
    auto in_s = [&](const EvRec& r, bool ok, BigKey& k) {
      k = big_key(r, tmin);
      return ok && (!last || r.time < we) && (!have || bk_less(kp, k));
    };
    BigKey kt = {~0ULL, ~0ULL, ~0ULL};
    if (!fin) {
      uint32_t* hist = (uint32_t*)lev;  // (lev is free until the piece is loaded)
      const uint64_t range = uni64(B.range);
      uint32_t p = range ? ((uint32_t)__builtin_clzll(range) & ~7u) : 64u;  // first digit that varies
      BigKey P = {0, 0, 0};
      uint32_t acc = 0;
      while (true) {
        for (uint32_t i = lane; i < 256; i += 64) hist[i] = 0;
        __syncthreads();
        const BigKey pm = bk_mask(p);
        big_scan_keys(ib, pb, nraw, [&](uint64_t t, uint64_t e, uint32_t src, bool ok) {
          const BigKey k = {t - tmin, ((uint64_t)src << 32) | (e >> 32), e << 32};
          if (ok && (!last || t < we) && (!have || bk_less(kp, k)) && bk_prefix_eq(k, P, pm))
            atomicAdd(&hist[bk_digit(k, p)], 1u);
        });
        __syncthreads();
        const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const uint32_t ls = h0 + h1 + h2 + h3;
        uint32_t incl = ls;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t y = __shfl_up(incl, off, 64);
          if ((int)lane >= off) incl += y;
        }
        const uint32_t want = SK(CAP) - acc;
        const uint32_t c0 = incl - ls + h0, c1 = c0 + h1, c2 = c1 + h2, c3 = c2 + h3;
        // this lane's largest bin whose cumulative count is <= want (-1: none)
        int dl = -1;
        uint32_t cl = 0;
        if (c0 <= want) { dl = 4 * (int)lane; cl = c0; }
        if (c1 <= want) { dl = 4 * (int)lane + 1; cl = c1; }
        if (c2 <= want) { dl = 4 * (int)lane + 2; cl = c2; }
        if (c3 <= want) { dl = 4 * (int)lane + 3; cl = c3; }
        int df = dl;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const int o = __shfl_xor(df, off, 64);
          df = o > df ? o : df;
        }
        df = (int)uni32((uint32_t)df);
        const uint32_t cf = uni32(df >= 0 ? __shfl(cl, df >> 2, 64) : 0u);
        __syncthreads();  // every lane has read the histogram
        if (df >= 0 && (2 * cf >= want || p + 8 >= 160 || df == 255)) {
          kt = bk_fill(bk_set_digit(P, p, (uint32_t)df), p + 8);
          break;
        }
        // descend into the bin that crosses: every key of the bins before it is in the piece
        acc += cf;
        P = bk_set_digit(P, p, (uint32_t)(df + 1));
        p += 8;
      }
    }
    N = 0;
    big_scan(ib, pb, nraw, [&](const EvRec& r, bool ok, uint64_t) {
      BigKey k;
      const bool sel = in_s(r, ok, k) && !bk_less(kt, k);
      const uint64_t m = __ballot(sel);
      if (sel && N + lanes_below(m) < SK(CAP)) lev[N + lanes_below(m)] = r;
      N += (uint32_t)__popcll(m);
    });
    bool bad = false;
    if (N > SK(CAP) || (!fin && N == 0)) {  // (cannot happen: the select bounds every piece by
      // CAP and takes at least one run) never silent, and the pieces end
      if (lane == 0 && (atomicOr(&C->overflow, OVF_SEG) & OVF_SEG) == 0) C->overflow_info = gbase;
      N = min(N, SK(CAP));
      bad = true;
    }
    if (fin || bad) {
      // runs taken from the spill area are tagged done (the re-layout must not file them again)
      big_scan(ib, pb, nraw, [&](const EvRec&, bool ok, uint64_t si) {
        if (ok && si != ~0ULL) st_dev(&SK(spill_idx)[si], SPILL_DEAD);
      });
    }
    __syncthreads();
    if (lane == 0) {
      B.done = bad ? B.ndue : B.done + N;
      B.have_prev = 1;
      B.kp[0] = kt.hi;
      B.kp[1] = kt.mid;
      B.kp[2] = kt.lo;
      // the host's runs of this piece end at the bound's time T: every later run is at or after it
      B.tail = fin || bad ? INVALID : (kt.hi > EMU_MAX - tmin ? EMU_MAX : tmin + kt.hi);
      B.flush = fin || bad ? 1u : 0u;
    }
    __syncthreads();
    return fin || bad;
  };
  auto slab_done = [&](size_t ib, uint32_t n) {
    if (lane == 0) {
      st_dev(&SK(slab_n)[ib], 0u);  // consumed (or moved); nobody appends to it this round
      if (n && X.wacc)
        wacc_max(&X.wacc[W_MAXFILL], n);
      else if (n)
        __hip_atomic_fetch_max(&SK(w_cnt)[W_MAXFILL * SK(G) + g], (uint64_t)n, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);  // high-water mark, this wave's slot
    }
  };
  // ---- k_rounds_x: the runs other shards sent this group last round (its inbox bins) ----
  // A run for a bucket of this window goes into its slab before the gathers read it (returns
  // true: the first gather's loads are redone); a later one goes through the outbox into its
  // bucket's slab like a send, with the bucket's minimum (its first bucket is not read while
  // it is the window's: k_import's rule). bp, r: this lane's entry of the first pass (r loaded);
  // a sender whose last entry of a pass was full is read on. Taken entries are zeroed (pc 0 is
  // an empty entry) for the bin's next use two rounds later; the runs were counted in this
  // shard's occupancy at the round edge (XH_TOT).
  auto take_bins = [&](SGN_GLB EvRec* bp, EvRec r, uint32_t q, uint32_t e, bool on) -> bool {
    const uint32_t E = 1u << (SK(n_ranks) <= 2 ? 5u : SK(n_ranks) <= 4 ? 4u : 3u);
    bool slow = false;
    bool more = on;
    for (uint32_t e0 = 0;;) {
      const bool ok = more && r.pc != 0;
      if (ok) {
        SGN_GLB uint64_t* pw = (SGN_GLB uint64_t*)(bp + e0) + 3;
        if (SK(xsys)) st_sys(pw, 0ull); else st_dev(pw, (uint64_t)0);
        if (r.time >= ob->hz) {
          if ((atomicOr(&C->overflow, OVF_HORIZON) & OVF_HORIZON) == 0) C->overflow_info = r.dst;
        } else {
          const uint32_t b = bucket_of(S, r.time);
          const size_t idx = (size_t)lbs[b] * SK(G) + g;
          bool direct = ((b - bs) & (SK(NB) - 1)) < nbk;
          slow |= direct;
          if (!direct) {
            // (the workgroup's LDS table of bucket minima where the kernel has one, as for sends:
            // config D's ~100 k imports a round per shard would queue on a few bucket words)
            if (kAggBmin<kApp> && SK(agg_bmin))
              atomicMin(&ob->bmin[b], (uint32_t)(r.time - ob->bbase));
            else
              min_nr(&SK(bucket_min)[b], r.time);
            const uint32_t k = atomicAdd(&ob->n, 1u);  // LDS
            if (k < kObox<kApp>) {
              ob->rec[k] = r;
              ob->idx[k] = (uint32_t)idx;
            } else {
              direct = true;
            }
          }
          if (direct) {
            const uint32_t pos = atomicAdd(&SK(slab_n)[idx], 1u);
            if (pos < SK(CAP))
              st_dev_rec(SK(pool) + idx * SK(CAP) + pos, r);
            else
              place_overflow(S, ob, (uint32_t)idx, pos, r);
          }
        }
      }
      const uint64_t m = __ballot(ok && e == E - 1);
      e0 += E;
      if (!m || e0 >= SK(xbk)) break;
      more = on && ((m >> (q * E + E - 1)) & 1ull) && e0 + e < SK(xbk);
      r = EvRec{};
      if (more) r = SK(xsys) ? ld_sys_rec(bp + e0) : ld_dev_rec(bp + e0);
    }
    return __ballot(slow) != 0;
  };
  for (uint32_t bi = 0; bi < nbk; bi++) {
    const uint64_t c0 = stamps ? __builtin_amdgcn_s_memtime() : 0;
    const uint32_t b = (bs + bi) & (SK(NB) - 1);
    bool last = bi == nbk - 1;
    uint64_t sub_end = last ? we : SIM_START + (SK(bw_div).div(ws - SIM_START) + bi + 1) * SK(BW);
    // ---- 1. gather the group's runs of bucket b that are due (all but the last bucket's
    //      runs at >= we, which join this round's new runs for it in the spare slab) ----
    const size_t ib = (size_t)uni32(SK(NB) <= LDS_BSLAB ? lbs[b] : ld_dev(&SK(bucket_slab)[b])) * SK(G) + g;
    // the slab's fill and its first GATHER_SPEC records in ONE round trip: the records are
    // loaded before the fill is known (S.gspec <= CAP; slots past the fill are ignored) — nothing
    // appends to a bucket's slab while its window runs (new runs for the window's last
    // bucket go to the spare slab set). Only GATHER_SPEC lanes load speculatively: a slab
    // holds ~4 runs on average, and loading all 64 slots pulled 2 KB of cold HBM lines per
    // slab (PMC fetch 58 -> 342 MB per launch); fuller slabs load the rest below.
    // A window that straddles one bucket boundary (the common case) loads both slabs in
    // that round trip and, when both fit one 64-run pass, runs as one sub-window: one sort,
    // one event-loop pass (the runs of the second bucket are all later than the first's).
    // (compiled into the PERIODIC kernel only: same-box A/B, config B +25 %, while C's TGEN
    // kernel — whose rounds are set by its servers' trains — measured 0.7 % slower with it)
    const bool pair = kApp == SGN_TRAFFIC_PERIODIC && bi == 0 && nbk == 2;
    SGN_GLB const EvRec* pb = SK(pool) + ib * SK(CAP);
    EvRec r0{}, r1{};
    size_t ib1 = 0;
    SGN_GLB const EvRec* pb1 = nullptr;
    if (pair) {
      ib1 = (size_t)(SK(NB) <= LDS_BSLAB ? lbs[(b + 1) & (SK(NB) - 1)] : ld_dev(&SK(bucket_slab)[(b + 1) & (SK(NB) - 1)])) * SK(G) + g;
      pb1 = SK(pool) + ib1 * SK(CAP);
    }
    // k_rounds_x: the first pass over the group's inbox bins, in the same round trip (lane =
    // sender x E + entry, E entries per sender and pass)
    const bool bins = kXb && bi == 0 && SK(xin_bins) != nullptr;
    const uint32_t bsh = SK(n_ranks) <= 2 ? 5u : SK(n_ranks) <= 4 ? 4u : 3u;
    const uint32_t bq = lane >> bsh, be_ = lane & ((1u << bsh) - 1);
    const bool bon = bins && bq < SK(n_ranks) && bq != SK(rank) && be_ < SK(xbk);
    SGN_GLB EvRec* bp = bon ? SK(xin_bins) + (((size_t)(ob->xbuf ^ 1u) * SK(n_ranks) + bq) * SK(G) + g) * SK(xbk) + be_ : nullptr;
    EvRec br{};
    if (bon) br = SK(xsys) ? ld_sys_rec(bp) : ld_dev_rec(bp);
    if (lane < SK(gspec)) {
      r0 = ld_dev_rec(pb + lane);
      if (pair) r1 = ld_dev_rec(pb1 + lane);
    }
    uint32_t nraw_v = ld_dev(&SK(slab_n)[ib]);
    uint32_t n1raw_v = pair ? ld_dev(&SK(slab_n)[ib1]) : 0u;
    // PERIODIC traffic (configs B and D: most executed hosts have their app timer due): the
    // host record of a lane whose local event is due in the window loads in the same round trip
    // as the gather, and the app's next route is prefetched behind the sort
    const bool early = kApp == SGN_TRAFFIC_PERIODIC && bi == 0 && valid && lmin < we;
    if (early) {
      ex.load();
      ex.prefetch_peer(np);
      loaded = true;
    }
    if (bins && take_bins(bp, br, bq, be_, bon)) {
      // runs due in this window's buckets went into their slabs ahead of the gathers: the
      // first bucket's (and its pair's) loads again (spill-area entries included, big path)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (kBig && lane == 0) X.big->spill_imp = ld_dev(&C->spill_n);
      if (lane < SK(gspec)) {
        r0 = ld_dev_rec(pb + lane);
        if (pair) r1 = ld_dev_rec(pb1 + lane);
      }
      nraw_v = ld_dev(&SK(slab_n)[ib]);
      n1raw_v = pair ? ld_dev(&SK(slab_n)[ib1]) : 0u;
    }
    // (scalar copies after the host record's loads are issued: a readfirstlane waits for its load)
    const uint32_t nraw = uni32(nraw_v), n1raw = uni32(n1raw_v);
    // more runs than the LDS holds: the big-slab path (ordered and executed in pieces). The
    // kernels without it (kBig false: no slab extension exists, so a run past CAP went to the
    // spill area and the round edge held for the re-layout before the slab could be due) never
    // see one; if one did, it is an overflow, not a silent truncation.
    const bool big = kBig && nraw > SK(CAP);
    if (!kBig && nraw > SK(CAP) && lane == 0) atomicOr((unsigned int*)&C->overflow, OVF_BUCKET);
    const uint32_t n = min(nraw, SK(CAP));
    uint32_t N = 0;
    if (!big) {
      lcnt[lane] = 0;
      gather_slab(pb, r0, n, last, N);
      slab_done(ib, n);
      // (merged only while the pair fits one 64-run pass: config D's slabs hold ~64 runs each,
      // and merging them made its longer per-lane rank sorts cost more than the pass saved)
      if (pair && n + n1raw <= min(SK(CAP), 64u)) {
        gather_slab(pb1, r1, n1raw, true, N);
        slab_done(ib1, n1raw);
        bi = 1;  // the second bucket is done: this is the window's last sub-window
        last = true;
        sub_end = we;
      }
      if (kBig && lane == 0) {  // one pass: no later packet run, digests close with it
        X.big->tail = INVALID;
        X.big->flush = 1;
      }
    } else {
      park();
      big_prepare(ib, nraw, last);
      slab_done(ib, nraw);
    }
    for (bool first = true;; first = false) {  // pieces (one unless big)
      uint64_t until = sub_end;
      bool fin = true;
      if (big) {
        if (!first) park();
        lcnt[lane] = 0;
        fin = big_piece(N);
        if (!fin) until = uni64(X.big->tail);
        n_pieces++;
        if (loaded) ex.load(false);
      }
    N_all += N;
    __syncthreads();
    // ---- 2. order: counting sort by destination lane, then rank sort by Shadow's key ----
    for (uint32_t j = lane; j < N; j += 64) atomicAdd(&lcnt[lev[j].dst - gbase], 1u);
    __syncthreads();
    const uint32_t cnt = lcnt[lane];
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(incl, off, 64);
      if ((int)lane >= off) incl += y;
    }
    const uint32_t start = incl - cnt;
    lcur[lane] = start;
    __syncthreads();
    for (uint32_t j = lane; j < N; j += 64) {
      const uint32_t pos = atomicAdd(&lcur[lev[j].dst - gbase], 1u);
      lb[pos] = (uint16_t)j;
    }
    __syncthreads();
    for (uint32_t q = lane; q < N; q += 64) {
      const uint32_t idx = lb[q];
      const EvRec& r = lev[idx];
      const uint32_t d = r.dst - gbase;
      const uint32_t k = lcnt[d], a = lcur[d] - k;  // (placement left lcur at the segment's end)
      uint32_t rank = 0;
      for (uint32_t t = a; k > 1 && t < a + k; t++) {
        const EvRec& o = lev[lb[t]];
        rank += (o.time < r.time ||
                 (o.time == r.time && (o.src < r.src || (o.src == r.src && o.eid < r.eid))))
                    ? 1u : 0u;
      }
      lc[a + rank] = (uint16_t)idx;
    }
    sorted += cnt > 1 ? 1u : 0u;
    if (early && !big) ex.prefetch_route();
    __syncthreads();
    // ---- 3. execute the sub-window [.., sub_end) (a big slab's piece: up to its bound) ----
    const uint64_t c1 = stamps ? __builtin_amdgcn_s_memtime() : 0;
#ifdef SGN_DIAG
    // wave-level phase times (the loads are drained inside the load phase here)
    const bool go = valid && (cnt > 0 || (loaded ? ex.next_local_time() : lmin) < until);
    const uint64_t ta = __builtin_amdgcn_s_memtime();
    if (go && !loaded) {
      ex.load();
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      loaded = true;
    }
    const uint64_t tb = __builtin_amdgcn_s_memtime();
    if (go) ex.run(lev, lc, start, start + cnt, until);
    const uint64_t tc = __builtin_amdgcn_s_memtime();
    w_load += tb - ta;
    w_run += tc - tb;
#else
    const bool go = valid && (cnt > 0 || (loaded ? ex.next_local_time() : lmin) < until);
    if (go) {
      if (!loaded) {
        ex.load();
        loaded = true;
      }
      ex.run(lev, lc, start, start + cnt, until);
    }
#endif
    // a big slab's host that ran in an earlier piece closes its digest runs with the last one
    if (big && fin && !go && loaded) ex.flush_digests();
    __syncthreads();  // LDS is reused by the next piece or bucket
    if (stamps) {
      const uint64_t c2 = __builtin_amdgcn_s_memtime();
      t_gather += c1 - c0;
      t_exec += c2 - c1;
    }
      if (fin) break;
    }
  }

  // the outbox's records into their slabs, all lanes at once (the arrival's vmcnt(0)
  // completes them before the round edge)
  {
    const uint32_t no = min(ob->n, kObox<kApp>);
    if constexpr (kApp == SGN_TRAFFIC_PERIODIC && !kBig && !kPairOff) {  // (not with the big-slab path: registers)
      // two lanes per record, each storing one 16-byte half: the record is one 32-byte write
      // (a lane's two 16-byte write-through stores of one record are two; config D writes a
      // record per host-round, MI355X_MICROARCH.md: write-through stores and their granules)
      for (uint32_t i0 = 0; i0 < no; i0 += 32) {
        const uint32_t i = i0 + (lane >> 1), half = lane & 1;
        const bool has = i < no;
        uint32_t idx = 0, pos = 0;
        if (has) idx = ob->idx[i];
        if (has && !half) pos = atomicAdd(&SK(slab_n)[idx], 1u);
        pos = __shfl(pos, (int)(lane & ~1u), 64);
        if (has) {
          const EvRec& r = ob->rec[i];
          if (pos < SK(CAP)) {
            SGN_GLB char* q = (SGN_GLB char*)(SK(pool) + (size_t)idx * SK(CAP) + pos) + 16 * half;
            if (half)
              st_wt16(q, (uint64_t)r.src | ((uint64_t)r.dst << 32), (uint64_t)r.pc | ((uint64_t)r.tag << 32));
            else
              st_wt16(q, r.time, r.eid);
          } else if (!half) {
            place_overflow(S, ob, idx, pos, r);
          }
        }
      }
    } else {
      for (uint32_t i = lane; i < no; i += 64) {
        const uint32_t idx = ob->idx[i];
        const uint32_t pos = atomicAdd(&SK(slab_n)[idx], 1u);
        if (pos < SK(CAP))
          st_dev_rec(SK(pool) + (size_t)idx * SK(CAP) + pos, ob->rec[i]);
        else
          place_overflow(S, ob, idx, pos, ob->rec[i]);
      }
    }
  }
  uint64_t my_min = lmin;  // a host with nothing due sleeps through the window
  if (loaded) my_min = ex.next_local_time();
  kmin = wave_min_u64(kmin);
  uint64_t m = wave_min_u64(my_min);
  m = ob->xmin < m ? ob->xmin : m;  // runs exported to other shards are pending events too
  *kmin_out = kmin;
  *next_out = m;
  // the calendar's occupancy change: runs this group appended minus the due runs it took out
  // (the last bucket's later runs moved to the spare slab set count out and in)
  const uint64_t occd = (uint64_t)wave_sum_u32((loaded ? ex.c_runs : 0u) + pk_runs) - (uint64_t)N_all;
  at_end(kmin, m, occd);
  uint32_t n_ev = 0;
#ifdef SGN_DIAG
  const uint64_t td = __builtin_amdgcn_s_memtime();
#endif
  if (loaded) {
    ex.store(lmin, np);
    n_ev = ex.c_popped + ex.c_sent + ex.c_loss + ex.c_deliv + ex.c_localev;
  }
#ifdef SGN_DIAG
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  const uint64_t w_store = __builtin_amdgcn_s_memtime() - td;
#endif
  if (stamps) {
    // per-wave diagnostics: shader cycles, total and max events over the wave's lanes
    const uint64_t clk1 = __builtin_amdgcn_s_memtime();
    uint32_t sum = n_ev, mx = n_ev;
    for (int off = 32; off > 0; off >>= 1) {
      sum += __shfl_xor(sum, off, 64);
      const uint32_t o = __shfl_xor(mx, off, 64);
      mx = o > mx ? o : mx;
    }
    const uint32_t busy = __popcll(__ballot(n_ev > 0));
    SGN_GLB uint64_t* st = stamps + SGN_STAMP_WORDS * (size_t)g;
    if (lane == 0) {
      st[0] = clk1 - clk0;
      st[1] = sum;
      st[2] = mx;
      st[3] = busy;
      st[4] = N_all;
      st[5] = t_gather;
      st[6] = t_exec;
      st[7] = rt0;  // 100 MHz constant clock: wave start / end across the chip
      st[8] = ob->n;  // records sent to this shard's calendar (past the outbox: placed at once)
      st[30] = __builtin_amdgcn_s_memrealtime();
    }
#ifdef SGN_DIAG
    for (int i = 0; i < DGT_N; i++) {
      const uint32_t v = loaded ? ex.dgt[i] : 0u;
      const uint32_t vs = wave_sum_u32(v);  // the wave's time in section i
      if (lane == 0) st[i < 16 ? 80 + i : 10 + (i - 16)] = vs;  // (sections past 15: words 10..)
    }
    if (lane == 0) {
      st[32] = w_load;
      st[33] = w_run;
      st[34] = w_store;
    }
    for (int i = 0; i < 5; i++) {
      const uint32_t v = wave_sum_u32(loaded ? ex.wk[i] : 0u);
      if (lane == 0) st[35 + i] = v;
    }
#endif
  }
  // ---- 4. hosts that ran (roofline accounting): per-wave counters, no-return adds ----
  const uint64_t ex_mask = __ballot(loaded);
  const uint32_t n_sorted = wave_sum_u32(sorted);
  const uint32_t w_loss = wave_sum_u32((loaded ? ex.c_loss : 0u) + pk_loss);
  const uint32_t w_lev = wave_sum_u32((loaded ? ex.c_localev : 0u) + pk_lev);
  uint64_t w_bytes = (loaded ? ex.c_bytes : 0) + pk_bytes;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) w_bytes += shfl_xor64(w_bytes, off);
  if (lane == 0 && X.wacc) {  // (persistent launches: per-round statistics stay in LDS; at config
    // B these ~8 small atomics per group and round were ~70 % of the round kernel's PMC writes;
    // no-return LDS atomics: this runs after the round's arrival, on the next round's path)
    wacc_add(&X.wacc[W_EXEC], (uint64_t)__popcll(ex_mask));
    wacc_add(&X.wacc[W_RUNS], N_all);
    wacc_add(&X.wacc[W_SORTED], n_sorted);
    wacc_add(&X.wacc[W_LOSS], w_loss);
    wacc_add(&X.wacc[W_LOCAL_EV], w_lev);
    wacc_add(&X.wacc[W_BYTES], w_bytes);
    if (n_pieces) wacc_add(&X.wacc[W_BIG], n_pieces);
  } else if (lane == 0) {
    const size_t G = SK(G);
    if (ex_mask) cnt_add(&SK(w_cnt)[W_EXEC * G + g], (uint64_t)__popcll(ex_mask));
    if (N_all) cnt_add(&SK(w_cnt)[W_RUNS * G + g], N_all);
    if (n_sorted) cnt_add(&SK(w_cnt)[W_SORTED * G + g], n_sorted);
    if (w_loss) cnt_add(&SK(w_cnt)[W_LOSS * G + g], w_loss);
    if (w_lev) cnt_add(&SK(w_cnt)[W_LOCAL_EV * G + g], w_lev);
    if (w_bytes) cnt_add(&SK(w_cnt)[W_BYTES * G + g], w_bytes);
    if (n_pieces) cnt_add(&SK(w_cnt)[W_BIG * G + g], n_pieces);
  }
}

#define SGN_EXEC_LDS(X)                                                              \
  extern __shared__ __attribute__((aligned(16))) char lds_dyn[];                     \
  __shared__ uint32_t lcnt_[64], lcur_[64];                                         \
  __shared__ LaneLDS<kApp> lslot_[64];                                               \
  __shared__ uint16_t lbs_[LDS_BSLAB];                                               \
  __shared__ Outbox<kApp> ob_;                                                       \
  __shared__ BigLDS big_;                                                            \
  ExecLDS X;                                                                         \
  X.lev = (EvRec*)lds_dyn;                                                           \
  X.lb = (uint16_t*)(X.lev + SK(CAP));                                                 \
  X.lc = X.lb + ((SK(CAP) + 3) & ~3u);                                                 \
  X.bmin = SK(agg_bmin) ? (uint32_t*)(lds_dyn + exec_lds_runs_bytes(SK(CAP))) : nullptr;  \
  X.lcnt = lcnt_;                                                                    \
  X.lcur = lcur_;                                                                    \
  X.lslot = lslot_;                                                                  \
  X.lbs = lbs_;                                                                      \
  X.ob = &ob_;                                                                       \
  X.big = &big_;                                                                     \
  X.wacc = nullptr;                                                                  \
  if (threadIdx.x == 0) {                                                            \
    ob_.bmin = X.bmin;                                                               \
    ob_.xc = nullptr;                                                                \
    big_.spill_imp = ld_dev(&SK(ctrl)->spill_imp);                                     \
  }

// The workgroup's LDS table of bucket minima (S.agg_bmin): its sends of the round fold their
// delivery times there with LDS atomics; before the round's arrival every lane publishes a
// share of the table with one device atomic per touched bucket and resets it. Config D (every
// host sends to a random peer every round) otherwise puts ~1 M device atomics per round on
// the ~50 bucket words of the next 50 ms — a few cache lines — and serialises on them.
// Entries are u32 offsets from the round's window start (a delivery is below the calendar's
// horizon, at most (NB + 1) bucket widths ahead; sim_init enables the table only when that
// fits 32 bits).
template <uint32_t kApp, class SV>
__device__ __forceinline__ void init_bmin(const SV& S, const ExecLDS& X) {
  if (kAggBmin<kApp> && X.bmin)
    for (uint32_t i = threadIdx.x; i <= SK(NB); i += blockDim.x) X.bmin[i] = 0xFFFFFFFFu;
}
template <uint32_t kApp, class SV>
__device__ __forceinline__ void flush_bmin(const SV& S, const ExecLDS& X) {
  if (!kAggBmin<kApp> || !X.bmin) return;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i <= SK(NB); i += blockDim.x) {
    const uint32_t v = X.bmin[i];
    if (v != 0xFFFFFFFFu) {
      min_nr(i == SK(NB) ? X.ob->keepmin : &SK(bucket_min)[i], X.ob->bbase + v);
      X.bmin[i] = 0xFFFFFFFFu;
    }
  }
}

// Arrival of one workgroup at the end of a round: its minima go into its chunk's slots with
// returning device-scope atomics, then it counts itself in (64 workgroups per chunk counter,
// then chunks). Only atomics cross between workgroups (no fences: an agent-scope release
// writes the whole L2 back on gfx950). Returns true (all lanes) for the last arrival.
__device__ bool arrive(const DevSim& S, uint32_t w, uint32_t nw, uint64_t kmin, uint64_t m, uint64_t occd) {
  uint32_t last = 0;
  if (threadIdx.x == 0) {
    const uint32_t ch = w >> 6;
    const uint32_t csz = min(64u, nw - (ch << 6));
    const uint32_t nch = (nw + 63) >> 6;
    if (occd) cnt_add(&SK(fin_occ)[ch], occd);
    if (kmin != INVALID)
      __hip_atomic_fetch_min(&SK(fin_keep)[ch], (unsigned long long)kmin, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    if (m != INVALID)
      __hip_atomic_fetch_min(&SK(fin_next)[ch], (unsigned long long)m, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every store/atomic of the round done
    const uint32_t c = __hip_atomic_fetch_add(&SK(fin_cnt)[ch], 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    if (c == csz - 1) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const uint32_t t = __hip_atomic_fetch_add(&SK(fin_cnt)[nch], 1u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
      last = t == nch - 1 ? 1u : 0u;
    }
  }
  return __shfl(last, 0, 64) != 0;
}

// One round per launch: one workgroup (one wave) per group; single shard: the last arrival
// runs the round edge (finalize_fused), multi-shard: comm.cpp's exchange follows.
// kTrace: the per-packet trace compiled in (traced runs); untraced per-round launches — the
// multi-shard rounds, sgn_round, the persistent kernel's fallback — use the lean twin.
template <bool kTrace, uint32_t kApp>
__global__ __launch_bounds__(64, 2) void k_execute(const DevSim* __restrict__ Sg) {
  // the simulation constants are read from device memory where they are used (a by-value
  // kernel argument would pin ~90 scalar registers for the whole kernel)
  const DevSim& S = *Sg;
  SGN_GLB Ctrl* C = SK(ctrl);
  if (!C->active || C->xspill || C->hold) return;  // a held round waits for the host
  SGN_EXEC_LDS(X)
  const uint64_t ws = C->ws, we = C->we;
  const uint32_t ks = C->keep_slab;
  if (SK(NB) <= LDS_BSLAB)
    for (uint32_t i = threadIdx.x; i < SK(NB); i += 64) X.lbs[i] = (uint16_t)SK(bucket_slab)[i];
  if (threadIdx.x == 0) {
    X.ob->keepmin = &C->keep_min;
    X.ob->bbase = C->ws;
    X.ob->pg_avail = C->pg_avail;
    X.ob->pg_freed = &C->pg_freed;
    X.ob->pg_allocd = &C->rnd_alloc;
    X.ob->spilled = &C->rnd_spill;
    X.ob->xn = SK(xout_n);
    X.ob->xbuf = 2;  // (the RCCL send blocks)
  }
  init_bmin<kApp>(S, X);
  __syncthreads();
  uint64_t kmin, m;
  bool last = false;
  exec_group<kTrace, kApp, true>(S, blockIdx.x, ws, we, ks, X, &kmin, &m, [&](uint64_t k, uint64_t n, uint64_t od) {
    flush_bmin<kApp>(S, X);
    last = arrive(S, blockIdx.x, gridDim.x, k, n, od);
  });
  if (!last) return;
  const uint32_t b1 = bucket_of(S, we - 1);
  // single shard: the round edge; multi-shard: the local part of it (comm.cpp finishes it)
  finalize_fused(S, threadIdx.x, (gridDim.x + 63) >> 6, ws, we, ks,
                 SK(NB) <= LDS_BSLAB ? X.lbs[b1] : ld_dev(&SK(bucket_slab)[b1]), SK(fuse_finalize) ? 0 : 1);
}

// ---- persistent rounds: a decentralized round edge ----
// Per round r every workgroup folds its minima (runs kept in the spare slab, next local
// events) into its chunk's slots of buffer p = r % 3, counts itself in (64 workgroups per
// chunk, then chunks), waits for the whole grid, and then computes the next window ITSELF
// from the same values (Controller::manager_finished_current_round, controller.rs:88-112):
// no workgroup publishes the edge, so the barrier costs one arrival and one observation
// instead of arrival + finalize + publish + wake-up. Shared bookkeeping is done by workgroup
// 0 during the FOLLOWING round (bucket minima of consumed buckets, the swapped bucket's new
// minimum, the global bucket -> slab table) and before the launch ends; buffer (r + 1) % 3 is
// reset by workgroup 0 during round r (its last readers passed barrier r - 1). sim_init sizes
// the calendar so no send of round r + 1 can reach a bucket consumed in round r.
// Strides between chunks (u32 counters, u64 minimum pairs, u64 occupancy sums). TGEN rounds
// (config C: 1563 workgroups in 25 chunks) give every chunk its own 128-B line for each, so
// the ~4.7 k arrival atomics of a round do not queue on a few shared lines: same-box A/B on
// C 3549 -> 3513 us per 100-round launch; with config B at 16 hosts per wave (625 workgroups)
// and D at 8 workgroups per CU (2048), padding plus a poll sleep of 8 is -0.6 % on B and
// -0.3 % on D. Buffers are allocated for the padded layout.
template <uint32_t kApp> struct RbLayout {
  static constexpr bool pad = kApp != SGN_TRAFFIC_EXTERNAL;
  static constexpr uint32_t CS = pad ? 32 : 1, MS = pad ? 16 : 2, OS = pad ? 16 : 1;
  static constexpr uint32_t CB = (RB_CH + 1) * CS;  // u32 per buffer of counters (chunks, then the top)
};

template <uint32_t kApp, class SV>
__device__ __forceinline__ void rb_arrive(const SV& S, uint32_t p, uint32_t w, uint32_t nw, uint64_t kmin,
                                          uint64_t m, uint64_t occd) {
  if (threadIdx.x != 0) return;
  const uint32_t ch = w >> 6;
  const uint32_t csz = min(64u, nw - (ch << 6));
  using Y = RbLayout<kApp>;
  SGN_GLB uint64_t* mn = SK(rb_min) + ((size_t)p * RB_CH + ch) * Y::MS;
  if (kmin != INVALID) min_nr(mn, kmin);
  if (m != INVALID) min_nr(mn + 1, m);
  if (occd) cnt_add(&SK(rb_occ)[((size_t)p * RB_CH + ch) * Y::OS], occd);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this round's stores and atomics done
  SGN_GLB uint32_t* cnt = SK(rb_cnt) + (size_t)p * Y::CB;
  const uint32_t c = __hip_atomic_fetch_add(&cnt[ch * Y::CS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (c == csz - 1) (void)__hip_atomic_fetch_add(&cnt[RB_CH * Y::CS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The next window from buffer p after the barrier (every workgroup, identical results).
struct RbEdge {
  uint64_t ws, we, min_next, nb1;
  uint64_t occd, nalloc, nfree, nspill;  // the round's calendar occupancy change, CoDel pages
                                         // allocated / freed, runs spilled (buffer p: stable)
  uint32_t active;
};
template <uint32_t kApp, class SV>
__device__ __forceinline__ RbEdge rb_edge(const SV& S, uint32_t p, uint32_t nch, uint64_t ws, uint64_t we) {
  using Y = RbLayout<kApp>;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t b0 = bucket_of(S, ws), b1 = bucket_of(S, we - 1);
  // Every load of the edge is issued before any is used: one round trip. (The loop form of the
  // bucket scan — one load per 64 buckets, each waited for before the next — and the counters
  // loaded after it made the edge ~5 dependent round trips; C scans ~151 buckets.) Lanes past
  // a range load a valid word of it and ignore it; the single words are loaded by every lane
  // (one request), so no broadcast follows.
  const uint32_t nc = nch ? nch : 1u;
  SGN_GLB uint64_t* mn = SK(rb_min) + ((size_t)p * RB_CH + min(lane, nc - 1)) * Y::MS;
  uint64_t kk = ld_dev(mn), wn = ld_dev(mn + 1);
  uint64_t od = ld_dev(&SK(rb_occ)[((size_t)p * RB_CH + min(lane, nc - 1)) * Y::OS]);
  const uint64_t km = ld_dev(&SK(rb_keep)[p]), mu = ld_dev(&SK(ctrl)->min_used);
  const uint64_t na = ld_dev(&SK(rb_occ)[3 * RB_CH * RB_OS_MAX + p]), ns = ld_dev(&SK(rb_occ)[3 * RB_CH * RB_OS_MAX + 3 + p]);
  const uint64_t nf = ld_dev(&SK(rb_free)[p]);
  // the buckets to scan: synthetic traffic — every pending event is a delivery, so it lies in
  // [we, we + max_lat) (sends happen inside a window and arrive at most max_lat later,
  // worker.rs:386-390): only the buckets after b1 up to bucket_of(we + max_lat - 1) can hold
  // one (b1: nb1 below; C scans ~151 of its 256 buckets, B and D ~51). CPU-submitted datagrams
  // may be filed further ahead: every bucket the window has not consumed. (The persistent
  // kernels run with NB <= LDS_BSLAB = 256: at most four buckets per lane.)
  const bool ext = SK(tkind) == SGN_TRAFFIC_EXTERNAL;
  const uint32_t span = (b1 - b0) & (SK(NB) - 1);
  const uint32_t nscan = ext ? SK(NB) - 1 - span
                             : (uint32_t)min<uint64_t>(SK(NB) - 1 - span, SK(bw_div).div(SK(max_lat) + SK(BW) - 1) + 1);
  uint64_t m = INVALID;
  if (nscan) {
    uint64_t bm[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
      bm[q] = ld_dev(&SK(bucket_min)[(b1 + 1 + min(lane + 64 * q, nscan - 1)) & (SK(NB) - 1)]);
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
      if (lane + 64 * q < nscan) m = bm[q] < m ? bm[q] : m;
    for (uint32_t k = lane + 256; k < nscan; k += 64) {  // (NB > 256: not on the persistent path)
      const uint64_t v = ld_dev(&SK(bucket_min)[(b1 + 1 + k) & (SK(NB) - 1)]);
      m = v < m ? v : m;
    }
  }
  if (lane >= nch) {
    kk = INVALID;
    wn = INVALID;
    od = 0;
  }
  kk = wave_min_u64(kk);
  wn = wave_min_u64(wn);
  m = wave_min_u64(m);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) od += shfl_xor64(od, off);
  RbEdge e;
  e.occd = od;
  e.nalloc = na;
  e.nfree = nf;
  e.nspill = ns;
  e.nb1 = km < kk ? km : kk;  // the spare slab set becomes bucket b1
  m = e.nb1 < m ? e.nb1 : m;
  m = wn < m ? wn : m;
  e.min_next = m == INVALID ? EMU_MAX : m;  // unwrap_or(MAX)
  // window_end's rule (sgn_internal.h), written out: through the function the compiler works it
  // out on the scalar unit and waits for mu in the middle of the loads above — a second round
  // trip per round (config C: +0.45 % per step, same-box ABBA)
  uint64_t ra = (SK(dynamic) && mu != INVALID) ? mu : SK(min_possible);
  ra = ra > SK(runahead_cfg) ? ra : SK(runahead_cfg);
  uint64_t ne = e.min_next + ra;
  if (ne < e.min_next || ne > EMU_MAX) ne = EMU_MAX;
  ne = ne < SK(end_time) ? ne : SK(end_time);
  e.active = e.min_next < ne ? 1u : 0u;
  e.ws = e.min_next;
  e.we = ne;
  return e;
}

// Workgroup 0's bookkeeping of a finished round [ws, we) (lane-parallel plain stores).
template <class SV>
__device__ __forceinline__ void rb_bookkeep(const SV& S, uint64_t ws, uint64_t we, uint64_t nb1,
                                            uint32_t new_keep) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t b0 = bucket_of(S, ws), b1 = bucket_of(S, we - 1);
  const uint32_t nc = (b1 - b0) & (SK(NB) - 1);
  for (uint32_t i = lane; i < nc; i += 64) st_dev(&SK(bucket_min)[(b0 + i) & (SK(NB) - 1)], (uint64_t)INVALID);
  if (lane == 0) {
    st_dev(&SK(bucket_min)[b1], nb1);
    st_dev(&SK(bucket_slab)[b1], new_keep);
  }
}

// Persistent rounds (single shard): the grid stays resident and runs up to max_rounds
// rounds, workgroup w serving groups w, w + P, ... every round (a group's host state stays
// with one CU). Data another workgroup wrote in this launch is read with device-scope loads
// (event records, slab fills, bucket minima, the round buffers); the rest (host records,
// queues) belongs to this workgroup's groups.
// kBig: compiled with the big-slab path (launched while some slab has an extension; without
// one, the path's code cost config C 2.6 % per launch in same-box A/B, round 4)

// Round buffer q of a grid of nch chunks, reset by the bookkeeping workgroup: chunk minima and
// occupancy sums, the counters of both barriers (the grid's chunks, then the top counter; the
// second barrier's and the exports: k_rounds_x, null in a single shard), the spare-slab minimum
// and the freed / allocated / spilled counts.
template <uint32_t kApp, bool kX, class SV>
__device__ __forceinline__ void rb_reset(const SV& S, uint32_t q, uint32_t nch) {
  using Y = RbLayout<kApp>;
  for (uint32_t i = threadIdx.x; i < nch; i += 64) {
    st_dev(&SK(rb_min)[((size_t)q * RB_CH + i) * Y::MS], (uint64_t)INVALID);
    st_dev(&SK(rb_min)[((size_t)q * RB_CH + i) * Y::MS + 1], (uint64_t)INVALID);
    st_dev(&SK(rb_occ)[((size_t)q * RB_CH + i) * Y::OS], (uint64_t)0);
  }
  for (uint32_t i = threadIdx.x; i <= nch; i += 64) {
    const size_t o = (size_t)q * Y::CB + (i == nch ? RB_CH : i) * Y::CS;
    st_dev(&SK(rb_cnt)[o], 0u);
    if constexpr (kX) st_dev(&SK(rb2_cnt)[o], 0u);
  }
  if constexpr (kX)
    for (uint32_t i = threadIdx.x; i < SK(n_ranks); i += 64) {
      st_dev(&SK(xout_n)[q * SK(n_ranks) + i], 0u);
      st_dev(&SK(xout_n)[(3 + q) * SK(n_ranks) + i], 0u);  // (k_rounds_x: the per-peer totals)
    }
  if (threadIdx.x == 0) {
    st_dev(&SK(rb_keep)[q], (uint64_t)INVALID);
    st_dev(&SK(rb_free)[q], (uint64_t)0);
    st_dev(&SK(rb_occ)[3 * RB_CH * RB_OS_MAX + q], (uint64_t)0);
    st_dev(&SK(rb_occ)[3 * RB_CH * RB_OS_MAX + 3 + q], (uint64_t)0);
  }
}
// The persistent kernels' per-launch state, reset by the launch itself (no host memsets before
// a launch): round buffer 0 and the idle-gap counter, by the shard's
// bookkeeping workgroup BEFORE it counts itself into the residency census — every workgroup
// waits for the whole census, so no arrival can reach the buffers first. Buffers 1 and 2 are
// reset during rounds 0 and 1 (buffer (r + 1) % 3 during round r).
template <uint32_t kApp, bool kX, class SV>
__device__ __forceinline__ void rb_reset0(const SV& S, uint32_t nch) {
  rb_reset<kApp, kX>(S, 0, nch);
  if (threadIdx.x == 0) st_dev(&SK(rb_cnt)[3 * RB_CB_MAX], 0u);  // the idle-gap barrier's counter
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// A workgroup of k_rounds that gives up on a barrier (OVF_TIMEOUT) may do so after the
// bookkeeping workgroup copied the control block into host memory: it also marks the copy
// stale (the word after the epoch), and the host then reads the device's block.
__device__ __forceinline__ void fail_timeout(const DevSim& S) {
  atomicOr((unsigned int*)&SK(ctrl)->overflow, OVF_TIMEOUT);
  if (SK(ctrl_mirror)) st_sys(&SK(ctrl_mirror)[kMirrorWords - 1], 1ull);
}

// Residency census (thread 0 of each workgroup): the workgroup counts itself in and waits,
// bounded, for the whole grid of P; the first to see it, or to give up, sets the verdict with a
// compare-and-swap, so every workgroup acts on the same one. The arrival counter is never reset
// (the host passes its value before the launch, base) and the verdict carries the launch's epoch
// (epoch << 2 | verdict: 1 resident, 2 not). *decided: this workgroup set it.
__device__ __forceinline__ uint32_t census(SGN_GLB Ctrl* C, uint32_t P, uint32_t epoch, uint32_t base,
                                           bool* decided) {
  __hip_atomic_fetch_add(&C->res_arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t want = epoch << 2;
  uint32_t v = 0, spins = 0;
  *decided = false;
  while (((v = ld_dev(&C->res_verdict)) & ~3u) != want) {
    uint32_t nv;
    if (ld_dev(&C->res_arrive) - base >= P) {
      nv = want | 1u;
    } else if (++spins > (1u << 14)) {
      nv = want | 2u;
    } else {
      __builtin_amdgcn_s_sleep(2);
      continue;
    }
    uint32_t expect = v;
    if (__hip_atomic_compare_exchange_strong(&C->res_verdict, &expect, nv, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      *decided = true;
  }
  return v & 3u;
}

template <bool kTab>
__device__ __forceinline__ decltype(auto) sim_view(const DevSim* __restrict__ Sg) {
  if constexpr (kTab)
    return ktab_fill(Sg);
  else
    return (*Sg);
}

// ---- the steps of a persistent round that k_rounds and k_rounds_x share ----
// Each kernel keeps its round state in a RoundLDS of its own (k_rounds_x packs its flags into half
// words and adds the exchange's); the steps below take either one.

// Launch prologue (thread 0): the control block into the workgroup's round state.
template <class RS>
__device__ __forceinline__ void round_state_load(RS& rs, SGN_GLB Ctrl* C) {
  rs.pg_avail = ld_dev(&C->pg_avail);
  rs.ws = ld_dev(&C->ws);
  rs.we = ld_dev(&C->we);
  rs.active = (decltype(rs.active))ld_dev(&C->active);
  rs.ks = ld_dev(&C->keep_slab);
  rs.pend = 0;
  rs.ngap = 0;
  rs.pg_alloc = ld_dev(&C->pg_alloc);
  rs.occ = ld_dev(&C->cal_occ);
  rs.hold = ld_dev(&C->hold);  // (a round still held: the launch returns at once)
  rs.hold_need = ld_dev(&C->hold_need);
  rs.pause_at = ld_dev(&C->pause_at);  // (read once: every workgroup decides alike; the host
                                       // writes every shard the same target)
}

// Launch epilogue (the bookkeeping workgroup's thread 0): the round state into the host-visible
// control block. rounds: the control block's round count after this launch; spill_imp
// (k_rounds_x): the spill-area entries that may hold imported runs.
template <class RS>
__device__ __forceinline__ void round_state_store(SGN_GLB Ctrl* C, const RS& rs, uint64_t rounds,
                                                  const uint64_t* spill_imp) {
  st_dev(&C->keep_slab, rs.ks);
  st_dev(&C->ws, rs.ws);
  st_dev(&C->we, rs.we);
  st_dev(&C->active, (uint32_t)rs.active);
  st_dev(&C->rounds, rounds);
  st_dev(&C->pg_avail, rs.pg_avail);
  st_dev(&C->cal_occ, rs.occ);
  if (spill_imp)
    (void)__hip_atomic_fetch_max(&C->spill_imp, *spill_imp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (rs.hold) {
    st_dev(&C->hold, rs.hold);
    st_dev(&C->hold_need, rs.hold_need);
  }
}

// Per round (thread 0): the outbox header of round buffer p for the window starting at ws.
template <class SV>
__device__ __forceinline__ void ob_round_begin(const SV& S, const ExecLDS& X, uint32_t p, uint64_t ws,
                                               uint64_t pg_avail) {
  X.ob->keepmin = &SK(rb_keep)[p];
  X.ob->bbase = ws;
  X.ob->pg_avail = pg_avail;
  X.ob->pg_freed = &SK(rb_free)[p];
  X.ob->pg_allocd = &SK(rb_occ)[3 * RB_CH * RB_OS_MAX + p];
  X.ob->spilled = &SK(rb_occ)[3 * RB_CH * RB_OS_MAX + 3 + p];
}

// The idle gap after the round [ws, we) whose next window ends at nwe. This round's bucket
// bookkeeping (consumed minima -> INVALID, bucket b1 -> nb1) is done by the bookkeeping workgroup
// during the next round, with plain stores: safe while the next round's sends cannot reach this
// round's buckets. They can after an idle gap: a send at t maps to this round's bucket indices
// again once t >= bucketstart(ws) + NB * BW, and t < nwe + max_lat. Then (every workgroup decides
// alike) the bookkeeping workgroup does it now and a second grid barrier keeps every send of the
// next round behind it (a lost bucket minimum). bk: this is the bookkeeping workgroup.
// Returns whether the gap was taken; timed_out(): what the kernel does when the barrier does not complete.
template <class SV, class RS, class OnTimeout>
__device__ __forceinline__ bool gap_barrier(const SV& S, RS& rs, bool bk, uint32_t P, uint64_t ws, uint64_t we,
                                            uint32_t ks, uint32_t active, uint64_t nwe, uint64_t nb1,
                                            OnTimeout&& timed_out) {
  const uint64_t span = (uint64_t)SK(NB) * SK(BW);
  const uint64_t bstart = SIM_START + SK(bw_div).div(ws - SIM_START) * SK(BW);
  const bool gap = active && (nwe + SK(max_lat) >= bstart + span || nwe + SK(max_lat) < nwe);
  if (gap) {
    if (bk) rb_bookkeep(S, ws, we, nb1, ks);  // (the previous round's: done at this round's start)
    if (threadIdx.x == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the bookkeeping workgroup's stores are done
      SGN_GLB uint32_t* gc = SK(rb_cnt) + 3 * RB_CB_MAX;
      const uint32_t target = (rs.ngap + 1) * P;
      __hip_atomic_fetch_add(gc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      uint32_t sp = 0;
      while (ld_dev(gc) < target && ++sp < (1u << 24)) __builtin_amdgcn_s_sleep(2);
      if (sp >= (1u << 24)) timed_out();
      rs.ngap++;
    }
  }
  return gap;
}

// Round end (thread 0), after the barrier: the spare slab set (survivors + this round's new runs
// for b1 = bucket_of(S, we - 1), the window's last bucket) becomes bucket b1 — in the workgroup's own bucket -> slab
// table when it keeps one (lds_tab) —, the finished round's bookkeeping is left for the next
// round's start unless the idle gap did it, the next window [nws, nwe), and the round's freed and
// allocated pages and occupancy change (all written: barrier).
template <class SV, class RS>
__device__ __forceinline__ void round_state_advance(const SV& S, const ExecLDS& X, RS& rs, bool lds_tab, uint32_t b1,
                                                    uint64_t ws, uint64_t we, uint32_t ks, bool gap, uint64_t nb1,
                                                    uint64_t nws, uint64_t nwe, uint32_t active, uint64_t nfree,
                                                    uint64_t nalloc, uint64_t occd) {
  const uint32_t slab_b1 = lds_tab ? X.lbs[b1] : ld_dev(&SK(bucket_slab)[b1]);
  if (lds_tab) X.lbs[b1] = (uint16_t)ks;
  rs.pend = gap ? 0u : 1u;
  rs.pend_ws = ws;
  rs.pend_we = we;
  rs.pend_nb1 = nb1;
  rs.pend_new = ks;
  rs.ks = slab_b1;
  rs.ws = nws;
  rs.we = nwe;
  rs.active = active;
  rs.pg_avail += nfree;
  rs.pg_alloc += nalloc;
  rs.occ += occd;
}

// Launch end: the launch's per-wave statistics, in the slot of this workgroup's first group (the
// host sums the slots; the mapping is a bijection, so gq0 < G is this workgroup's alone — a forced
// grid larger than G has workgroups w >= G; one without groups has nothing to flush)
template <class SV>
__device__ __forceinline__ void wacc_flush(const SV& S, const ExecLDS& X, uint32_t gq0, uint32_t gq1) {
  __syncthreads();
  if (X.wacc && threadIdx.x < W_N && X.wacc[threadIdx.x] && gq0 < gq1) {
    const uint32_t k = threadIdx.x;
    if (k == W_MAXFILL)
      __hip_atomic_fetch_max(&SK(w_cnt)[k * SK(G) + gq0], X.wacc[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      cnt_add(&SK(w_cnt)[k * SK(G) + gq0], X.wacc[k]);
  }
}

template <uint32_t kApp, bool kBig, bool kDiag>
__device__ __forceinline__ void rounds_body(const DevSim* __restrict__ Sg, uint32_t max_rounds, uint32_t epoch,
                                            uint32_t res_base) {
  // TGEN: the lane table, filled here under full EXEC (every workgroup is one whole wave), once
  // per launch: the host writes the device's DevSim only between launches (sim_upload)
  decltype(auto) S = sim_view<kKtab<kApp>>(Sg);
  SGN_GLB Ctrl* C = SK(ctrl);
  SGN_EXEC_LDS(X)
  // PERIODIC (configs B, D): the per-wave statistics in LDS for the launch (B: ~70 % of the
  // PMC writes were their per-round atomics); TGEN keeps the per-round no-return adds (config
  // C: 0.45 % faster per launch without the LDS accumulator, same-box A/B)
  if constexpr (kApp == SGN_TRAFFIC_PERIODIC) {
    __shared__ uint64_t wacc_[W_N];
    X.wacc = wacc_;
    if (threadIdx.x < W_N) wacc_[threadIdx.x] = 0;
  }
  const uint32_t w = blockIdx.x, P = gridDim.x;
  // the workgroup's groups: [gq0, gq1) in steps of gqs (wg_groups, sgn_internal.h)
  uint32_t gq0, gq1, gqs;
  wg_groups<kApp>(SK(G), w, P, gq0, gq1, gqs);
  // Residency census before any simulation state is touched: the grid barrier below needs
  // every workgroup on the chip at once. Each workgroup counts itself in and waits (bounded)
  // for the rest; the first to see the whole grid, or to give up, sets the verdict with a
  // compare-and-swap, so all workgroups act on the same one. A grid that is not resident
  // leaves untouched and the host runs the rounds with per-round launches instead.
  {
    __shared__ uint32_t verdict;
    if (w == P - 1) rb_reset0<kApp, false>(S, (P + 63) >> 6);
    if (threadIdx.x == 0) {
      bool decided;
      verdict = census(C, P, epoch, res_base, &decided);
    }
    __syncthreads();
    if (verdict != 1) return;
  }
  const uint32_t nch = (P + 63) >> 6;
  // the workgroup that does the shared bookkeeping (the previous round's bucket minima and
  // slab table, the next round buffer's reset, the control block): the last one, whose group
  // is a client group (slots start with the TGEN servers, whose groups are the slowest)
  const uint32_t wbk = P - 1;
  // The round state every workgroup keeps for itself, in LDS (registers are the scarce
  // resource of the round kernel): the window, the spare slab, and the previous round's
  // bookkeeping that workgroup 0 does during the next round. The bucket -> slab table
  // changes by one swap per round, applied by every workgroup to its own LDS copy.
  struct RoundLDS {
    uint64_t ws, we, pend_ws, pend_we, pend_nb1, pg_avail;
    uint64_t pg_alloc, occ, nspill, hold_need;  // CoDel pages taken, calendar runs, runs spilled
    uint64_t pause_at;                          // Ctrl::pause_at as of the launch (sgn_run_until)
    uint32_t active, ks, pend_new, pend, ngap, hold;
  };
  __shared__ RoundLDS rs;
  if (threadIdx.x == 0) {
    round_state_load(rs, C);
    rs.nspill = ld_dev(&C->spill_n);
  }
  // (the launch's first round number is read back at its end: nothing else writes it, and a
  // register live across the whole launch spilled the PERIODIC big-slab kernel)
  const bool lds_tab = SK(NB) <= LDS_BSLAB;
  if (lds_tab)
    for (uint32_t i = threadIdx.x; i < SK(NB); i += 64) X.lbs[i] = (uint16_t)ld_dev(&SK(bucket_slab)[i]);
  init_bmin<kApp>(S, X);
  __syncthreads();
  uint32_t r = 0;
  for (; r < max_rounds; r++) {
    // (a held round: the host grows a pool between launches, then the round runs)
    if (!__builtin_amdgcn_readfirstlane((int)rs.active) || __builtin_amdgcn_readfirstlane((int)rs.hold)) break;
    const uint64_t ws = uni64(rs.ws), we = uni64(rs.we);
    const uint32_t ks = (uint32_t)__builtin_amdgcn_readfirstlane((int)rs.ks);
    const uint32_t p = r % 3;
    if (w == wbk) {
      if (rs.pend) rb_bookkeep(S, rs.pend_ws, rs.pend_we, rs.pend_nb1, rs.pend_new);
      rb_reset<kApp, false>(S, (r + 1) % 3, nch);  // for the next round
    }
    // diagnostics (SGN_STAMPS): per round of this launch, {earliest start, latest arrival,
    // round edge known} on the 100 MHz clock
    SGN_GLB uint64_t* rd = kDiag && SK(rdbg) ? SK(rdbg) + 3 * (size_t)(r & 127) : nullptr;
    if (rd && threadIdx.x == 0)
      __hip_atomic_fetch_min(rd, (unsigned long long)__builtin_amdgcn_s_memrealtime(),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0) ob_round_begin(S, X, p, ws, rs.pg_avail);
    uint64_t kall = INVALID, mall = INVALID, oall = 0;
    bool arrived = false;
    for (uint32_t g = gq0; g < gq1; g += gqs) {
      uint64_t kmin, m;
      const bool lastg = g + gqs >= gq1;  // the workgroup's last group arrives
      exec_group<false, kApp, kBig, false, kDiag>(S, g, ws, we, ks, X, &kmin, &m, [&](uint64_t k, uint64_t n, uint64_t od) {
        kall = k < kall ? k : kall;
        mall = n < mall ? n : mall;
        oall += od;
        if (lastg) {
          if (rd && threadIdx.x == 0)
            __hip_atomic_fetch_max(rd + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime(),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          flush_bmin<kApp>(S, X);
          rb_arrive<kApp>(S, p, w, P, kall, mall, oall);
          arrived = true;
        }
      });
      __syncthreads();
    }
    if (!arrived) rb_arrive<kApp>(S, p, w, P, INVALID, INVALID, 0);  // a workgroup without groups
    // grid barrier: every chunk complete, bounded
    uint32_t spins = 0;
    bool ok = true;
    while (ld_dev(&SK(rb_cnt)[(size_t)p * RbLayout<kApp>::CB + RB_CH * RbLayout<kApp>::CS]) < nch) {
      // (TGEN: 1563 workgroups poll one word; a longer sleep between polls leaves the memory
      // side to the last arrivals' atomics: same-box A/B on C, 3639 -> 3586 us per 100-round
      // launch; PERIODIC: 8, see RbLayout)
      __builtin_amdgcn_s_sleep(kApp == SGN_TRAFFIC_TGEN ? 16 : kApp == SGN_TRAFFIC_PERIODIC ? 8 : 1);
      if (++spins > (1u << 22)) {
        ok = false;
        break;
      }
    }
    if (!ok) {
      if (threadIdx.x == 0) fail_timeout(sk_mem(S));
      return;
    }
    asm volatile("" ::: "memory");
    const RbEdge e = rb_edge<kApp>(S, p, nch, ws, we);
    if (rd && w == wbk && threadIdx.x == 0) st_dev(rd + 2, (uint64_t)__builtin_amdgcn_s_memrealtime());
    const bool gap =
        gap_barrier(S, rs, w == wbk, P, ws, we, ks, e.active, e.we, e.nb1, [&] { fail_timeout(sk_mem(S)); });
    __syncthreads();
    if (threadIdx.x == 0) {
      round_state_advance(S, X, rs, lds_tab, bucket_of(S, we - 1), ws, we, ks, gap, e.nb1, e.ws, e.we, e.active,
                          e.nfree, e.nalloc, e.occd);
      rs.nspill += e.nspill;
      if (e.active) {  // the next round's guards: every workgroup decides alike (same values)
        const uint64_t need = codel_round_bound(S, rs.occ, e.ws, e.we);
        rs.hold = (pages_free(rs.pg_avail, rs.pg_alloc) < need ? HOLD_CODEL : 0u) | (rs.nspill ? HOLD_SPILL : 0u) |
                  (e.ws >= rs.pause_at ? HOLD_PAUSE : 0u);
        rs.hold_need = need;
      }
      if (w == wbk) {
        st_dev(&C->last_min_next, e.min_next);
        st_dev(&C->prev_we, we);
      }
    }
    __syncthreads();
  }
  wacc_flush(S, X, gq0, gq1);
  // the last round's bookkeeping and the host-visible control block
  if (w == wbk) {
    if (rs.pend) rb_bookkeep(S, rs.pend_ws, rs.pend_we, rs.pend_nb1, rs.pend_new);
    if (threadIdx.x == 0) round_state_store(C, rs, ld_dev(&C->rounds) + r, nullptr);
    // ... and its copy in host memory: after the last barrier no other workgroup writes the
    // control block (their counters and flags arrived with them)
    if (SK(ctrl_mirror)) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      constexpr uint32_t NW = sizeof(Ctrl) / 8;
      for (uint32_t i = threadIdx.x; i < NW; i += 64) st_sys(&SK(ctrl_mirror)[i], ld_dev(&((SGN_GLB uint64_t*)C)[i]));
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (threadIdx.x == 0) st_sys(&SK(ctrl_mirror)[NW], (uint64_t)epoch);
    }
  }
}

// The product kernel, and its twin with the diagnostics (SGN_STAMPS: per-wave stamps, the
// per-round timeline). The stamps' clocks, accumulators and pointers stay live across the event
// loop, where the product kernel has no scalar register to spare.
template <uint32_t kApp, bool kBig>
__global__ __launch_bounds__(64, 2) void k_rounds(const DevSim* __restrict__ Sg, uint32_t max_rounds, uint32_t epoch,
                                                  uint32_t res_base) {
  rounds_body<kApp, kBig, false>(Sg, max_rounds, epoch, res_base);
}
template <uint32_t kApp, bool kBig>
__global__ __launch_bounds__(64, 2) void k_rounds_diag(const DevSim* __restrict__ Sg, uint32_t max_rounds,
                                                       uint32_t epoch, uint32_t res_base) {
  rounds_body<kApp, kBig, true>(Sg, max_rounds, epoch, res_base);
}

// ---- persistent multi-shard rounds (k_rounds_x) ----
// N shards, each on its own GPU (one launch per GPU) or, for the one-GPU rehearsal, on its own
// range of workgroups of ONE launch. A round of shard s is the single-shard persistent round
// (k_rounds) plus the exchange that replaces the RCCL send/recv and k_import — in the source too:
// both kernels call the shared round steps above (wg_groups, rb_reset0 / rb_reset,
// round_state_load, ob_round_begin, gap_barrier, round_state_advance, wacc_flush,
// round_state_store) and the local round edge (rb_edge, rb_bookkeep); what is written here only is
// the exchange (the arrival that learns it is last, the messages, the imports: file_run):
//  1. execute: runs for another shard's hosts go straight into that shard's inbox slot for this
//     shard and round parity (peer-mapped memory, system-scope write-through stores), counted
//     per peer in local counters (Worker::send_packet pushes into the destination host's queue
//     from any thread: core/worker.rs:603-613);
//  2. the local barrier (k_rounds' chunk counters) and the local round edge (rb_edge: this
//     shard's minima, the runs it exported included);
//  3. the shard's last workgroup writes one 128-B message per shard (its own included) into the
//     receivers' inboxes — run count, min next event, min used latency, the pool figures every
//     shard needs for the same hold decisions — and then, after every store has completed, the
//     message's tag (the global round number);
//  4. every workgroup waits for the N messages of its own inbox and computes the next window
//     from them: the min over messages is the min over all pending events (each message counts
//     its shard's, exported runs included), i.e. the RCCL min all-reduce of the north star and
//     Controller::manager_finished_current_round (controller.rs:88-112) over the global min;
//  5. the workgroups file the runs of their inbox into the local calendar (k_import's work) and
//     meet at a second local barrier before the next round's gathers read the slabs.
// Inbox slots alternate by round parity: a sender writes round r + 1's runs while the receiver
// may still be filing round r's. Rounds that would need more than a slot, or a larger pool, or a
// re-layout, are held on every shard alike (the same messages, the same decisions) and the host
// completes them between launches.
// The round-edge messages across GPUs: a system-scope release before them (kept: it costs
// nothing measurable), and no system-scope acquire after them. The acquire (buffer_inv sc0 sc1
// in every workgroup, every round) cost 9 us per round on the two-process rehearsal (41.6 ->
// 50.6 us, profiles/r06/xfence_ab.txt), and every byte it would order is read by system-coherent
// loads anyway: the tags by an asm global_load sc0 sc1 followed by s_waitcnt vmcnt(0), so every
// later load issues after the tag was read, and the bins and slots by sc0 sc1 loads of uncached
// memory (no cache can hold an older copy). SGN_XACQ builds it in (for that price), SGN_XNOFENCE
// builds neither (experiments only, build_exp.sh).
#ifdef SGN_XNOFENCE
constexpr bool kXFenceRel = false, kXFenceAcq = false;
#elif defined(SGN_XACQ)
constexpr bool kXFenceRel = true, kXFenceAcq = true;
#else
constexpr bool kXFenceRel = true, kXFenceAcq = false;
#endif
#ifdef SGN_KX_NOBIG  // cost experiment only (build_exp.sh): k_rounds_x without the big-slab path
constexpr bool kKxBig = false;
#else
constexpr bool kKxBig = true;
#endif
// shards of up to this many workgroups arrive on one counter (k_rounds' chunk counters take
// two returning atomics for the last arrival; at config C's ~200 workgroups per shard, spread
// over the round's ~15 us of arrivals, one counter does not queue)
constexpr uint32_t kXFlat = 256;
constexpr uint64_t kXWaitTicks = 2000000000ull;  // 20 s on the 100 MHz clock: a peer that never
                                                 // answers is an error (OVF_TIMEOUT), not a hang
// the census across GPUs: 60 s, so that shards whose launches start far apart (one of them
// re-laying its calendar out or growing a pool first) wait instead of failing
constexpr uint64_t kXCensusTicks = 6000000000ull;

template <uint32_t kApp>
__device__ __forceinline__ bool rb_wait(SGN_GLB uint32_t* top, uint32_t nch) {
  uint32_t spins = 0;
  while (ld_dev(top) < nch) {
    __builtin_amdgcn_s_sleep(kApp == SGN_TRAFFIC_TGEN ? 16 : kApp == SGN_TRAFFIC_PERIODIC ? 8 : 1);
    if (++spins > (1u << 22)) return false;
  }
  return true;
}

// the second local barrier (after the imports): chunk counters, then the top counter
template <uint32_t kApp>
__device__ __forceinline__ void rb2_arrive(const DevSim& S, uint32_t p, uint32_t w, uint32_t nw) {
  if (threadIdx.x != 0) return;
  using Y = RbLayout<kApp>;
  const uint32_t ch = w >> 6;
  const uint32_t csz = min(64u, nw - (ch << 6));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this workgroup's imports are in place
  SGN_GLB uint32_t* cnt = S.rb2_cnt + (size_t)p * Y::CB;
  const uint32_t c = __hip_atomic_fetch_add(&cnt[ch * Y::CS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (c == csz - 1) (void)__hip_atomic_fetch_add(&cnt[RB_CH * Y::CS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the local arrival of k_rounds_x (k_rounds' chunk counters): *last = 1 for the workgroup whose
// count completes the shard's barrier (it computes the round edge and sends the messages)
template <uint32_t kApp>
__device__ __forceinline__ void rb_arrive_x(const DevSim& S, uint32_t p, uint32_t w, uint32_t nw, uint64_t kmin,
                                            uint64_t m, uint64_t occd, uint32_t* last, const uint32_t* xc) {
  // this workgroup's runs per peer this round (LDS, bins and slots) into the shard's totals
  if (xc && threadIdx.x < S.n_ranks && threadIdx.x != S.rank) {
    const uint32_t v = xc[threadIdx.x];
    if (v)
      (void)__hip_atomic_fetch_add(&S.xout_n[(size_t)(3 + p) * S.n_ranks + threadIdx.x], v, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x != 0) return;
  const uint32_t ch = w >> 6;
  const uint32_t csz = min(64u, nw - (ch << 6));
  const uint32_t nch = (nw + 63) >> 6;
  using Y = RbLayout<kApp>;
  SGN_GLB uint64_t* mn = S.rb_min + ((size_t)p * RB_CH + ch) * Y::MS;
  if (kmin != INVALID) min_nr(mn, kmin);
  if (m != INVALID) min_nr(mn + 1, m);
  if (occd) cnt_add(&S.rb_occ[((size_t)p * RB_CH + ch) * Y::OS], occd);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this round's stores and atomics done
  SGN_GLB uint32_t* cnt = S.rb_cnt + (size_t)p * Y::CB;
  uint32_t l = 0;
  if (nw <= kXFlat) {  // one counter: the last arrival learns it in one round trip
    l = __hip_atomic_fetch_add(&cnt[RB_CH * Y::CS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nw - 1 ? 1u : 0u;
  } else {
    const uint32_t c = __hip_atomic_fetch_add(&cnt[ch * Y::CS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c == csz - 1)
      l = __hip_atomic_fetch_add(&cnt[RB_CH * Y::CS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nch - 1 ? 1u : 0u;
  }
  *last = l;
}

// a 16-byte message granule {value, tag}: one load (device scope: sc1; system: sc0 sc1)
__device__ __forceinline__ u64x2 ld_gran16(SGN_GLB const uint64_t* p, bool sys) {
  u64x2 v;
  if (sys)
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"((uint64_t)p) : "memory");
  else
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"((uint64_t)p) : "memory");
  return v;
}

// A run another shard sent, for group g, into the calendar with the workgroup's bucket -> slab
// table as it is now: a run at or past the horizon fhz is an overflow (OVF_HORIZON); the bucket
// minimum except in the sbn buckets from sb0 (the window the run will be gathered in). Returns
// whether the run went past its slab: into the extension, or the spill area — the gathers read it
// there, and the spill flag holds the round after on every shard for the re-layout.
__device__ __forceinline__ bool file_run(const DevSim& S, const ExecLDS& X, SGN_GLB Ctrl* C, const EvRec& ev,
                                         uint32_t g, uint64_t fhz, uint32_t sb0, uint32_t sbn) {
  if (ev.time >= fhz) {
    if ((atomicOr(&C->overflow, OVF_HORIZON) & OVF_HORIZON) == 0) C->overflow_info = ev.dst;
    return false;
  }
  const uint32_t b = bucket_of(S, ev.time);
  const size_t idx = (size_t)X.lbs[b] * S.G + g;
  const uint32_t pos = atomicAdd(&S.slab_n[idx], 1u);
  if (((b - sb0) & (S.NB - 1)) >= sbn) min_nr(&S.bucket_min[b], ev.time);
  if (pos < S.CAP) {
    st_dev_rec(S.pool + idx * S.CAP + pos, ev);
    return false;
  }
  place_overflow(S, nullptr, (uint32_t)idx, pos, ev);
  return true;
}

template <uint32_t kApp>
__global__ __launch_bounds__(64, 2) void k_rounds_x(const XLaunch* __restrict__ L, uint32_t max_rounds) {
  // this workgroup's shard and its place in the shard's range
  const uint32_t nl = L->n_local;
  uint32_t si = 0;
  while (si + 1 < nl && blockIdx.x >= L->base[si + 1]) si++;
  const DevSim& S = *(const DevSim*)L->S[si];
  SGN_GLB Ctrl* C = S.ctrl;
  const uint32_t w_i = blockIdx.x - L->base[si], P_i = L->base[si + 1] - L->base[si];
  SGN_EXEC_LDS(X)
  if constexpr (kApp == SGN_TRAFFIC_PERIODIC) {
    __shared__ uint64_t wacc_[W_N];
    X.wacc = wacc_;
    if (threadIdx.x < W_N) wacc_[threadIdx.x] = 0;
  }
  // the workgroup's groups, as in k_rounds
  uint32_t gq0_i, gq1_i, gqs_i;
  wg_groups<kApp>(S.G, w_i, P_i, gq0_i, gq1_i, gqs_i);
  const uint32_t w = w_i, P = P_i, gq0 = gq0_i, gq1 = gq1_i, gqs = gqs_i;
  const uint32_t R = S.n_ranks, me = S.rank;
  const uint32_t nch = (P + 63) >> 6;
  const uint32_t wbk = P - 1;  // this shard's bookkeeping workgroup (and its messages)
  // residency census over the whole launch (the control block of its first shard), then, one
  // shard per GPU, over the shards: every shard publishes its verdict to every inbox and waits for
  // all of them — a grid that is not resident anywhere makes every shard fall back alike
  {
    __shared__ uint32_t verdict;
    SGN_GLB Ctrl* C0 = L->S[0]->ctrl;
    const uint32_t ep32 = (uint32_t)L->epoch << 2;
    if (w == P - 1 && !L->refuse) rb_reset0<kApp, true>(S, (P + 63) >> 6);
    if (threadIdx.x == 0) {
      bool decided = true;
      // (a refused launch is one workgroup on a GPU that cannot hold the grid: it only tells the
      // peers, so that every shard falls back together — ADVICE r5)
      uint32_t v = L->refuse ? 2u : census(C0, gridDim.x, (uint32_t)L->epoch, L->res_base, &decided);
      if (L->refuse) st_dev(&C->res_verdict, ep32 | 2u);
      if (L->peers_census) {
        const uint64_t ep = L->epoch << 2;
        if (decided) {
          // the deciding workgroup tells every shard (its own inbox too), then combines the
          // peers' verdicts for its whole shard under ONE deadline: a peer that is not resident,
          // or never answers, stops this shard too
          for (uint32_t q = 0; q < R; q++) st_sys(S.xp[q].cen, ep | v);
          if (v == 1) {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            for (uint32_t q = 0; q < R && v == 1; q++) {
              uint64_t c;
              while (((c = ld_sys(&S.xin_cen[q])) >> 2) != L->epoch) {
                if (__builtin_amdgcn_s_memrealtime() - t0 > kXCensusTicks) {
                  c = ep | 2;
                  atomicOr((unsigned int*)&C->overflow, OVF_TIMEOUT);
                  break;
                }
                __builtin_amdgcn_s_sleep(8);
              }
              if ((c & 3) != 1) v = 3;
            }
          }
          st_dev(&C->res_xverdict, ep32 | v);
        } else if (v == 1) {
          // the other workgroups act on the decider's combined verdict only (its deadline, then
          // a margin: they never time out on their own before it does)
          const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
          uint32_t c;
          while (((c = ld_dev(&C->res_xverdict)) & ~3u) != ep32) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > 2 * kXCensusTicks) {
              c = ep32 | 3u;
              atomicOr((unsigned int*)&C->overflow, OVF_TIMEOUT);
              break;
            }
            __builtin_amdgcn_s_sleep(8);
          }
          v = c & 3u;
        }
      }
      verdict = v;
    }
    __syncthreads();
    if (verdict != 1) {
      if (verdict == 3 && w == P - 1 && threadIdx.x == 0) st_dev(&C->res_verdict, ep32 | 3u);
      return;
    }
  }
  struct RoundLDS {
    uint64_t ws, we, pend_ws, pend_we, pend_nb1, pg_avail;
    uint64_t pg_alloc, occ, hold_need;
    uint64_t pause_at;           // Ctrl::pause_at as of the launch (sgn_shards_run_until)
    uint32_t ks, pend_new, ngap, hold;
    // (flags, as half words: with them pause_at costs this kernel no LDS — config C's grid stays
    // resident only while the static LDS stays within its 512-byte granule)
    uint16_t active, pend, fpend, fbuf;  // fpend, fbuf: imports left for the next round's start
                                         // (and their slot parity; their horizon: the round pend_ws started)
    // runs to file from the inbox slots this round: in all, and from each shard (nin, from the
    // exchange until they are filed); while the workgroup executes, nin counts its runs to each
    // shard instead (OutboxHdr::xc; reset after the filing, flushed at the arrival)
    uint32_t n_in, nin[XR_MAX];
    uint32_t last;               // this workgroup arrived last at the shard's local barrier
  };
  __shared__ RoundLDS rs;
  if (threadIdx.x == 0) {
    round_state_load(rs, C);
    rs.fpend = 0;
    rs.n_in = 0;
    rs.last = 0;
    rs.pend_ws = rs.ws;
    // (every spill-area entry so far may hold an import a gather must read: the re-layout at a
    // held edge empties the area)
    X.big->spill_imp = ld_dev(&C->spill_n);
  }
  const uint64_t rounds0 = ld_dev(&C->rounds);
  // the calendar horizon of a round starting at ws0 (OutboxHdr::hz)
  auto hz_of = [&](uint64_t ws0) { return SIM_START + (S.bw_div.div(ws0 - SIM_START) + S.NB) * S.BW; };
  // this workgroup's share of the senders' bin counters of round parity k (zeroed in the round
  // before their next use: no workgroup of this shard sends with them then)
  auto bin_counters_reset = [&](uint32_t k) {
    if (!S.xin_bins) return;
    const uint32_t nb = R * S.xgx;
    for (uint32_t i = w * 64 + threadIdx.x; i < nb; i += P * 64) st_dev(&S.xbin_n[(size_t)k * nb + i], 0u);
  };
  // The runs other shards sent this shard (inbox slot parity fbuf, rs.nin per sender) into the
  // calendar with the bucket -> slab table as it is now; their bucket minima except for the
  // buckets of the window [nws, nwe) they will be gathered in (its first bucket's minimum is not
  // read while it is the window's, and its last bucket's later runs join the kept minimum).
  // own: this workgroup's groups only (every workgroup scans every run: no barrier needed
  // before its own gathers); else a share of all of them (then a barrier).
  auto file_in = [&](uint32_t fbuf, uint64_t fhz, uint64_t nws, uint64_t nwe, bool own) {
    uint32_t ln = threadIdx.x;
    asm volatile("" : "+v"(ln));
    const uint32_t sb0 = bucket_of(S, nws), sbn = ((bucket_of(S, nwe - 1) - sb0) & (S.NB - 1)) + 1;
    const uint32_t n = rs.n_in;
    for (uint32_t i = (own ? 0u : w * 64) + ln; i < n; i += own ? 64u : P * 64) {
      uint32_t q = 0, off = i;
      while (off >= rs.nin[q]) off -= rs.nin[q++];
      SGN_GLB const EvRec* src = S.xin_runs + ((size_t)fbuf * R + q) * S.xislot + off;
      const EvRec ev = S.xsys ? ld_sys_rec(src) : ld_dev_rec(src);
      const uint32_t g = (ev.dst - S.lo) >> S.gsh;
      if (own && (g < gq0 || g >= gq1 || (g - gq0) % gqs != 0)) continue;
      (void)file_run(S, X, C, ev, g, fhz, sb0, sbn);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  for (uint32_t i = threadIdx.x; i < S.NB; i += 64) X.lbs[i] = (uint16_t)ld_dev(&S.bucket_slab[i]);
  init_bmin<kApp>(S, X);
  __syncthreads();
  uint32_t r = 0;
  for (; r < max_rounds; r++) {
    if (!__builtin_amdgcn_readfirstlane((int)rs.active) || __builtin_amdgcn_readfirstlane((int)rs.hold)) break;
    const uint64_t ws = uni64(rs.ws), we = uni64(rs.we);
    const uint32_t ks = (uint32_t)__builtin_amdgcn_readfirstlane((int)rs.ks);
    const uint32_t p = r % 3;
    if (w == wbk) {
      if (rs.pend) rb_bookkeep(S, rs.pend_ws, rs.pend_we, rs.pend_nb1, rs.pend_new);
      rb_reset<kApp, true>(S, (r + 1) % 3, nch);  // for the next round: both barriers and the exports too
    }
    // (the bins this round's gathers read were filled with parity (rounds0 + r) & 1 last round;
    // the next round sends with it again)
    bin_counters_reset((uint32_t)((rounds0 + r) & 1));
    if (threadIdx.x == 0) {
      ob_round_begin(S, X, p, ws, rs.pg_avail);
      X.ob->xn = S.xout_n + (size_t)p * R;
      X.ob->xc = S.xin_bins ? rs.nin : nullptr;
      X.ob->xbuf = (uint32_t)((rounds0 + r + 1) & 1);
    }
    // diagnostics (SGN_STAMPS=2): per round of this launch, on the 100 MHz clock: {earliest start,
    // latest local arrival, local barrier seen (last workgroup), its messages sent, latest "all
    // messages seen", latest imports filed, latest second barrier seen}
    // (SGN_STAMPS=3: every workgroup's own stamps, plain stores: [128 rounds][2048][8])
    SGN_GLB uint64_t* rd = S.rdbg ? S.rdbg + (S.rdbg_wg ? ((size_t)(r & 127) * 2048 + w) * 8 : 8 * (size_t)(r & 127)) : nullptr;
    auto stamp = [&](uint32_t i, bool mx) {
      if (rd && threadIdx.x == 0) {
        const uint64_t t = __builtin_amdgcn_s_memrealtime();
        if (S.rdbg_wg)
          rd[i] = t;
        else if (mx)
          __hip_atomic_fetch_max(rd + i, (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
          __hip_atomic_fetch_min(rd + i, (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    };
    stamp(0, false);
    // the previous round's imports for this workgroup's groups (few of them: every workgroup
    // scans them all instead of a second barrier), before its gathers read the slabs
    if (uni32(rs.fpend)) {
      file_in(rs.fbuf, hz_of(rs.pend_ws), ws, we, true);
      __syncthreads();
      if (threadIdx.x == 0) {
        X.big->spill_imp = ld_dev(&C->spill_n);
        rs.fpend = 0;
      }
      __syncthreads();
    }
    if (threadIdx.x < XR_MAX) rs.nin[threadIdx.x] = 0;  // (now the per-peer send counts: xc)
    // ---- 1. execute this workgroup's groups, then arrive (the last arrival learns it is) ----
    uint64_t kall = INVALID, mall = INVALID, oall = 0;
    bool arrived = false;
    for (uint32_t g = gq0; g < gq1; g += gqs) {
      uint64_t kmin, m;
      const bool lastg = g + gqs >= gq1;
      exec_group<false, kApp, kKxBig, true>(S, g, ws, we, ks, X, &kmin, &m, [&](uint64_t k, uint64_t n, uint64_t od) {
        kall = k < kall ? k : kall;
        mall = n < mall ? n : mall;
        oall += od;
        if (lastg) {
          flush_bmin<kApp>(S, X);
          stamp(1, true);
          rb_arrive_x<kApp>(S, p, w, P, kall, mall, oall, &rs.last, X.ob->xc);
          arrived = true;
        }
      });
      __syncthreads();
    }
    if (!arrived) rb_arrive_x<kApp>(S, p, w, P, INVALID, INVALID, 0, &rs.last, nullptr);
    __syncthreads();
    const uint64_t tag = rounds0 + r + 1;  // the global round number + 1 (the same on every shard)
    const uint32_t buf = (uint32_t)(tag & 1);
    // (the lane index laundered every round: the compiler would otherwise hoist this section's
    // lane-dependent values out of the round loop and keep them in registers through the
    // execute phase, where the round kernels have none to spare)
    uint32_t lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    // ---- 2. the shard's last arrival: its round edge, and its message to every shard ----
    if (uni32(rs.last)) {
      stamp(2, true);
      // the message's own inputs beside the round edge's loads (no dependent round trips)
      SGN_GLB uint64_t* hm = nullptr;
      uint64_t cnt = 0, tot = 0;  // runs to the peer: in its slot; in all (bins and slot)
      if (lane < R) hm = S.xp[lane].hdr[buf];
      if (lane < R && lane != me) {
        cnt = ld_dev(&S.xout_n[(size_t)p * R + lane]);
        tot = S.xin_bins ? (uint64_t)ld_dev(&S.xout_n[(size_t)(3 + p) * R + lane]) : cnt;
      }
      const uint64_t spilled = ld_dev(&C->spill_n);
      const uint64_t mu = ld_dev(&C->min_used);
      const RbEdge e = rb_edge<kApp>(S, p, nch, ws, we);  // (its window: this shard's view only)
      uint64_t xmax = cnt, xsum = tot;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = shfl_xor64(xmax, off);
        xmax = o > xmax ? o : xmax;
        xsum += shfl_xor64(xsum, off);
      }
      if (kXFenceRel && S.xsys) {
        // System-scope release before the message (the peers are other GPUs): every run this
        // shard stored into a peer's bins or slot was a write-through sc0 sc1 store whose wave
        // waited for it (s_waitcnt vmcnt(0)) before arriving, and the arrivals completed before
        // this workgroup learned it is last; the fence writes back anything else of this XCD's
        // L2 and orders it all before the message words. (The wait after it is explicit: the
        // compiler may drop its own, MI355X_MICROARCH.md "compiler hazard".)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      if (lane < R) {
        const uint64_t v[XH_N] = {cnt, e.min_next, mu, xmax, spilled ? 1ull : 0ull,
                                  pages_free(rs.pg_avail + e.nfree, rs.pg_alloc + e.nalloc),
                                  rs.occ + e.occd, xsum, (uint64_t)S.G * S.CAP + S.ext_total, S.nH,
                                  e.nb1, e.occd, e.nalloc, e.nfree, tot};
        // every 8-byte word tagged (xh_lo / xh_hi): across GPUs each is its own 8-byte atomic
        // store, so no receiver relies on a 16-byte store arriving untorn over xGMI
        if (S.xsys) {
#pragma unroll
          for (uint32_t k = 0; k < XH_N; k++) {
            st_sys(hm + 2 * k, xh_lo(v[k], tag));
            st_sys(hm + 2 * k + 1, xh_hi(v[k], tag));
          }
        } else {
#pragma unroll
          for (uint32_t k = 0; k < XH_N; k++) st_wt16(hm + 2 * k, xh_lo(v[k], tag), xh_hi(v[k], tag));
        }
      }
      stamp(3, true);
    }
    // ---- 3. every shard's message (granule q + 8 j: words 2 j, 2 j + 1 of sender q) ----
    uint64_t ga = 0, gb = 0;
    {
      const uint32_t q = lane & 7, jj = lane >> 3;
      const bool mine = q < R && 2 * jj < XH_N;
      SGN_GLB const uint64_t* h = S.xin_hdr + ((size_t)buf * R + q) * XH_WORDS + 4 * jj;
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      bool ok = true;
      // every workgroup of every shard waits here: only the first granule of each message is
      // polled (R lanes; a poll of every granule by every workgroup swamped the L2 channel that
      // holds them), then every granule is read once and its tag checked (re-read if late)
      while (true) {
        bool good = true;
        if (lane < R) {
          const u64x2 x = ld_gran16(S.xin_hdr + ((size_t)buf * R + lane) * XH_WORDS, S.xsys != 0);
          good = xh_ok(x.x, x.y, tag);
        }
        if (__ballot(!good) == 0) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > kXWaitTicks) {
          ok = false;
          break;
        }
        __builtin_amdgcn_s_sleep(kApp == SGN_TRAFFIC_TGEN ? 8 : 4);
      }
      while (ok) {
        bool good = true;
        if (mine) {
          const u64x2 x = ld_gran16(h, S.xsys != 0), y = ld_gran16(h + 2, S.xsys != 0);
          ga = xh_val(x.x, x.y);
          gb = xh_val(y.x, y.y);
          good = xh_ok(x.x, x.y, tag) && (2 * jj + 1 >= XH_N || xh_ok(y.x, y.y, tag));
        }
        if (__ballot(!good) == 0) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > kXWaitTicks) ok = false;
      }
      if (!ok) {
        if (lane == 0) atomicOr((unsigned int*)&C->overflow, OVF_TIMEOUT);
        return;
      }
      // (a system-scope acquire here: not built by default, see kXFenceAcq)
      if (kXFenceAcq && S.xsys) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      stamp(4, true);
      // the words into LDS (the event list's space, free between rounds): word k of sender q
      // at [k][q], read below as broadcasts (a shuffle per word and sender serialised ~200
      // cross-lane reads on the round's critical path)
      uint64_t* mw = (uint64_t*)X.lev;
      if (mine) {
        mw[(2 * jj) * XR_MAX + q] = ga;
        if (2 * jj + 1 < XH_N) mw[(2 * jj + 1) * XR_MAX + q] = gb;
      }
      __syncthreads();
    }
    // word k of sender q
    auto xw = [&](uint32_t k, uint32_t q) { return ((const uint64_t*)X.lev)[k * XR_MAX + q]; };
    uint64_t gm = INVALID, gmu = INVALID, xs = 0, xmax = 0;
    uint32_t spill_any = 0, nin_l = 0;
    uint64_t bin_l = 0;  // (lane q: runs sender q put in this shard's bins)
    for (uint32_t q = 0; q < R; q++) {
      const uint64_t a0 = xw(XH_MIN, q), a1 = xw(XH_MU, q), a2 = xw(XH_XSUM, q), a3 = xw(XH_XMAX, q);
      const uint64_t a4 = xw(XH_SPILL, q), a5 = xw(XH_CNT, q), a6 = xw(XH_TOT, q);
      gm = a0 < gm ? a0 : gm;
      gmu = a1 < gmu ? a1 : gmu;
      xs += a2;
      xmax = a3 > xmax ? a3 : xmax;
      spill_any |= a4 ? 1u : 0u;
      if (lane == q && q != me) {
        nin_l = (uint32_t)min(a5, (uint64_t)S.xislot);
        bin_l = a6 - a5;
      }
    }
    // Runahead::get (runahead.rs:44-57) over the global min used latency; the controller
    // (controller.rs:88-112) over the global min next event
    const uint64_t min_next = gm;  // (each message's minimum is already unwrapped: EMU_MAX = none)
    // (window_end's rule written out, as in rb_edge)
    uint64_t ra = (S.dynamic && gmu != INVALID) ? gmu : S.min_possible;
    ra = ra > S.runahead_cfg ? ra : S.runahead_cfg;
    uint64_t ne = min_next + ra;
    if (ne < min_next || ne > EMU_MAX) ne = EMU_MAX;
    ne = ne < S.end_time ? ne : S.end_time;
    const uint32_t active = min_next < ne ? 1u : 0u;
    // the next round's guards, evaluated for every shard from the messages alike (k_import's):
    // CoDel pages for the next window's due runs (occupancy plus everything exported this round,
    // a bound on what any shard receives), a re-layout after spills, the inbox slots
    uint32_t hflags = 0;
    uint64_t own_need = 0;
    if (active) {
      const uint32_t nbk = ((bucket_of(S, ne - 1) - bucket_of(S, min_next)) & (S.NB - 1)) + 1;
      for (uint32_t q = 0; q < R; q++) {
        const uint64_t occ = xw(XH_OCC, q) + xs, capb = (uint64_t)nbk * xw(XH_CAPB, q) + xs;
        const uint64_t need = codel_pages_bound(occ < capb ? occ : capb, xw(XH_NH, q));
        if (xw(XH_PFREE, q) < need) hflags |= HOLD_CODEL;
        if (q == me) own_need = need;
      }
      if (spill_any) hflags |= HOLD_SPILL;
      if (xmax > S.xislot) hflags |= HOLD_XSLOT;
      else if (2 * xmax > S.xislot) hflags |= HOLD_XGROW;
      // (min_next is the messages' minimum: every workgroup of every shard decides alike)
      if (min_next >= rs.pause_at) hflags |= HOLD_PAUSE;
    }
    // this shard's own round edge, from its message to itself
    const uint64_t e_nb1 = xw(XH_NB1, me), e_occd = xw(XH_OCCD, me), e_nalloc = xw(XH_NALLOC, me),
                   e_nfree = xw(XH_NFREE, me);
    uint32_t n_in = nin_l;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      n_in += __shfl_xor(n_in, off, 64);
      bin_l += shfl_xor64(bin_l, off);
    }
    // the idle-gap case of k_rounds: the bookkeeping now, and a local barrier before any send of
    // the next round can reach this round's bucket indices again
    // (a barrier that does not complete: the bare flag, as this kernel's other timeouts)
    const bool gap = gap_barrier(S, rs, w == wbk, P, ws, we, ks, active, ne, e_nb1,
                                 [&] { atomicOr((unsigned int*)&C->overflow, OVF_TIMEOUT); });
    if (lane < XR_MAX) rs.nin[lane] = nin_l;  // (lanes >= R hold 0)
    __syncthreads();
    const uint32_t b1 = bucket_of(S, we - 1);
    if (threadIdx.x == 0) {
      // (every import counts from here: slots and bins)
      round_state_advance(S, X, rs, true, b1, ws, we, ks, gap, e_nb1, min_next, ne, active, e_nfree, e_nalloc,
                          e_occd + n_in + bin_l);
      rs.n_in = n_in;
      rs.hold = hflags;
      rs.hold_need = own_need;
      rs.last = 0;
      if (w == wbk) {
        st_dev(&C->last_min_next, min_next);
        st_dev(&C->prev_we, we);
        if (gmu != INVALID) min_nr(&C->min_used, gmu);  // (the next rounds' messages carry it)
        // the largest per-peer count any shard produced (the host sizes the inbox slots by it)
        (void)__hip_atomic_fetch_max(&C->xhwm, xmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
    // ---- 5. the runs other shards sent this shard: a few are filed by their own workgroups at
    // the next round's start; many are shared out now and a second local barrier follows ----
    if (uni32(rs.n_in)) {
      if (uni32(rs.n_in) <= S.xown) {
        if (threadIdx.x == 0) {
          rs.fpend = 1;
          rs.fbuf = buf;
        }
        __syncthreads();
      } else {
        file_in(buf, hz_of(ws), uni64(rs.ws), uni64(rs.we), false);
        stamp(5, true);
        rb2_arrive<kApp>(S, p, w, P);
        if (!rb_wait<kApp>(&S.rb2_cnt[(size_t)p * RbLayout<kApp>::CB + RB_CH * RbLayout<kApp>::CS], nch)) {
          if (threadIdx.x == 0) atomicOr((unsigned int*)&C->overflow, OVF_TIMEOUT);
          return;
        }
        stamp(6, true);
        if (threadIdx.x == 0) X.big->spill_imp = ld_dev(&C->spill_n);  // (imports past their slab)
        __syncthreads();
      }
    }
    stamp(7, true);
  }
  // imports left for a next round this launch does not run: shared out now (the launch's end is
  // the barrier)
  if (uni32(rs.fpend)) file_in(rs.fbuf, hz_of(uni64(rs.pend_ws)), uni64(rs.ws), uni64(rs.we), false);
  // ... and the last round's bins of this workgroup's groups (file_in's rules: the launch's end
  // leaves every bin empty and every counter zero, whatever runs next)
  if (S.xin_bins) {
    const uint32_t ib = (uint32_t)((rounds0 + r) & 1);
    const uint64_t nws = uni64(rs.ws), nwe = uni64(rs.we), fhz = hz_of(uni64(rs.pend_ws));
    const uint32_t sb0 = bucket_of(S, nws), sbn = ((bucket_of(S, nwe - 1) - sb0) & (S.NB - 1)) + 1;
    uint32_t ln = threadIdx.x;
    asm volatile("" : "+v"(ln));
    const uint32_t bsh = R <= 2 ? 5u : R <= 4 ? 4u : 3u, E = 1u << bsh, q = ln >> bsh, e = ln & (E - 1);
    const bool on = q < R && q != me && e < S.xbk;
    bool spilled = false;
    for (uint32_t g = gq0; g < gq1; g += gqs) {
      SGN_GLB EvRec* bp = on ? S.xin_bins + (((size_t)ib * R + q) * S.G + g) * S.xbk + e : nullptr;
      bool more = on;
      for (uint32_t e0 = 0; e0 < S.xbk; e0 += E) {
        EvRec ev{};
        if (more) ev = S.xsys ? ld_sys_rec(bp + e0) : ld_dev_rec(bp + e0);
        const bool ok = more && ev.pc != 0;
        if (ok) {
          SGN_GLB uint64_t* pw = (SGN_GLB uint64_t*)(bp + e0) + 3;
          if (S.xsys) st_sys(pw, 0ull); else st_dev(pw, (uint64_t)0);
          if (file_run(S, X, C, ev, g, fhz, sb0, sbn)) spilled = true;
        }
        const uint64_t m = __ballot(ok && e == E - 1);
        if (!m) break;
        more = on && ((m >> (q * E + E - 1)) & 1ull) && e0 + E + e < S.xbk;
      }
    }
    bin_counters_reset(ib);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // (runs past their slab: the next launch's gathers read the spill area up to here)
    if (__ballot(spilled) && threadIdx.x == 0)
      (void)__hip_atomic_fetch_max(&C->spill_imp, ld_dev(&C->spill_n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  wacc_flush(S, X, gq0, gq1);
  // the last round's bookkeeping and the host-visible control block
  if (w == wbk) {
    if (rs.pend) rb_bookkeep(S, rs.pend_ws, rs.pend_we, rs.pend_nb1, rs.pend_new);
    if (threadIdx.x == 0) round_state_store(C, rs, rounds0 + r, &X.big->spill_imp);
  }
}

// Multi-shard round edge, after the exchange: the runs other shards sent this round into the
// local calendar, then the window advance from every shard's message. k_execute's last wave
// already did the local bucket bookkeeping, so every run goes to its bucket's current slab
// set (runs for the window's last bucket into the spare slab, like local sends).
// The advance (Controller::manager_finished_current_round, controller.rs:88-112, over the
// global {min next event, min used latency}: each message's minimum counts every pending
// event of its shard, exported runs included, so the min over messages is what an all-reduce
// would give) is done by the LAST block to finish: every block has read the window that just
// ran before it counts itself in, so no block sees the new one. One kernel per round edge.
__device__ __forceinline__ void advance_window(const DevSim& S, Ctrl* C) {
  uint64_t m = INVALID, mu = INVALID;
  for (uint32_t p = 0; p < S.n_ranks; p++) {
    const uint64_t* msg = (const uint64_t*)(S.xin + (size_t)p * (S.xslot + XHDR));
    const uint64_t a = msg[1], b = msg[2];
    m = a < m ? a : m;
    mu = b < mu ? b : mu;
    S.xout_n[p] = 0;  // the next round's sends count from zero
  }
  if (S.dynamic && mu != INVALID && mu < C->min_used) C->min_used = mu;
  const uint64_t min_next = m == INVALID ? EMU_MAX : m;
  C->last_min_next = min_next;
  const uint64_t ne = window_end(min_next, S.dynamic ? C->min_used : INVALID, S.dynamic, S.min_possible,
                                 S.runahead_cfg, S.end_time);
  C->active = min_next < ne ? 1u : 0u;
  C->prev_we = C->we;
  C->ws = min_next;
  C->we = ne;
  C->round_min = INVALID;
  C->rounds++;
}

__global__ __launch_bounds__(256) void k_import(DevSim S) {
  Ctrl* C = S.ctrl;
  // every block reads the same values: nothing changes them before all blocks count in
  if (!C->active || C->xspill || C->hold) return;
  // The send/recv moved the first C->xsz runs of each slot. If any shard had more for some
  // peer (the messages carry every shard's maximum), the round is held on every shard alike:
  // nothing is imported, the window stays, and the host completes the round with a
  // full-slot exchange and this kernel again (comm_complete_spill). Counts above the slot
  // itself are an overflow the sender already reported.
  uint64_t gm = 0;
  for (uint32_t r = 0; r < S.n_ranks; r++) {
    const uint64_t x = ((const uint64_t*)(S.xin + (size_t)r * (S.xslot + XHDR)))[3] & 0xFFFFFFFFull;
    gm = x > gm ? x : gm;
  }
  const uint32_t sz = C->xsz;
  // (gm > xslot: some shard spilled runs past a slot; the host grows the slots, then completes)
  const bool hold = gm > sz && (sz < S.xslot || gm > S.xslot);
  // the window that just ran (still C->ws): the same horizon as sends
  const uint64_t hz = SIM_START + (S.bw_div.div(C->ws - SIM_START) + S.NB) * S.BW;
  uint32_t filed = 0;
  for (uint32_t r = 0; r < S.n_ranks && !hold; r++) {
    if (r == S.rank) continue;
    const EvRec* blk = S.xin + (size_t)r * (S.xslot + XHDR);  // message, then the runs
    const uint32_t n = (uint32_t)min(((const uint64_t*)blk)[0], (uint64_t)S.xslot);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gridDim.x * blockDim.x) {
      const EvRec e = blk[XHDR + i];
      if (e.time >= hz) {
        if ((atomicOr(&C->overflow, OVF_HORIZON) & OVF_HORIZON) == 0) C->overflow_info = e.dst;
        continue;
      }
      const uint32_t b = bucket_of(S, e.time);
      const size_t idx = (size_t)S.bucket_slab[b] * S.G + ((e.dst - S.lo) >> S.gsh);
      const uint32_t pos = atomicAdd(&S.slab_n[idx], 1u);
      atomicMin((unsigned long long*)&S.bucket_min[b], (unsigned long long)e.time);
      if (pos < S.CAP)
        S.pool[idx * S.CAP + pos] = e;
      else  // the extension, or the spill area: the next round's gather reads it (lossless), and
            // the spill flag holds the round after that on every shard for the re-layout
        place_overflow(S, nullptr, (uint32_t)idx, pos, e);
      filed++;
    }
  }
  __shared__ uint32_t last, bfiled;
  if (threadIdx.x == 0) bfiled = 0;
  __syncthreads();
  if (filed) atomicAdd(&bfiled, filed);
  __syncthreads();  // this block's reads of C->ws are done
  if (threadIdx.x == 0) {
    if (bfiled) (void)atomicAdd((unsigned long long*)&C->cal_occ, (unsigned long long)bfiled);  // (completes first)
    last = atomicAdd(&C->imp_done, 1u) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!last || threadIdx.x != 0) return;
  C->imp_done = 0;
  // the spill-area entries the next round's gathers scan for runs imported past their slab
  C->spill_imp = ld_dev(&S.ctrl->spill_n);
  if (gm > C->xhwm) C->xhwm = gm;
  if (hold) {
    C->xspill = 1;
    return;
  }
  advance_window(S, C);
  if (!C->active) return;
  // the next round's guards, evaluated for EVERY shard from the messages alike (so all shards
  // hold the same round, or none): a shard's CoDel pages may not cover the next window's due
  // runs — its occupancy plus everything exported this round (a bound on what it received)
  // and at most its slabs of the window's buckets — or some shard spilled runs
  uint64_t xs = 0;
  for (uint32_t q = 0; q < S.n_ranks; q++) xs += ((const uint64_t*)(S.xin + (size_t)q * (S.xslot + XHDR)))[6];
  const uint32_t nbk = ((bucket_of(S, C->we - 1) - bucket_of(S, C->ws)) & (S.NB - 1)) + 1;
  uint32_t hflags = 0;
  uint64_t own = 0;
  for (uint32_t q = 0; q < S.n_ranks; q++) {
    const uint64_t* msg = (const uint64_t*)(S.xin + (size_t)q * (S.xslot + XHDR));
    // (msg[7]: the shard's runs per bucket, extensions included; imported runs may go past it)
    const uint64_t occ = msg[5] + xs, capb = (uint64_t)nbk * msg[7] + xs;
    const uint64_t need = codel_pages_bound(occ < capb ? occ : capb, S.rank_lo[q + 1] - S.rank_lo[q]);
    if (msg[4] < need) hflags |= HOLD_CODEL;
    if ((msg[3] >> 32) & 1) hflags |= HOLD_SPILL;
    if (q == S.rank) own = need;
  }
  // (sgn_shards_run_until: the window every shard just computed from the same messages)
  if (C->ws >= C->pause_at) hflags |= HOLD_PAUSE;
  if (hflags) {
    C->hold = hflags;
    C->hold_need = own;
  }
}

// CoDel control-law self test (f64 sqrt/div/round on the device vs the host).
__global__ void k_codel_law_test(uint64_t n, uint64_t* out) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = codel_law(SIM_START, i) - SIM_START;
}

// sgn_submit: each datagram becomes an event record of its source host in the calendar
// bucket of its send time (validated on the host: owned source, time within the horizon).
__global__ void k_inject(const DevSim* Sp, const EvRec* recs, uint32_t n) {
  const DevSim& S = *Sp;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const EvRec r = recs[i];
  const uint32_t g = (r.dst - S.lo) >> S.gsh;
  const uint32_t b = bucket_of(S, r.time);
  const size_t idx = (size_t)S.bucket_slab[b] * S.G + g;
  const uint32_t pos = atomicAdd(&S.slab_n[idx], 1u);
  atomicMin((unsigned long long*)&S.bucket_min[b], (unsigned long long)r.time);
  (void)atomicAdd((unsigned long long*)&S.ctrl->cal_occ, 1ULL);
  if (pos < S.CAP)
    S.pool[idx * S.CAP + pos] = r;
  else
    place_overflow(S, nullptr, (uint32_t)idx, pos, r);  // (a spill: sgn_submit re-lays out right after)
}

// Calendar re-layout (a held round edge after a spill, or sgn_submit): every slab's runs into
// the new layout — slabs of cap runs, and extensions (ext: offset | capacity << 40) for the hot
// ones — then the spilled runs after them. Order inside a slab is free (the gather sorts by
// Shadow's key); slab_n already counts every run of a slab, spilled ones included.
__device__ __forceinline__ EvRec* relayout_dst(EvRec* pool, uint32_t cap, const uint64_t* ext, EvRec* ext_pool,
                                               uint64_t idx, uint32_t j) {
  return j < cap ? pool + idx * cap + j : ext_pool + (ext[idx] & EXT_OFF_MASK) + (j - cap);
}
// the pool part of every slab (thread = (slab, position)); sets each slab's respill cursor
__global__ void k_relayout(const EvRec* __restrict__ old_pool, uint32_t old_cap, const uint64_t* __restrict__ old_ext,
                           EvRec* pool, uint32_t cap, const uint64_t* __restrict__ ext, EvRec* ext_pool,
                           const uint32_t* __restrict__ slab_n, uint32_t* cursor, uint64_t n_slabs) {
  const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t idx = t / old_cap;
  const uint32_t j = (uint32_t)(t % old_cap);
  if (idx >= n_slabs) return;
  const uint32_t fill = slab_n[idx];
  if (j < min(fill, old_cap)) *relayout_dst(pool, cap, ext, ext_pool, idx, j) = old_pool[idx * old_cap + j];
  if (j == 0) cursor[idx] = min(fill, old_cap + (old_ext ? (uint32_t)(old_ext[idx] >> 40) : 0u));
}
// the old extensions' runs (thread = (hot slab k of the list, position))
__global__ void k_relayout_ext(const uint64_t* __restrict__ hot, uint64_t n_hot, uint32_t max_ecap,
                               const EvRec* __restrict__ old_ext_pool, const uint64_t* __restrict__ old_ext,
                               uint32_t old_cap, EvRec* pool, uint32_t cap, const uint64_t* __restrict__ ext,
                               EvRec* ext_pool, const uint32_t* __restrict__ slab_n) {
  const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t k = t / max_ecap;
  const uint32_t j = (uint32_t)(t % max_ecap);
  if (k >= n_hot) return;
  const uint64_t idx = hot[k], x = old_ext[idx];
  const uint32_t fill = slab_n[idx];
  if (j < (uint32_t)(x >> 40) && old_cap + j < fill)
    *relayout_dst(pool, cap, ext, ext_pool, idx, old_cap + j) = old_ext_pool[(x & EXT_OFF_MASK) + j];
}
__global__ void k_respill(const EvRec* __restrict__ spill, const uint32_t* __restrict__ spill_idx, uint64_t n,
                          EvRec* pool, uint32_t cap, const uint64_t* __restrict__ ext, EvRec* ext_pool,
                          uint32_t* cursor, uint32_t* lost) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = spill_idx[i];
  if (idx & SPILL_PEER) return;  // a run for another shard (grow_exchange_slot), or one a gather took
  const uint32_t pos = atomicAdd(&cursor[idx], 1u);
  const uint32_t room = cap + (ext ? (uint32_t)(ext[idx] >> 40) : 0u);
  if (pos < room)
    *relayout_dst(pool, cap, ext, ext_pool, idx, pos) = spill[i];
  else  // the host sized every slab for its fill (room >= fill): a violation is an error, never
        // a silent loss (relayout_calendar reads this count)
    atomicAdd(lost, 1u);
}

// sgn_rng_*: draws of host Xoshiro256++ streams (the state stays on the device). One thread
// per requested host (hosts distinct, checked on the host): its count[i] draws go to
// out[off[i] ..), in stream order.
__global__ void k_rng(const DevSim* Sp, const uint32_t* hosts, const uint32_t* count,
                      const uint64_t* off, uint32_t n, uint64_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  SGN_GLB HostRec* R = Sp->hrec + hosts[i];
  // (the state's two chunks: in the tiles, or in the record's hot line)
  SGN_GLB uint64_t* rg0 = Sp->htile ? Sp->htile + 2 * hot_idx(hosts[i], 0) : &R->rng[0];
  SGN_GLB uint64_t* rg1 = Sp->htile ? Sp->htile + 2 * hot_idx(hosts[i], 1) : &R->rng[2];
  uint64_t s0 = rg0[0], s1 = rg0[1], s2 = rg1[0], s3 = rg1[1];
  uint64_t* o = out + off[i];
  for (uint32_t k = 0; k < count[i]; k++) {
    o[k] = rotl64(s0 + s3, 23) + s0;
    const uint64_t t = s1 << 17;
    s2 ^= s0;
    s3 ^= s1;
    s1 ^= s2;
    s0 ^= s3;
    s2 ^= t;
    s3 = rotl64(s3, 45);
  }
  rg0[0] = s0;
  rg0[1] = s1;
  rg1[0] = s2;
  rg1[1] = s3;
  R->rng_pos += count[i];
}

// CPU-held host RNG states back into the records (sgn_rng_* single draws): per entry
// {slot, s0..s3, draws}; the stream position advances by the draws made on the CPU
__global__ void k_rng_set(const DevSim* Sp, const uint64_t* st, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* e = st + 6 * (size_t)i;
  SGN_GLB HostRec* R = Sp->hrec + (uint32_t)e[0];
  SGN_GLB uint64_t* rg0 = Sp->htile ? Sp->htile + 2 * hot_idx((uint32_t)e[0], 0) : &R->rng[0];
  SGN_GLB uint64_t* rg1 = Sp->htile ? Sp->htile + 2 * hot_idx((uint32_t)e[0], 1) : &R->rng[2];
  rg0[0] = e[1];
  rg0[1] = e[2];
  rg1[0] = e[3];
  rg1[1] = e[4];
  R->rng_pos += e[5];
}

// Host::next_event_time (host.rs:832-834) for the owned HostIds [lo, lo + n), between rounds:
// the earliest local event (the host record's slots) ...
__global__ void k_next_local(const DevSim* Sp, uint32_t lo, uint32_t n, uint64_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = Sp->sid_of[lo + i] - Sp->lo;
  const HostRec& r = Sp->hrec[slot];
  const uint64_t m0 = Sp->htile ? Sp->htile[2 * hot_idx(slot, 2) + 1] : r.st2;                   // st2
  const uint32_t flg = Sp->htile ? (uint32_t)Sp->htile[2 * hot_idx(slot, 7) + 1] : r.flags;     // flags
  uint64_t m = m0;
  if (Sp->tkind != SGN_TRAFFIC_PERIODIC || (flg & F_COLD)) {  // (else both relays idle)
    m = r.st0 < m ? r.st0 : m;
    m = r.st1 < m ? r.st1 : m;
  }
  out[i] = m;
}
// ... and the earliest pending packet event: one wave per (bucket, host group) slab,
// atomicMin into the destination's slot of out when it is in the range. Between rounds every
// pending event is in a bucket's slab (the spare slab set is empty).
__global__ void k_next_packet(const DevSim* Sp, uint32_t lo, uint32_t n, uint32_t g0, uint32_t ng,
                              uint64_t* out) {
  const DevSim& S = *Sp;
  const uint32_t w = blockIdx.x;  // (bucket, group) pair
  const uint32_t b = w / ng, g = g0 + w % ng;
  const size_t idx = (size_t)S.bucket_slab[b] * S.G + g;
  const uint32_t fill = S.slab_n[idx];
  const uint64_t x = S.ext && fill > S.CAP ? S.ext[idx] : 0ULL;
  const uint32_t np = min(fill, S.CAP), ne = min(fill - np, (uint32_t)(x >> 40));
  for (uint32_t j = threadIdx.x; j < np + ne; j += blockDim.x) {
    const EvRec& e = j < np ? S.pool[idx * S.CAP + j] : S.ext_pool[(x & EXT_OFF_MASK) + j - np];
    const uint32_t d = S.host_of[e.dst - S.lo];
    if (d >= lo && d < lo + n) atomicMin((unsigned long long*)&out[d - lo], (unsigned long long)e.time);
  }
}

}  // namespace sgn

// ====================================================================================
// Launch surface: the only host code of this translation unit (declared in sgn_internal.h).
// The host half lives in sim_init.cpp, run.cpp, pools.cpp and interop.cpp; it reaches the
// kernels through the table and the launch functions below and nothing else.
// ====================================================================================
namespace sgn {

namespace {
// The table, by traffic kind (index 0 TGEN, 1 EXTERNAL, 2 PERIODIC). Filling it is what instantiates
// the 21 templated round kernels, and the compiler emits them in the order they are first named:
// the entries are written out in the order these names had in the launch ladders that stood here,
// so the code object keeps its kernel order (profiles/r09 suspected code placement behind a 0.3 %
// shift on config D).
struct RoundKernelTable {
  RoundKernels k[3];
  RoundKernelTable() {
    constexpr uint32_t T = SGN_TRAFFIC_TGEN, E = SGN_TRAFFIC_EXTERNAL, P = SGN_TRAFFIC_PERIODIC;
    typedef const void* F;
    k[0].execute[1] = (F)k_execute<true, T>, k[1].execute[1] = (F)k_execute<true, E>, k[2].execute[1] = (F)k_execute<true, P>;
    k[0].execute[0] = (F)k_execute<false, T>, k[1].execute[0] = (F)k_execute<false, E>, k[2].execute[0] = (F)k_execute<false, P>;
    k[0].rounds[1][1] = (F)k_rounds_diag<T, true>, k[1].rounds[1][1] = (F)k_rounds_diag<E, true>, k[2].rounds[1][1] = (F)k_rounds_diag<P, true>;
    k[0].rounds[0][1] = (F)k_rounds<T, true>, k[1].rounds[0][1] = (F)k_rounds<E, true>, k[2].rounds[0][1] = (F)k_rounds<P, true>;
    k[0].rounds[1][0] = (F)k_rounds_diag<T, false>, k[1].rounds[1][0] = (F)k_rounds_diag<E, false>, k[2].rounds[1][0] = (F)k_rounds_diag<P, false>;
    k[0].rounds[0][0] = (F)k_rounds<T, false>, k[1].rounds[0][0] = (F)k_rounds<E, false>, k[2].rounds[0][0] = (F)k_rounds<P, false>;
    k[0].rounds_x = (F)k_rounds_x<T>, k[1].rounds_x = (F)k_rounds_x<E>, k[2].rounds_x = (F)k_rounds_x<P>;
  }
};
}  // namespace

const RoundKernels& round_kernels(uint32_t tkind) {
  static const RoundKernelTable t;
  return t.k[tkind == SGN_TRAFFIC_TGEN ? 0 : tkind == SGN_TRAFFIC_EXTERNAL ? 1 : 2];
}
const void* import_kernel() { return (const void*)k_import; }

void launch_k_import(hipStream_t st, const DevSim& S) {
  hipLaunchKernelGGL(k_import, dim3(kImportBlocks), dim3(256), 0, st, S);
}
void launch_k_inject(hipStream_t st, const DevSim* Sp, const EvRec* recs, uint32_t n) {
  hipLaunchKernelGGL(k_inject, dim3((n + 255) / 256), dim3(256), 0, st, Sp, recs, n);
}
void launch_k_relayout(hipStream_t st, const EvRec* old_pool, uint32_t old_cap, const uint64_t* old_ext, EvRec* pool,
                       uint32_t cap, const uint64_t* ext, EvRec* ext_pool, const uint32_t* slab_n, uint32_t* cursor,
                       uint64_t n_slabs) {
  const uint64_t nt = n_slabs * old_cap;  // thread = (slab, position)
  hipLaunchKernelGGL(k_relayout, dim3((uint32_t)((nt + 255) / 256)), dim3(256), 0, st, old_pool, old_cap, old_ext, pool,
                     cap, ext, ext_pool, slab_n, cursor, n_slabs);
}
void launch_k_relayout_ext(hipStream_t st, const uint64_t* hot, uint64_t n_hot, uint32_t max_ecap,
                           const EvRec* old_ext_pool, const uint64_t* old_ext, uint32_t old_cap, EvRec* pool,
                           uint32_t cap, const uint64_t* ext, EvRec* ext_pool, const uint32_t* slab_n) {
  const uint64_t ne = n_hot * max_ecap;  // thread = (hot slab of the list, position)
  hipLaunchKernelGGL(k_relayout_ext, dim3((uint32_t)((ne + 255) / 256)), dim3(256), 0, st, hot, n_hot, max_ecap,
                     old_ext_pool, old_ext, old_cap, pool, cap, ext, ext_pool, slab_n);
}
void launch_k_respill(hipStream_t st, const EvRec* spill, const uint32_t* spill_idx, uint64_t n, EvRec* pool,
                      uint32_t cap, const uint64_t* ext, EvRec* ext_pool, uint32_t* cursor, uint32_t* lost) {
  hipLaunchKernelGGL(k_respill, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, spill, spill_idx, n, pool, cap, ext,
                     ext_pool, cursor, lost);
}
void launch_k_rng(hipStream_t st, const DevSim* Sp, const uint32_t* hosts, const uint32_t* count, const uint64_t* off,
                  uint32_t n, uint64_t* out) {
  hipLaunchKernelGGL(k_rng, dim3((n + 63) / 64), dim3(64), 0, st, Sp, hosts, count, off, n, out);
}
void launch_k_rng_set(hipStream_t st, const DevSim* Sp, const uint64_t* states, uint32_t n) {
  hipLaunchKernelGGL(k_rng_set, dim3((n + 63) / 64), dim3(64), 0, st, Sp, states, n);
}
void launch_k_next_local(hipStream_t st, const DevSim* Sp, uint32_t lo, uint32_t n, uint64_t* out) {
  hipLaunchKernelGGL(k_next_local, dim3((n + 255) / 256), dim3(256), 0, st, Sp, lo, n, out);
}
void launch_k_next_packet(hipStream_t st, uint32_t n_buckets, const DevSim* Sp, uint32_t lo, uint32_t n, uint32_t g0,
                          uint32_t ng, uint64_t* out) {
  hipLaunchKernelGGL(k_next_packet, dim3(n_buckets * ng), dim3(64), 0, st, Sp, lo, n, g0, ng, out);
}
void launch_k_codel_law_test(hipStream_t st, uint64_t n, uint64_t* out) {
  hipLaunchKernelGGL(k_codel_law_test, dim3(1024), dim3(256), 0, st, n, out);
}

uint64_t layout_sig_engine() { return kLayoutSig; }

}  // namespace sgn
