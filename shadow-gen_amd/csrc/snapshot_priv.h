// snapshot_priv.h — what snapshot.hip (save, restore) and snapshot_file.hip (export, import)
// share: the snapshot object, the description of what one holds, and the few helpers that build,
// check and release one.
//
// WHAT A SNAPSHOT HOLDS is said here once per kind of item; save, restore, release, info, export
// and import walk these and name no item themselves. New simulation state goes into one of them:
//   state_buffers()   the device buffers that never move or change size after sgn_sim_init
//   for_each_pool()   the device pools that grow (their sizes follow the layout scalars)
//   SnapLayout        the layout scalars a restore reads
//   sgn::SimCounters  the host-side counters (sgn_internal.h)
// and, named members of sgn_snapshot: the packed calendar, the trace records and the host vectors.
#pragma once

#include <array>
#include <string>
#include <type_traits>
#include <vector>

#include "sgn_internal.h"

namespace sgn {

// the layout scalars a restore reads, as a snapshot file's header carries them (every field a u64)
struct SnapLayout {
  uint64_t cap, cq_pages, spill_cap, ext_total, gspec;
};
inline SnapLayout layout_of(const DevSim& S) { return {S.CAP, S.cq_pages, S.spill_cap, S.ext_total, S.gspec}; }

// a device section: its name (snapshot files, messages), where it lives in a DevSim, its size
struct StateBuf {
  const char* name;
  void* p;
  size_t bytes;
};

// The pools that grow, in file order: f(index, name, the pointer member of S, bytes). The sizes are
// those of layout L holding n_spill spilled runs and n_drain undrained records — a snapshot's
// sections with the record counts at the save, the pools themselves with n_spill = L.spill_cap.
// (S may be const: f reads the member; or not: f may set it.)
enum : uint32_t { POOL_CODEL = 0, POOL_CQ_NEXT, POOL_CQ_FREE, POOL_SPILL, POOL_SPILL_IDX, POOL_DRAIN, POOL_N };
template <typename Sim, typename F>
void for_each_pool(Sim& S, const SnapLayout& L, uint64_t n_spill, uint64_t n_drain, F&& f) {
  f(POOL_CODEL, "codel", S.codel, (size_t)(L.cq_pages * CQ_PAGE * sizeof(CodelEnt)));
  f(POOL_CQ_NEXT, "cq_next", S.cq_next, (size_t)(L.cq_pages * 4));
  f(POOL_CQ_FREE, "cq_free", S.cq_free, (size_t)(L.cq_pages * 4));
  f(POOL_SPILL, "spill", S.spill, (size_t)(n_spill * sizeof(EvRec)));
  f(POOL_SPILL_IDX, "spill_idx", S.spill_idx, (size_t)(n_spill * 4));
  f(POOL_DRAIN, "drain", S.drain, (size_t)(n_drain * sizeof(sgn_drain_rec)));  // undrained records [0, drain_n)
}
inline std::array<StateBuf, POOL_N> pool_buffers(const DevSim& S, const SnapLayout& L, uint64_t n_spill, uint64_t n_drain) {
  std::array<StateBuf, POOL_N> v{};
  for_each_pool(S, L, n_spill, n_drain,
                [&](uint32_t k, const char* name, const auto& member, size_t bytes) { v[k] = {name, (void*)member, bytes}; });
  return v;
}

// The mutable buffers of DevSim that never move or change size after sgn_sim_init, in file order
// (null: this simulation has none)
std::vector<StateBuf> state_buffers(const DevSim& S);

}  // namespace sgn

struct sgn_snapshot {
  sgn_ctx* ctx = nullptr;
  uint64_t gen = 0;
  sgn::SnapLayout lay{};  // the layout at save (an imported snapshot: the file's)
  sgn::Ctrl ctrl{};       // the control block at save
  struct Buf {
    void* d = nullptr;
    size_t bytes = 0;
  };
  std::vector<Buf> fixed;    // state_buffers() order
  Buf pool[sgn::POOL_N];     // for_each_pool() order
  Buf packed;                // the calendar's runs
  Buf trace;                 // imported snapshots only: trace records [trace_b, trace_n)
                             // (sgn_snapshot_save leaves it empty: in its own
                             // context the records are still in the trace buffer)
  bool imported = false;     // built by sgn_snapshot_import
  uint64_t trace_b = 0;      // imported: records sgn_trace_take had handed out
                             // before the export (the file's first record)
  uint64_t runs = 0;
  // host-side simulation state
  sgn::SimCounters counters{};
  std::vector<uint64_t> handles;
  std::vector<uint32_t> submit_seq;
  std::vector<sgn_drain_rec> drain_held;
  std::vector<uint64_t> h_ext;  // (restored only with the re-layout)
  sgn_snapshot_info info{};
};

namespace sgn {

// s->fixed[k] of the state buffer at p in S (save and import fill fixed in state_buffers() order)
const sgn_snapshot::Buf* snap_fixed(const sgn_snapshot* s, const DevSim& S, const void* p);

bool snap_buf_alloc(sgn_snapshot::Buf* b, size_t bytes);
void snap_release(sgn_snapshot* s);
// fills s->info's sizes from the snapshot's buffers and vectors (not the times)
void snap_fill_info(sgn_snapshot* s, uint64_t n_slabs);
// what a restore — and an export — checks before it touches anything (what: the entry point's name)
int snap_check(sgn_ctx* ctx, const sgn_snapshot* snap, const char* what, sgn_snapshot** s_out);
// the calendar scan over device fills slab_n and extensions ext (null: none): the runs a packed
// section for them holds (synchronous on the context's stream)
int snap_scan_total(sgn_ctx* ctx, const uint32_t* slab_n, const uint64_t* ext, uint32_t cap, uint64_t n_slabs,
                    uint64_t* total);

}  // namespace sgn
