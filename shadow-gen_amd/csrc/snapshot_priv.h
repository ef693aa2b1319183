// snapshot_priv.h — what snapshot.hip (save, restore) and snapshot_file.hip (export, import)
// share: the snapshot object and the few helpers that build, check and release one.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "sgn_internal.h"

struct sgn_snapshot {
  sgn_ctx* ctx = nullptr;
  uint64_t gen = 0;
  sgn::DevSim S{};   // the layout at save: CAP, cq_pages, spill_cap, ext_total, gspec (its pointers are
                     // the buffers of that time and are never followed; an imported snapshot carries
                     // the importing context's DevSim with those five scalars from the file)
  sgn::Ctrl ctrl{};  // the control block at save
  struct Buf {
    void* d = nullptr;
    size_t bytes = 0;
  };
  std::vector<Buf> fixed;                         // state_buffers() order
  Buf codel, cq_next, cq_free, spill, spill_idx;  // the pools that grow
  Buf drain;                                      // undrained records [0, drain_n)
  Buf packed;                                     // the calendar's runs
  Buf trace;                                      // imported snapshots only: trace records [trace_b, trace_n)
                                                  // (sgn_snapshot_save leaves it empty: in its own
                                                  // context the records are still in the trace buffer)
  bool imported = false;                          // built by sgn_snapshot_import
  uint64_t trace_b = 0;                           // imported: records sgn_trace_take had handed out
                                                  // before the export (the file's first record)
  uint64_t runs = 0;
  // host-side simulation state
  uint64_t rounds_enqueued = 0;
  std::vector<uint64_t> handles;
  std::vector<uint32_t> submit_seq;
  std::vector<sgn_drain_rec> drain_held;
  std::vector<uint64_t> h_ext;
  uint64_t codel_grows = 0, cal_grows = 0, cal_spill_runs = 0, ext_slabs = 0, spill_grows = 0, rounds_held = 0,
           codel_allocs_before = 0;
  sgn_snapshot_info info{};
};

namespace sgn {

// The mutable buffers of DevSim that never move or change size after sgn_sim_init, in a fixed
// order (null: this simulation has none), and their names in that order (snapshot files, messages)
std::vector<std::pair<void*, size_t>> state_buffers(const DevSim& S);
extern const char* const kStateBufferNames[];
constexpr size_t kStateSlabN = 9;  // state_buffers()[kStateSlabN] is slab_n

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
