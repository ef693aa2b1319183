// snapshot_file.hip — snapshot files: sgn_snapshot_export / _import, the section digest kernel and
// the simulation's identity digest.
//
// A snapshot's state is pointer-free ("Snapshot files"), so a file is format, validation
// and integrity. Layout, little-endian, every payload padded to 16 bytes:
//   FileHeader | TableEnt[n_sections] | payloads in table order | trailer: digest(header + table)
// Export is one forward pass (the callbacks never seek): the device sections are digested by ONE
// launch of k_digest from the snapshot's own buffers, then streamed device -> pinned chunk ->
// callback through two chunks, the copy of one overlapping the write of the other. Import reads
// the same way into fresh device buffers, digests them again on the device after the upload, runs
// the calendar scan over the imported fills, and only then hands out a snapshot. The file is
// INPUT: every size is derived from the importing simulation and the header's layout scalars
// before anything is allocated, and nothing in it is used as an index before it has been bounded.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "snapshot_priv.h"
// (after the HIP runtime header above: its function qualifiers)
#include "report_common.h"  // (ms_since)
#include "sgn_workload.h"

using namespace sgn;
using sgn::report::ms_since;

// ---- device side ----------------------------------------------------------------------------
namespace {

constexpr uint64_t kGold = 0x9e3779b97f4a7c15ULL;
constexpr uint32_t kDigThreads = 256;    // four waves per workgroup
constexpr uint32_t kDigUnroll = 4;       // independent 16-byte loads in flight per lane and iteration
constexpr uint32_t kDigMaxBlocks = 2048; // per section: 8 workgroups per CU, the rest is grid-stride
constexpr uint32_t kDigPasses = 4;       // a section below the cap gets as many workgroups as walk it this often
constexpr uint32_t kDigSlots = 32;       // result words per section, one 128-byte line each
constexpr uint32_t kDigSlotWords = 16;   // (u64 words per line)

struct DigSec {
  const void* p;    // 16-byte aligned (null: bytes == 0)
  uint64_t bytes;   // % 4 == 0
  uint32_t first;   // the section's workgroups are [first, first + blocks) of the grid
  uint32_t blocks;  // >= 1
};

// the two words of 16-byte unit u: key = kGold * (2u + 1) is word 2u's, word 2u + 1's is one more
__device__ __forceinline__ uint64_t dig_unit(const uint4 v, uint64_t key) {
  const uint64_t w0 = (uint64_t)v.x | ((uint64_t)v.y << 32), w1 = (uint64_t)v.z | ((uint64_t)v.w << 32);
  return sgn_mix64(w0 ^ key) + sgn_mix64(w1 ^ (key + kGold));
}

// One launch digests every section: section y owns the workgroups [first, first + blocks) of a
// flat grid — a grid row of its own length, so a small section costs one workgroup and not a row
// as wide as the largest — and the result words out[y][0 .. kDigSlots) (zeroed), whose sum is its
// digest. The terms are keyed by position and summed, so lanes, waves and workgroups add theirs in
// any order: a lane accumulates over a grid-stride walk of 16-byte units, the wave folds its 64
// accumulators with shuffles, and one 64-bit atomic add per wave lands in the slot its workgroup
// number picks. The slots are a cache line apart, so thousands of waves do not add to one word, or
// to neighbouring sections' words in one line (DESIGN.md §7a has the launch this one replaced).
// Read-only streaming: the loads of an iteration are issued together, nothing else is written.
__global__ __launch_bounds__(kDigThreads) void k_digest(const DigSec* __restrict__ secs, uint32_t n_secs,
                                                        uint64_t* __restrict__ out) {
  // the section of this workgroup: the last one that starts at or before it (uniform: scalar loads)
  uint32_t y = 0;
  for (uint32_t lo = 0, hi = n_secs; hi - lo > 1;) {
    const uint32_t mid = (lo + hi) >> 1;
    if (secs[mid].first <= blockIdx.x) lo = mid; else hi = mid;
    y = lo;
  }
  const DigSec sc = secs[y];
  const uint32_t bx = blockIdx.x - sc.first;
  const uint64_t n16 = sc.bytes >> 4;
  const uint64_t stride = (uint64_t)sc.blocks * kDigThreads;
  const uint64_t t = (uint64_t)bx * kDigThreads + threadIdx.x;
  // (the pointer comes from memory: say that it is global memory, or the loads are flat_load)
  const SGN_GLB uint4* __restrict__ p = (const SGN_GLB uint4*)sc.p;
  const uint64_t dkey = kGold * 2 * stride;
  uint64_t key = kGold * (2 * t + 1);
  uint64_t acc = 0;
  uint64_t u = t;
  for (; u + (kDigUnroll - 1) * stride < n16; u += kDigUnroll * stride) {
    uint4 v[kDigUnroll];
#pragma unroll
    for (uint32_t k = 0; k < kDigUnroll; k++) v[k] = p[u + k * stride];
#pragma unroll
    for (uint32_t k = 0; k < kDigUnroll; k++) {
      acc += dig_unit(v[k], key);
      key += dkey;
    }
  }
  for (; u < n16; u += stride) {
    acc += dig_unit(p[u], key);
    key += dkey;
  }
  if (t == 0) {  // the length term and the 4 / 8 / 12-byte tail
    acc += sgn_mix64(sc.bytes ^ SGN_DIGEST_SEED);
    const uint32_t tail = (uint32_t)(sc.bytes & 15);
    const SGN_GLB uint32_t* q = (const SGN_GLB uint32_t*)sc.p + 4 * n16;
    uint64_t j = 2 * n16;
    if (tail >= 8) {
      acc += sgn_mix64(((uint64_t)q[0] | ((uint64_t)q[1] << 32)) ^ (kGold * (j + 1)));
      j++;
      q += 2;
    }
    if (tail & 4) acc += sgn_mix64((uint64_t)q[0] ^ (kGold * (j + 1)));
  }
#pragma unroll
  for (int m = 32; m; m >>= 1) acc += __shfl_xor(acc, m);
  if ((threadIdx.x & 63) == 0 && acc)
    atomicAdd((unsigned long long*)&out[((size_t)y * kDigSlots + bx % kDigSlots) * kDigSlotWords], (unsigned long long)acc);
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------
namespace {

using Buf = sgn_snapshot::Buf;
using Clock = std::chrono::steady_clock;

constexpr size_t kChunk = 4u << 20;  // one pinned staging chunk (two per context)
constexpr uint64_t kFormat = 1;
const char kMagic[8] = {'S', 'G', 'N', 'S', 'N', 'A', 'P', '1'};

// Every field a u64, so the header has no padding and reads the same from any compiler.
struct FileHeader {
  char magic[8];
  uint64_t format, abi, layout_sig;
  uint64_t sz_ctrl, sz_hostrec, sz_evrec, sz_codelent, sz_fifoent, sz_drain_rec, sz_trace_rec;
  uint64_t identity;
  uint64_t shard_rank, shard_count;
  uint64_t rounds, ws, we;
  SnapLayout lay;        // the layout scalars a restore reads
  uint64_t traced;       // the simulation keeps a trace
  SimCounters counters;  // the host-side counters of sgn_snapshot
  uint64_t calendar_runs, trace_records;
  uint64_t n_sections, file_bytes;
  uint64_t reserved;  // the trace records sgn_trace_take had handed out before the export: the
                      // section holds the records from this one on (0 without a take: the spare
                      // word that keeps the header a multiple of 16 bytes)
};
static_assert(sizeof(FileHeader) % 16 == 0, "the table and the payloads start 16-byte aligned");
// format 1, to the byte: 8 bytes of magic, then 35 u64 (a field added to SnapLayout or SimCounters
// moves what follows it: that is a new kFormat)
static_assert(sizeof(FileHeader) == 288 && offsetof(FileHeader, lay) == 136 && offsetof(FileHeader, traced) == 176 &&
                  offsetof(FileHeader, counters) == 184 && offsetof(FileHeader, calendar_runs) == 248 &&
                  offsetof(FileHeader, n_sections) == 264 && offsetof(FileHeader, reserved) == 280,
              "FileHeader is not the header of format 1");
struct TableEnt {
  uint64_t id, bytes, digest;
};

// The sections, in file order; id = index + 1.
enum : uint32_t {
  SEC_CTRL = 0,
  SEC_FIXED = 1,  // one per state_buffers() entry, then one per for_each_pool() entry, and from there:
  SECT_PACKED = 0, SECT_HANDLES, SECT_SUBMIT_SEQ, SECT_DRAIN_HELD, SECT_H_EXT, SECT_TRACE, SECT_N
};
const char* const kTailNames[SECT_N] = {"calendar", "handles", "submit_seq", "drain_held", "h_ext", "trace"};
struct Sec {
  std::string name;
  bool dev = false;       // device memory (digested by k_digest), else host memory
  const void* p = nullptr;
  uint64_t bytes = 0;
};
inline uint64_t pad16(uint64_t n) { return (n + 15) & ~(uint64_t)15; }

// the pinned staging chunks (kept by the context: pinning is slow)
int stage_get(sgn_ctx* ctx) {
  for (void*& p : ctx->file_stage)
    if (!p && hipHostMalloc(&p, kChunk, 0) != hipSuccess) {
      p = nullptr;
      return set_error(ctx, SGN_ENOMEM, "pinned staging chunk allocation failed (snapshot file)");
    }
  return 0;
}

// a section for k_digest (the launcher fills first / blocks)
inline DigSec dsec(const void* p, uint64_t bytes) { return DigSec{p, bytes, 0u, 1u}; }

// k_digest over device sections; out[i] their digests. Synchronous on the context's stream.
int digest_device(sgn_ctx* ctx, std::vector<DigSec> secs, uint64_t* out, float* ms = nullptr) {
  if (secs.empty()) return 0;
  const size_t n = secs.size();
  const uint64_t per_pass = (uint64_t)kDigThreads * kDigUnroll * kDigPasses;
  uint32_t total = 0;
  for (DigSec& s : secs) {
    if (s.bytes % 4 || (s.bytes && (!s.p || ((uintptr_t)s.p & 15))))
      return set_error(ctx, SGN_EINVAL, "digest: a section is not 16-byte aligned or not a multiple of 4 bytes");
    s.first = total;
    s.blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kDigMaxBlocks, ((s.bytes >> 4) + per_pass - 1) / per_pass));
    total += s.blocks;
  }
  const size_t out_words = n * kDigSlots * kDigSlotWords;
  void* d = nullptr;  // the result slots, then the table
  if (hipMalloc(&d, out_words * 8 + n * sizeof(DigSec)) != hipSuccess) return set_error(ctx, SGN_ENOMEM, "device allocation failed (digest)");
  uint64_t* d_out = (uint64_t*)d;
  DigSec* d_secs = (DigSec*)(d_out + out_words);
  std::vector<uint64_t> h_out(out_words);
  hipStream_t st = ctx->stream;
  report::ReportEvents<2> ev;
  bool ok = hipMemcpyAsync(d_secs, secs.data(), n * sizeof(DigSec), hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemsetAsync(d_out, 0, out_words * 8, st) == hipSuccess;
  if (ok && ms) ok = ev.make() && hipEventRecord(ev[0], st) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_digest, dim3(total), dim3(kDigThreads), 0, st, (const DigSec*)d_secs, (uint32_t)n, d_out);
    ok = hipGetLastError() == hipSuccess;
  }
  if (ok && ms) ok = hipEventRecord(ev[1], st) == hipSuccess;
  ok = ok && hipMemcpyAsync(h_out.data(), d_out, out_words * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
  ok = hipStreamSynchronize(st) == hipSuccess && ok;
  if (ok && ms) *ms = report::elapsed_ms(ev[0], ev[1]);
  (void)hipFree(d);
  if (!ok) return set_error(ctx, SGN_EDEVICE, "the digest kernel failed");
  for (size_t i = 0; i < n; i++) {
    uint64_t sum = 0;
    for (uint32_t k = 0; k < kDigSlots; k++) sum += h_out[(i * kDigSlots + k) * kDigSlotWords];
    out[i] = sum;
  }
  return 0;
}

// ---- identity: what a simulation is made from ----
// Field by field where a struct has padding or reserved words (sgn_sim_config, sgn_traffic); whole
// buffers where every byte follows from the inputs (the route tables; HostConst, whose pad word
// sgn_sim_init zeroes). The device-resident constants are digested where they live.
int identity(sgn_ctx* ctx, uint64_t* out) {
  if (ctx->identity_gen == ctx->sim_gen) {
    *out = ctx->identity;
    return 0;
  }
  const DevSim& S = ctx->S;
  const size_t UU = (size_t)S.U * S.U, N = S.n_all;
  const std::vector<DigSec> dev = {
      dsec(ctx->d_lat, UU * 8),                         // the route table as built ...
      dsec(ctx->d_loss, UU * 4),
      dsec((const void*)S.route, UU * sizeof(RouteEnt)),  // ... and as the packet path reads it
      dsec((const void*)S.hconst, (size_t)S.nH * sizeof(HostConst)),  // owned hosts: id, address, node, refills
      dsec((const void*)S.unode, N * 4),
      dsec((const void*)S.ip, N * 4),
      dsec((const void*)S.sid_of, N * 4),               // every shard's host placement
      dsec((const void*)S.host_of, (size_t)S.nH * 4),
      dsec((const void*)S.servers, S.servers ? (size_t)S.n_servers * 4 : 0),
      dsec((const void*)S.rank_lo, ((size_t)S.n_ranks + 1) * 4),
  };
  std::vector<uint64_t> v(dev.size());
  if (int rc = digest_device(ctx, dev, v.data())) return rc;
  // every host's constants as registered (all shards hold the full list)
  v.push_back(sgn_digest_bytes(ctx->node_id.data(), ctx->node_id.size() * 4));
  v.push_back(sgn_digest_bytes(ctx->bw_up.data(), ctx->bw_up.size() * 8));
  v.push_back(sgn_digest_bytes(ctx->bw_down.data(), ctx->bw_down.size() * 8));
  v.push_back(sgn_digest_bytes(ctx->seed.data(), ctx->seed.size() * 8));
  v.push_back(sgn_digest_bytes(ctx->used_ids.data(), ctx->used_ids.size() * 4));
  const sgn_sim_config& c = ctx->sim_cfg;
  const sgn_traffic& t = ctx->sim_tr;
  for (uint64_t x : {c.stop_time_ns, c.bootstrap_end_ns, c.runahead_ns, (uint64_t)(uint32_t)c.use_dynamic_runahead,
                     (uint64_t)c.out_fifo_cap, (uint64_t)c.codel_cap, (uint64_t)c.hosts_per_wave, c.event_capacity,
                     (uint64_t)c.interface_qdisc})
    v.push_back(x);
  for (uint64_t x : {(uint64_t)t.kind, (uint64_t)t.payload_len, t.flow_seed, t.start_ns, t.start_jitter_ns, t.period_ns,
                     t.period_jitter_ns, (uint64_t)t.unknown_dst_permille, (uint64_t)t.req_payload, (uint64_t)t.n_servers,
                     t.file_bytes[0], t.file_bytes[1], t.file_bytes[2]})
    v.push_back(x);
  // the shard and the calendar's derived shape
  for (uint64_t x : {(uint64_t)ctx->rank, (uint64_t)ctx->nranks, (uint64_t)ctx->lo, (uint64_t)ctx->hi, (uint64_t)S.n_all,
                     (uint64_t)S.U, (uint64_t)S.NB, S.BW, (uint64_t)S.G, (uint64_t)S.gsh, (uint64_t)S.fifo_cap, S.drain_cap,
                     S.min_possible, S.max_lat})
    v.push_back(x);
  // the traced hosts, only when sgn_trace_hosts gave a set (a simulation without one keeps the
  // identity it had before the call existed): their records, seq and rng_pos differ with the set
  if (S.trace_on == 2u) {
    v.push_back(0x7472616365686f73ull);  // "tracehos"
    v.push_back(ctx->trace_hosts.size());
    v.push_back(sgn_digest_bytes(ctx->trace_hosts.data(), ctx->trace_hosts.size() * 4));
  }
  ctx->identity = sgn_digest_bytes(v.data(), v.size() * 8);
  ctx->identity_gen = ctx->sim_gen;
  *out = ctx->identity;
  return 0;
}

void header_base(sgn_ctx* ctx, FileHeader* h) {
  std::memset(h, 0, sizeof(*h));
  std::memcpy(h->magic, kMagic, 8);
  h->format = kFormat;
  h->abi = SGN_ABI_VERSION;
  h->layout_sig = kLayoutSig;
  h->sz_ctrl = sizeof(Ctrl);
  h->sz_hostrec = sizeof(HostRec);
  h->sz_evrec = sizeof(EvRec);
  h->sz_codelent = sizeof(CodelEnt);
  h->sz_fifoent = sizeof(FifoEnt);
  h->sz_drain_rec = sizeof(sgn_drain_rec);
  h->sz_trace_rec = sizeof(sgn_trace_rec);
  h->shard_rank = ctx->rank;
  h->shard_count = ctx->nranks;
  h->traced = ctx->S.trace_on ? 1 : 0;
}

// the sections of snapshot s of simulation S (trace: where its trace records are, n_trace of them)
std::vector<Sec> sections_of(const DevSim& S, const sgn_snapshot* s, const void* trace, uint64_t n_trace) {
  std::vector<Sec> v;
  v.push_back({"ctrl", false, &s->ctrl, sizeof(Ctrl)});
  const auto fixed = state_buffers(S);  // (for the names: the bytes are the snapshot's own)
  const auto pools = pool_buffers(S, s->lay, 0, 0);
  for (size_t k = 0; k < s->fixed.size(); k++) v.push_back({fixed[k].name, true, s->fixed[k].d, s->fixed[k].bytes});
  for (size_t k = 0; k < POOL_N; k++) v.push_back({pools[k].name, true, s->pool[k].d, s->pool[k].bytes});
  v.push_back({kTailNames[SECT_PACKED], true, s->packed.d, s->packed.bytes});
  v.push_back({kTailNames[SECT_HANDLES], false, s->handles.data(), s->handles.size() * 8});
  v.push_back({kTailNames[SECT_SUBMIT_SEQ], false, s->submit_seq.data(), s->submit_seq.size() * 4});
  v.push_back({kTailNames[SECT_DRAIN_HELD], false, s->drain_held.data(), s->drain_held.size() * sizeof(sgn_drain_rec)});
  v.push_back({kTailNames[SECT_H_EXT], false, s->h_ext.data(), s->h_ext.size() * 8});
  v.push_back({kTailNames[SECT_TRACE], true, trace, n_trace * sizeof(sgn_trace_rec)});
  return v;
}

// the digests of a section list: the device sections by one launch, the host ones on the host
int digest_sections(sgn_ctx* ctx, const std::vector<Sec>& secs, std::vector<uint64_t>* dig, float* ms, uint64_t* dev_bytes) {
  std::vector<DigSec> dev;
  for (const Sec& s : secs)
    if (s.dev) dev.push_back(dsec(s.bytes ? s.p : nullptr, s.bytes));
  std::vector<uint64_t> dd(dev.size());
  if (int rc = digest_device(ctx, dev, dd.data(), ms)) return rc;
  dig->assign(secs.size(), 0);
  size_t k = 0;
  *dev_bytes = 0;
  for (size_t i = 0; i < secs.size(); i++) {
    (*dig)[i] = secs[i].dev ? dd[k++] : sgn_digest_bytes(secs[i].p, secs[i].bytes);
    if (secs[i].dev) *dev_bytes += secs[i].bytes;
  }
  return 0;
}

// the file functions' streams
int file_write(void* user, const void* data, size_t len) { return std::fwrite(data, 1, len, (FILE*)user) == len ? 0 : 1; }
int file_read(void* user, void* data, size_t len) { return std::fread(data, 1, len, (FILE*)user) == len ? 0 : 1; }

}  // namespace

// ---- export ----------------------------------------------------------------------------------
namespace {

int export_one(sgn_ctx* ctx, sgn_snapshot* s, sgn_write_fn wr, void* user, uint64_t* bytes_out) {
  const char* what = "sgn_snapshot_export";
  const Clock::time_point t_begin = Clock::now();
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  SGN_HIP(ctx, hipStreamSynchronize(st));
  if (int rc = stage_get(ctx)) return rc;
  report::ReportEvents<2> E;  // one per staging chunk
  if (!E.make()) return set_error(ctx, SGN_EDEVICE, "hipEventCreate failed (snapshot export)");
  FileHeader h;
  header_base(ctx, &h);
  if (int rc = identity(ctx, &h.identity)) return rc;
  // the trace records up to the save that sgn_trace_take has not handed out, [b, N): an imported
  // snapshot's own, else the context's — record p is at trace_buf[p - trace_base], so they start
  // the buffer (b = trace_base) or there are none (a take since the save passed N: b = N). Without
  // a take b = 0 and the section is the records [0, N), as before the call existed. (snap_check has
  // refused a snapshot ahead of the position whose records the buffer no longer holds.)
  const uint64_t trace_b = s->imported ? s->trace_b : std::min<uint64_t>(ctx->trace_base, s->ctrl.trace_n);
  const uint64_t n_trace = s->imported ? s->trace.bytes / sizeof(sgn_trace_rec)
                                       : (ctx->trace_buf ? std::min<uint64_t>(s->ctrl.trace_n - trace_b, ctx->trace_cap) : 0);
  const void* trace = s->imported ? s->trace.d : (const void*)ctx->trace_buf;
  const std::vector<Sec> secs = sections_of(ctx->S, s, trace, n_trace);
  std::vector<uint64_t> dig;
  float dig_ms = 0;
  uint64_t dev_bytes = 0;
  if (int rc = digest_sections(ctx, secs, &dig, &dig_ms, &dev_bytes)) return rc;

  h.rounds = s->ctrl.rounds;
  h.ws = s->ctrl.ws;
  h.we = s->ctrl.we;
  h.lay = s->lay;
  h.counters = s->counters;
  h.calendar_runs = s->runs;
  h.trace_records = n_trace;
  h.reserved = trace_b;
  h.n_sections = secs.size();
  std::vector<TableEnt> tab(secs.size());
  uint64_t total = sizeof(FileHeader) + secs.size() * sizeof(TableEnt) + 8;
  for (size_t i = 0; i < secs.size(); i++) {
    tab[i] = {i + 1, secs[i].bytes, dig[i]};
    total += pad16(secs[i].bytes);
  }
  h.file_bytes = total;

  uint64_t written = 0;
  auto put = [&](const void* p, size_t n) {
    if (n == 0) return true;
    written += n;
    return wr(user, p, n) == 0;
  };
  auto efile = [&]() { return set_error(ctx, SGN_EFILE, std::string(what) + ": the write callback failed"); };
  static const char zeros[16] = {0};
  // header, table; the trailer's digest is over exactly these bytes
  std::vector<unsigned char> head(sizeof(FileHeader) + tab.size() * sizeof(TableEnt));
  std::memcpy(head.data(), &h, sizeof(FileHeader));
  std::memcpy(head.data() + sizeof(FileHeader), tab.data(), tab.size() * sizeof(TableEnt));
  if (!put(&h, sizeof(FileHeader)) || !put(tab.data(), tab.size() * sizeof(TableEnt))) return efile();
  const Clock::time_point t_stream = Clock::now();
  for (const Sec& sc : secs) {
    if (!sc.dev) {
      if (!put(sc.p, sc.bytes) || !put(zeros, pad16(sc.bytes) - sc.bytes)) return efile();
      continue;
    }
    // device -> chunk k & 1 -> callback: the copy into one chunk runs while the other is written
    const uint64_t n_chunks = (sc.bytes + kChunk - 1) / kChunk;
    auto chunk_len = [&](uint64_t k) { return (size_t)std::min<uint64_t>(kChunk, sc.bytes - k * kChunk); };
    auto flush = [&](uint64_t k) {  // chunk k has been copied: write it (the section's last one with its padding)
      if (hipEventSynchronize(E.ev[k & 1]) != hipSuccess) return -1;
      size_t len = chunk_len(k);
      char* b = (char*)ctx->file_stage[k & 1];
      if (k + 1 == n_chunks) {
        std::memset(b + len, 0, pad16(len) - len);
        len = pad16(len);
      }
      return put(b, len) ? 0 : 1;
    };
    for (uint64_t k = 0; k < n_chunks; k++) {
      if (hipMemcpyAsync(ctx->file_stage[k & 1], (const char*)sc.p + k * kChunk, chunk_len(k), hipMemcpyDeviceToHost, st) !=
              hipSuccess ||
          hipEventRecord(E.ev[k & 1], st) != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return set_error(ctx, SGN_EDEVICE, std::string(what) + ": a device copy failed");
      }
      if (k) {
        const int f = flush(k - 1);
        if (f) {
          (void)hipStreamSynchronize(st);  // (the copy in flight targets a chunk the context keeps)
          return f < 0 ? set_error(ctx, SGN_EDEVICE, std::string(what) + ": a device copy failed") : efile();
        }
      }
    }
    if (n_chunks) {
      const int f = flush(n_chunks - 1);
      if (f) return f < 0 ? set_error(ctx, SGN_EDEVICE, std::string(what) + ": a device copy failed") : efile();
    }
  }
  const double stream_ms = ms_since(t_stream);
  const uint64_t trailer = sgn_digest_bytes(head.data(), head.size());
  if (!put(&trailer, 8)) return efile();
  if (written != total) return set_error(ctx, SGN_ESTATE, std::string(what) + ": internal size mismatch");
  if (bytes_out) *bytes_out = written;
  ctx->file_timing = {ms_since(t_begin), stream_ms, (double)dig_ms, dev_bytes, written};
  return 0;
}

}  // namespace

// ---- import ----------------------------------------------------------------------------------
namespace {

int import_one(sgn_ctx* ctx, sgn_read_fn rd, void* user, sgn_snapshot** out) {
  const std::string w = "sgn_snapshot_import: ";
  const Clock::time_point t_begin = Clock::now();
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = stage_get(ctx)) return rc;
  const DevSim& S = ctx->S;
  const uint64_t nH = S.nH, n_slabs = (uint64_t)(S.NB + 1) * S.G;
  auto efile = [&](const std::string& m) { return set_error(ctx, SGN_EFILE, w + m); };

  // ---- header: the file must come from this library build and this simulation
  FileHeader h;
  if (rd(user, &h, sizeof(h)) != 0) return efile("truncated in the header");
  if (std::memcmp(h.magic, kMagic, 8) != 0) return efile("not a snapshot file (magic)");
  FileHeader want;
  header_base(ctx, &want);
  if (int rc = identity(ctx, &want.identity)) return rc;
  {
    struct F {
      const char* name;
      uint64_t got, want;
      const char* whose;
    };
    const F fields[] = {
        {"format", h.format, want.format, "library"},
        {"abi", h.abi, want.abi, "library"},
        {"layout_sig", h.layout_sig, want.layout_sig, "library"},
        {"sizeof(Ctrl)", h.sz_ctrl, want.sz_ctrl, "library"},
        {"sizeof(HostRec)", h.sz_hostrec, want.sz_hostrec, "library"},
        {"sizeof(EvRec)", h.sz_evrec, want.sz_evrec, "library"},
        {"sizeof(CodelEnt)", h.sz_codelent, want.sz_codelent, "library"},
        {"sizeof(FifoEnt)", h.sz_fifoent, want.sz_fifoent, "library"},
        {"sizeof(sgn_drain_rec)", h.sz_drain_rec, want.sz_drain_rec, "library"},
        {"sizeof(sgn_trace_rec)", h.sz_trace_rec, want.sz_trace_rec, "library"},
        {"shard_rank", h.shard_rank, want.shard_rank, "context"},
        {"shard_count", h.shard_count, want.shard_count, "context"},
        {"identity", h.identity, want.identity, "simulation"},
    };
    for (const F& f : fields)
      if (f.got != f.want)
        return set_error(ctx, SGN_EINVAL, w + "header field " + f.name + " is " + std::to_string(f.got) + ", this " + f.whose +
                                              " has " + std::to_string(f.want));
  }
  // the trace: records need a buffer that holds them (and a traced simulation's sections differ)
  if (h.traced != want.traced || (h.trace_records && (!ctx->trace_buf || ctx->trace_cap < h.trace_records)))
    return set_error(ctx, SGN_ESTATE, w + (h.traced ? "the file has trace records and this context's trace buffer does not hold them "
                                                        "(sgn_trace_enable before sgn_sim_init)"
                                                      : "the file is of an untraced simulation and this context keeps a trace"));
  // the layout scalars: bounded before anything is sized from them
  const uint32_t cap_lim = std::max(S.CAP, max_slab_capacity(ctx, S));
  const SnapLayout& Z = h.lay;
  if (Z.cap == 0 || Z.cap > cap_lim) return efile("slab capacity outside what this device's round kernels hold");
  if (Z.cq_pages < nH || Z.cq_pages >= (1ULL << 28)) return efile("CoDel page count out of range");
  if (Z.spill_cap == 0 || Z.spill_cap > (1ULL << 28)) return efile("spill area capacity out of range");
  if (Z.ext_total >= (1ULL << 40)) return efile("slab extension total out of range");
  if (Z.gspec > 64 || Z.gspec > Z.cap) return efile("gather width out of range");
  if (h.calendar_runs > n_slabs * Z.cap + Z.ext_total) return efile("more calendar runs than the layout holds");
  const auto fixed = state_buffers(S);
  const size_t P0 = SEC_FIXED + fixed.size(), T0 = P0 + POOL_N;  // the first pool section, the first after the pools
  const size_t n_sec = T0 + SECT_N;
  if (h.n_sections != n_sec) return efile("section count");

  // ---- table: every size follows from the simulation and the header
  std::vector<TableEnt> tab(n_sec);
  if (rd(user, tab.data(), n_sec * sizeof(TableEnt)) != 0) return efile("truncated in the section table");
  // the pools at the header's layout: nothing in the spill area (a snapshot is of a resolved round
  // edge), and as many undrained records as the drain section says it holds
  const uint64_t n_drain = tab[P0 + POOL_DRAIN].bytes / sizeof(sgn_drain_rec);
  const auto pools = pool_buffers(S, Z, 0, n_drain);
  auto name_of = [&](size_t i) -> std::string {
    return i == SEC_CTRL ? "ctrl" : i < P0 ? fixed[i - SEC_FIXED].name : i < T0 ? pools[i - P0].name : kTailNames[i - T0];
  };
  uint64_t total = sizeof(FileHeader) + n_sec * sizeof(TableEnt) + 8;
  for (size_t i = 0; i < n_sec; i++) {
    if (tab[i].id != i + 1) return efile("section table: id of section " + name_of(i));
    if (tab[i].bytes % 4 || tab[i].bytes > (1ULL << 44)) return efile("section table: size of section " + name_of(i));
    total += pad16(tab[i].bytes);
  }
  if (total != h.file_bytes) return efile("section sizes do not add up to the file length");
  auto size_is = [&](size_t i, uint64_t bytes) { return tab[i].bytes == bytes; };
  auto bad_size = [&](size_t i) { return efile("section " + name_of(i) + " has a size this simulation's layout does not give"); };
  if (!size_is(SEC_CTRL, sizeof(Ctrl))) return bad_size(SEC_CTRL);
  for (size_t k = 0; k < fixed.size(); k++)
    if (!size_is(SEC_FIXED + k, fixed[k].bytes)) return bad_size(SEC_FIXED + k);
  for (size_t k = 0; k < POOL_N; k++)  // (drain: whole records, no more than this context's buffer holds)
    if (!size_is(P0 + k, pools[k].bytes) || (k == POOL_DRAIN && n_drain > S.drain_cap)) return bad_size(P0 + k);
  if (tab[T0 + SECT_PACKED].bytes % 32 || !size_is(T0 + SECT_PACKED, h.calendar_runs * sizeof(EvRec))) return bad_size(T0 + SECT_PACKED);
  if (tab[T0 + SECT_HANDLES].bytes % 8 || tab[T0 + SECT_HANDLES].bytes / 8 > SGN_TAG_SLOT_MASK + 1ull) return bad_size(T0 + SECT_HANDLES);
  if (!size_is(T0 + SECT_SUBMIT_SEQ, nH * 4)) return bad_size(T0 + SECT_SUBMIT_SEQ);
  if (tab[T0 + SECT_DRAIN_HELD].bytes % sizeof(sgn_drain_rec)) return bad_size(T0 + SECT_DRAIN_HELD);
  if (!size_is(T0 + SECT_H_EXT, 0) && !size_is(T0 + SECT_H_EXT, n_slabs * 8)) return bad_size(T0 + SECT_H_EXT);
  if (!size_is(T0 + SECT_TRACE, h.trace_records * sizeof(sgn_trace_rec))) return bad_size(T0 + SECT_TRACE);
  if (size_is(T0 + SECT_H_EXT, 0) && Z.ext_total) return efile("slab extensions without their table");

  // ---- the snapshot's buffers, then the payloads into them
  sgn_snapshot* s = new sgn_snapshot();
  uint64_t* d_ext = nullptr;  // the extension table on the device, for the scan
  auto fail = [&](int code, const std::string& m) {
    (void)hipStreamSynchronize(st);
    if (d_ext) (void)hipFree(d_ext);
    snap_release(s);
    return set_error(ctx, code, m);
  };
  s->lay = Z;  // (bounded above; restore reads it)
  s->fixed.resize(fixed.size());
  bool ok = true;
  for (size_t k = 0; ok && k < fixed.size(); k++) ok = snap_buf_alloc(&s->fixed[k], tab[SEC_FIXED + k].bytes);
  for (size_t k = 0; ok && k < POOL_N; k++) ok = snap_buf_alloc(&s->pool[k], tab[P0 + k].bytes);
  ok = ok && snap_buf_alloc(&s->packed, tab[T0 + SECT_PACKED].bytes) && snap_buf_alloc(&s->trace, tab[T0 + SECT_TRACE].bytes);
  if (!ok) return fail(SGN_ENOMEM, "device allocation failed (snapshot import)");
  try {
    s->handles.resize(tab[T0 + SECT_HANDLES].bytes / 8);
    s->submit_seq.resize(tab[T0 + SECT_SUBMIT_SEQ].bytes / 4);
    s->drain_held.resize(tab[T0 + SECT_DRAIN_HELD].bytes / sizeof(sgn_drain_rec));
    s->h_ext.resize(tab[T0 + SECT_H_EXT].bytes / 8);
  } catch (const std::bad_alloc&) {
    return fail(SGN_ENOMEM, "host allocation failed (snapshot import)");
  }
  report::ReportEvents<2> E;  // one per staging chunk
  if (!E.make()) return fail(SGN_EDEVICE, "hipEventCreate failed (snapshot import)");
  std::vector<Sec> secs = sections_of(S, s, s->trace.d, h.trace_records);  // (the same list export walks)
  const Clock::time_point t_stream = Clock::now();
  bool used[2] = {false, false};
  char padbuf[16];
  for (size_t i = 0; i < n_sec; i++) {
    const Sec& sc = secs[i];
    const std::string trunc = "truncated in section " + sc.name;
    if (!sc.dev) {
      if ((sc.bytes && rd(user, const_cast<void*>(sc.p), sc.bytes) != 0) ||
          (pad16(sc.bytes) != sc.bytes && rd(user, padbuf, pad16(sc.bytes) - sc.bytes) != 0))
        return fail(SGN_EFILE, w + trunc);
      continue;
    }
    // callback -> chunk k & 1 -> device: the upload of one chunk runs while the other is filled
    const uint64_t n_chunks = (sc.bytes + kChunk - 1) / kChunk;
    for (uint64_t k = 0; k < n_chunks; k++) {
      const size_t len = (size_t)std::min<uint64_t>(kChunk, sc.bytes - k * kChunk);
      const size_t rlen = k + 1 == n_chunks ? (size_t)pad16(len) : len;
      const uint32_t b = (uint32_t)(k & 1);
      if (used[b] && hipEventSynchronize(E.ev[b]) != hipSuccess) return fail(SGN_EDEVICE, w + "a device copy failed");
      if (rd(user, ctx->file_stage[b], rlen) != 0) return fail(SGN_EFILE, w + trunc);
      if (hipMemcpyAsync((char*)const_cast<void*>(sc.p) + k * kChunk, ctx->file_stage[b], len, hipMemcpyHostToDevice, st) !=
              hipSuccess ||
          hipEventRecord(E.ev[b], st) != hipSuccess)
        return fail(SGN_EDEVICE, w + "a device copy failed");
      used[b] = true;
    }
  }
  uint64_t trailer = 0;
  if (rd(user, &trailer, 8) != 0) return fail(SGN_EFILE, w + "truncated before the trailer");
  if (hipStreamSynchronize(st) != hipSuccess) return fail(SGN_EDEVICE, w + "a device copy failed");
  const double stream_ms = ms_since(t_stream);

  // ---- integrity: the trailer over header and table, then every section against the table
  {
    std::vector<unsigned char> head(sizeof(FileHeader) + n_sec * sizeof(TableEnt));
    std::memcpy(head.data(), &h, sizeof(FileHeader));
    std::memcpy(head.data() + sizeof(FileHeader), tab.data(), n_sec * sizeof(TableEnt));
    if (sgn_digest_bytes(head.data(), head.size()) != trailer) return fail(SGN_EFILE, w + "the header's digest does not match (trailer)");
  }
  std::vector<uint64_t> dig;
  float dig_ms = 0;
  uint64_t dev_bytes = 0;
  if (int rc = digest_sections(ctx, secs, &dig, &dig_ms, &dev_bytes)) return fail(rc, ctx->err);
  for (size_t i = 0; i < n_sec; i++)
    if (dig[i] != tab[i].digest) return fail(SGN_EFILE, w + "section " + secs[i].name + " is corrupt (digest mismatch)");

  // ---- consistency: what the restore will trust
  const Ctrl& c = s->ctrl;
  if (c.rounds != h.rounds || c.ws != h.ws || c.we != h.we) return fail(SGN_EFILE, w + "the control block is of another round edge than the header");
  if (c.spill_n || c.hold) return fail(SGN_EFILE, w + "the control block is not of a resolved round edge");
  if (c.keep_slab > S.NB) return fail(SGN_EFILE, w + "the control block's spare slab is outside the calendar");
  if (n_drain != (S.drain ? std::min<uint64_t>(c.drain_n, S.drain_cap) : 0))
    return fail(SGN_EFILE, w + "section drain does not hold the control block's record count");
  // (the section holds the records [reserved, trace_n) that sgn_trace_take had not handed out)
  if (h.reserved > c.trace_n || h.trace_records > c.trace_n - h.reserved || (!h.traced && h.reserved))
    return fail(SGN_EFILE, w + "more trace records than the control block counts");
  {  // the extension table: every extension inside the extension pool
    uint64_t n_ext = 0;
    for (uint64_t e : s->h_ext) {
      if (!e) continue;
      n_ext++;
      if ((e & EXT_OFF_MASK) + (e >> 40) > Z.ext_total) return fail(SGN_EFILE, w + "a slab extension lies outside the extension pool");
    }
    if (n_ext != h.counters.ext_slabs) return fail(SGN_EFILE, w + "the extension table disagrees with the header's count");
  }
  {  // the scan k_snap_copy<unpack> trusts: the imported fills must add up to the packed runs
    if (!s->h_ext.empty()) {
      if (hipMalloc((void**)&d_ext, n_slabs * 8) != hipSuccess) return fail(SGN_ENOMEM, "device allocation failed (snapshot import)");
      if (hipMemcpy(d_ext, s->h_ext.data(), n_slabs * 8, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SGN_EDEVICE, w + "a device copy failed");
    }
    uint64_t scan_total = 0;
    const uint32_t* fills = (const uint32_t*)snap_fixed(s, S, (const void*)S.slab_n)->d;
    if (int rc = snap_scan_total(ctx, fills, d_ext, (uint32_t)Z.cap, n_slabs, &scan_total))
      return fail(rc, ctx->err);
    if (scan_total != h.calendar_runs)
      return fail(SGN_EFILE, w + "the slab fills add up to " + std::to_string(scan_total) + " runs, the packed calendar holds " +
                                 std::to_string(h.calendar_runs));
    if (d_ext) (void)hipFree(d_ext);
    d_ext = nullptr;
  }

  // ---- a snapshot of this context, as sgn_snapshot_save would have left it
  s->ctx = ctx;
  s->gen = ctx->sim_gen;
  s->runs = h.calendar_runs;
  s->imported = true;
  s->trace_b = h.reserved;
  s->counters = h.counters;
  snap_fill_info(s, n_slabs);
  s->info.save_ms = s->info.pack_ms = 0;
  ctx->snapshots.push_back(s);
  *out = s;
  ctx->file_timing = {ms_since(t_begin), stream_ms, (double)dig_ms, dev_bytes, h.file_bytes};
  return 0;
}

}  // namespace

extern "C" {

uint64_t sgn_digest_bytes(const void* p, size_t len) {
  if (len % 4 || (!p && len)) return 0;
  const unsigned char* b = (const unsigned char*)p;
  uint64_t d = sgn_mix64((uint64_t)len ^ SGN_DIGEST_SEED);
  const size_t full = len / 8;
  for (size_t j = 0; j < full; j++) {
    uint64_t w;
    std::memcpy(&w, b + 8 * j, 8);  // little-endian host
    d += sgn_mix64(w ^ (kGold * (uint64_t)(j + 1)));
  }
  if (len & 4) {
    uint32_t w;
    std::memcpy(&w, b + 8 * full, 4);
    d += sgn_mix64((uint64_t)w ^ (kGold * (uint64_t)(full + 1)));
  }
  return d;
}

int sgn_selftest_digest(sgn_ctx* ctx, const void* host_bytes, size_t len, uint64_t* out) {
  if (!ctx || !out || (!host_bytes && len)) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_selftest_digest: null argument") : SGN_EINVAL;
  if (len % 4) return set_error(ctx, SGN_EINVAL, "sgn_selftest_digest: len must be a multiple of 4");
  SGN_HIP(ctx, hipSetDevice(ctx->device));
  void* d = nullptr;
  if (len) {
    if (hipMalloc(&d, len) != hipSuccess) return set_error(ctx, SGN_ENOMEM, "device allocation failed (digest)");
    if (hipMemcpy(d, host_bytes, len, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      return set_error(ctx, SGN_EDEVICE, "sgn_selftest_digest: upload failed");
    }
  }
  const int rc = digest_device(ctx, {dsec(d, len)}, out);
  if (d) (void)hipFree(d);
  return rc;
}

int sgn_snapshot_export(sgn_ctx* ctx, const sgn_snapshot* snap, sgn_write_fn write, void* user, uint64_t* bytes) {
  if (bytes) *bytes = 0;
  if (!ctx || !snap || !write) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_snapshot_export: null argument") : SGN_EINVAL;
  sgn_snapshot* s = nullptr;
  if (int rc = snap_check(ctx, snap, "sgn_snapshot_export", &s)) return rc;
  return export_one(ctx, s, write, user, bytes);
}

int sgn_snapshot_import(sgn_ctx* ctx, sgn_read_fn read, void* user, sgn_snapshot** out) {
  if (out) *out = nullptr;
  if (!ctx || !read || !out) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_snapshot_import: null argument") : SGN_EINVAL;
  if (!ctx->sim_ready) return set_error(ctx, SGN_ESTATE, "no simulation");
  if (!ctx->failed.empty()) return set_error(ctx, SGN_ESTATE, "simulation unusable: " + ctx->failed);
  return import_one(ctx, read, user, out);
}

int sgn_snapshot_export_file(sgn_ctx* ctx, const sgn_snapshot* snap, const char* path, uint64_t* bytes) {
  if (bytes) *bytes = 0;
  if (!ctx || !snap || !path) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_snapshot_export_file: null argument") : SGN_EINVAL;
  const std::string tmp = std::string(path) + ".tmp";
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) return set_error(ctx, SGN_EFILE, "sgn_snapshot_export_file: cannot create " + tmp);
  int rc = sgn_snapshot_export(ctx, snap, file_write, f, bytes);
  if (std::fclose(f) != 0 && !rc) rc = set_error(ctx, SGN_EFILE, "sgn_snapshot_export_file: closing " + tmp + " failed");
  if (!rc && std::rename(tmp.c_str(), path) != 0) rc = set_error(ctx, SGN_EFILE, std::string("sgn_snapshot_export_file: cannot rename to ") + path);
  if (rc) {
    (void)std::remove(tmp.c_str());
    if (bytes) *bytes = 0;
  }
  return rc;
}

int sgn_snapshot_import_file(sgn_ctx* ctx, const char* path, sgn_snapshot** out) {
  if (out) *out = nullptr;
  if (!ctx || !path || !out) return ctx ? set_error(ctx, SGN_EINVAL, "sgn_snapshot_import_file: null argument") : SGN_EINVAL;
  FILE* f = std::fopen(path, "rb");
  if (!f) return set_error(ctx, SGN_ENOENT, std::string("sgn_snapshot_import_file: cannot open ") + path);
  const int rc = sgn_snapshot_import(ctx, file_read, f, out);
  std::fclose(f);
  return rc;
}

int sgn_snapshot_file_info_get(const char* path, sgn_snapshot_file_info* out) {
  if (!path || !out) return SGN_EINVAL;
  std::memset(out, 0, sizeof(*out));
  FILE* f = std::fopen(path, "rb");
  if (!f) return SGN_ENOENT;
  FileHeader h;
  int rc = SGN_EFILE;
  do {
    if (std::fread(&h, 1, sizeof(h), f) != sizeof(h) || std::memcmp(h.magic, kMagic, 8) != 0) break;
    if (h.n_sections == 0 || h.n_sections > 4096) break;
    std::vector<unsigned char> head(sizeof(FileHeader) + (size_t)h.n_sections * sizeof(TableEnt));
    std::memcpy(head.data(), &h, sizeof(h));
    if (std::fread(head.data() + sizeof(h), 1, head.size() - sizeof(h), f) != head.size() - sizeof(h)) break;
    uint64_t trailer = 0;
    if (std::fseek(f, 0, SEEK_END) != 0 || (uint64_t)std::ftell(f) != h.file_bytes) break;
    if (h.file_bytes < head.size() + 8 || std::fseek(f, -8, SEEK_END) != 0 || std::fread(&trailer, 1, 8, f) != 8) break;
    if (trailer != sgn_digest_bytes(head.data(), head.size())) break;
    rc = 0;
  } while (false);
  std::fclose(f);
  if (rc) return rc;
  out->format = h.format;
  out->abi = h.abi;
  out->layout_sig = h.layout_sig;
  out->identity = h.identity;
  out->rounds = h.rounds;
  out->window_start = h.ws;
  out->window_end = h.we;
  out->file_bytes = h.file_bytes;
  out->n_sections = h.n_sections;
  out->calendar_runs = h.calendar_runs;
  out->trace_records = h.trace_records;
  out->shard_rank = (uint32_t)h.shard_rank;
  out->shard_count = (uint32_t)h.shard_count;
  return 0;
}

int sgn_snapshot_file_timing_get(sgn_ctx* ctx, sgn_snapshot_file_timing* out) {
  if (!ctx || !out) return SGN_EINVAL;
  *out = ctx->file_timing;
  return 0;
}

}  // extern "C"

uint64_t sgn::layout_sig_snapshot_file() { return kLayoutSig; }
